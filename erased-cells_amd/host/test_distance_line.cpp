// test_distance_line.cpp — csrc/ec_distance_line.hpp alone, under a plain C++ compiler: the column sweeps and the row scans that the
// kernels of ec_distance run, against brute force (the minimum over all targets, in integers) over EVERY mask of every shape up to
// 4 x 4 and random masks up to 40 x 40.  The rows are scanned the way the kernel scans them: in pieces of a tile's width, with the
// stacks of several rows interleaved in one block, and g read through a stride.  Also the workspace's layout, and ec_distance's
// refusals in the order include/erased_cells.h states.  Built plainly and with -fsanitize=address,undefined (every stack and g plane
// is an exactly sized heap block, so a step outside one is reported).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "ec_distance_line.hpp"

using namespace ecd;

static long checks = 0, failures = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        ++checks;                                                                   \
        if (!(c)) {                                                                 \
            if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                           \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// d2 by brute force; kDistNone without a target
static std::vector<uint32_t> brute(const std::vector<uint8_t>& m, uint32_t cols, uint32_t rows) {
    std::vector<uint32_t> out(size_t(cols) * rows, kDistNone);
    for (uint32_t i = 0; i < rows; ++i)
        for (uint32_t j = 0; j < cols; ++j)
            for (uint32_t y = 0; y < rows; ++y)
                for (uint32_t x = 0; x < cols; ++x)
                    if (m[size_t(y) * cols + x]) {
                        const int32_t dy = int32_t(i) - int32_t(y), dx = int32_t(j) - int32_t(x);
                        const uint32_t d = uint32_t(dy * dy + dx * dx);
                        if (d < out[size_t(i) * cols + j]) out[size_t(i) * cols + j] = d;
                    }
    return out;
}

// the transform as the kernels make it: `piece` columns of a row at a time, `lanes` rows sharing one stack block
static std::vector<uint32_t> two_phase(const std::vector<uint8_t>& m, uint32_t cols, uint32_t rows, uint32_t piece, uint32_t lanes) {
    std::vector<uint16_t> g(size_t(cols) * rows);
    for (uint32_t x = 0; x < cols; ++x) {
        distance_column_down(m.data() + x, cols, rows, g.data() + x, cols);
        distance_column_up(g.data() + x, cols, rows);
    }
    std::vector<uint32_t> out(size_t(cols) * rows);
    const uint32_t waves = (rows + lanes - 1) / lanes;
    std::vector<uint16_t> S(size_t(waves) * lanes * cols), T(size_t(waves) * lanes * cols);
    for (uint32_t y = 0; y < rows; ++y) {
        const size_t at = size_t(y / lanes) * lanes * cols + y % lanes;
        const uint16_t* grow = g.data() + size_t(y) * cols;
        DistEnvelope e;
        for (uint32_t x0 = 0; x0 < cols; x0 += piece) {
            const uint32_t n = cols - x0 < piece ? cols - x0 : piece;
            distance_row_forward(e, grow + x0, 1, x0, n, cols, S.data() + at, T.data() + at, lanes, grow, 1);
        }
        const uint32_t pieces = (cols + piece - 1) / piece;
        for (uint32_t p = pieces; p-- > 0;) {
            const uint32_t x0 = p * piece, n = cols - x0 < piece ? cols - x0 : piece;
            distance_row_backward(e, x0, n, out.data() + size_t(y) * cols + x0, 1, S.data() + at, T.data() + at, lanes, grow, 1);
        }
        CHECK(e.q == -1);  // the bottom entry starts at column 0: the backward scan empties the stack
    }
    return out;
}

static void one(const std::vector<uint8_t>& m, uint32_t cols, uint32_t rows) {
    const std::vector<uint32_t> want = brute(m, cols, rows);
    const uint32_t pieces[3] = {cols, 1, 3};
    for (int k = 0; k < 3; ++k) {
        const std::vector<uint32_t> got = two_phase(m, cols, rows, pieces[k], k == 0 ? 1 : 3);
        bool same = true;
        for (size_t c = 0; c < want.size(); ++c) same = same && got[c] == want[c];
        CHECK(same);
    }
}

// ec_distance's refusals.  Addresses are plain integers, never dereferenced.
static const void* at(uint64_t a) { return reinterpret_cast<const void*>(uintptr_t(a)); }
static bool says(const ecv::Refusal& r, const char* text, bool bad_type = false) {
    return r.why && std::string_view(r.why) == text && r.bad_type == bad_type;
}

static void refusals() {
    const uint64_t M = 0x10000, D = 0x20000, E = D + 400, FAR = uint64_t(1) << 40, W = dist_workspace_bytes(10, 10);  // 10 x 10 cells of 4 bytes
    const void* far = at(FAR);
    CHECK(W > 0 && W % 16 == 0);
    CHECK(!distance_refusal(at(M), 10, 10, true, 4, at(D), at(E), far) && !distance_refusal(at(M), 10, 10, true, 8, at(D), nullptr, nullptr));
    CHECK(!distance_refusal(at(M), 10, 10, true, 4, nullptr, at(E), nullptr));
    // the order: each call is wrong in everything that comes later as well
    CHECK(says(distance_refusal(nullptr, 0, 10, false, 0, nullptr, nullptr, nullptr), "cols and rows must be within 1 .. EC_DISTANCE_MAX_SIDE"));
    CHECK(says(distance_refusal(nullptr, 10, 0, false, 0, nullptr, nullptr, nullptr), "cols and rows must be within 1 .. EC_DISTANCE_MAX_SIDE"));
    CHECK(says(distance_refusal(nullptr, 10, 10, false, 0, nullptr, nullptr, nullptr), "bad out_type", true));
    CHECK(says(distance_refusal(nullptr, 10, 10, true, 0, nullptr, nullptr, nullptr), "out_type is neither EC_U32 nor EC_F64"));
    CHECK(says(distance_refusal(nullptr, 10, 10, true, 4, nullptr, nullptr, nullptr), "null mask"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, nullptr, nullptr, at(M)), "dst and dst_mask are both NULL"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(M + 2), at(M), at(M)), "dst is not aligned to its cell type"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 8, at(M + 4), at(M), at(M)), "dst is not aligned to its cell type"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(M), at(M), at(M)), "dst overlaps the mask"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(M), at(M)), "dst_mask overlaps the mask"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(D), at(M)), "the workspace overlaps the mask"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(D), at(D)), "dst_mask overlaps dst"));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(E), at(E - 1)), "the workspace overlaps dst"));  // its second byte on dst_mask
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(E), at(E + 99)), "the workspace overlaps dst_mask"));
    // each overlap by one byte, and the same two blocks touching
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(M + 96), nullptr, far), "dst overlaps the mask") &&
          !distance_refusal(at(M), 10, 10, true, 4, at(M + 100), nullptr, far));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(M - 396), nullptr, far), "dst overlaps the mask") &&
          !distance_refusal(at(M), 10, 10, true, 4, at(M - 400), nullptr, far));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(M + 99), far), "dst_mask overlaps the mask") &&
          !distance_refusal(at(M), 10, 10, true, 4, at(D), at(M + 100), far));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(E), at(M - W + 1)), "the workspace overlaps the mask") &&
          !distance_refusal(at(M), 10, 10, true, 4, at(D), at(E), at(M - W)));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(E - 1), far), "dst_mask overlaps dst") &&
          !distance_refusal(at(M), 10, 10, true, 4, at(D), at(E), far));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), nullptr, at(D + 399)), "the workspace overlaps dst") &&
          !distance_refusal(at(M), 10, 10, true, 4, at(D), nullptr, at(D + 400)));
    CHECK(says(distance_refusal(at(M), 10, 10, true, 4, at(D), at(E), at(E - W + 1)), "the workspace overlaps dst") &&  // ends on dst's last byte
          says(distance_refusal(at(M), 10, 10, true, 4, nullptr, at(E), at(E - W + 1)), "the workspace overlaps dst_mask") &&
          !distance_refusal(at(M), 10, 10, true, 4, nullptr, at(E), at(E - W)) && !distance_refusal(at(M), 10, 10, true, 4, nullptr, at(E), at(E + 100)));
    // the largest shape, and one past it: 2^30 cells, every product in 64 bits
    const uint64_t S = kDistMaxSide, N = S * S, WS = dist_workspace_bytes(S, S);
    CHECK(WS >= 6 * N && WS > (uint64_t(1) << 32));
    CHECK(!distance_refusal(far, S, S, true, 8, at(FAR + N), at(FAR + 9 * N), at(FAR + 10 * N)));
    CHECK(says(distance_refusal(far, S, S, true, 8, at(FAR + N - 8), nullptr, nullptr), "dst overlaps the mask"));
    CHECK(says(distance_refusal(far, S, S, true, 8, at(FAR + N), at(FAR + 9 * N - 1), nullptr), "dst_mask overlaps dst"));
    CHECK(says(distance_refusal(far, S, S, true, 8, at(FAR + N), at(FAR + 9 * N), at(FAR - WS + 1)), "the workspace overlaps the mask") &&
          !distance_refusal(far, S, S, true, 8, at(FAR + N), at(FAR + 9 * N), at(FAR - WS)));
    CHECK(says(distance_refusal(far, S, S, true, 8, at(FAR + N), at(FAR + 9 * N), at(FAR + 10 * N - 1)), "the workspace overlaps dst_mask"));
    CHECK(says(distance_refusal(far, S + 1, S, true, 8, far, far, far), "cols and rows must be within 1 .. EC_DISTANCE_MAX_SIDE") &&
          says(distance_refusal(far, S, S + 1, true, 8, far, far, far), "cols and rows must be within 1 .. EC_DISTANCE_MAX_SIDE") &&
          says(distance_refusal(far, 1, uint64_t(1) << 63, true, 8, far, far, far), "cols and rows must be within 1 .. EC_DISTANCE_MAX_SIDE"));
}

int main() {
    refusals();
    // every mask of every shape up to 4 x 4
    for (uint32_t rows = 1; rows <= 4; ++rows)
        for (uint32_t cols = 1; cols <= 4; ++cols) {
            const uint32_t n = rows * cols;
            std::vector<uint8_t> m(n);
            for (uint32_t bits = 0; bits < (1u << n); ++bits) {
                for (uint32_t c = 0; c < n; ++c) m[c] = (bits >> c) & 1u ? uint8_t(1 + (c * 85u) % 255u) : uint8_t(0);
                one(m, cols, rows);
            }
        }
    // random masks up to 40 x 40 at several densities, among them one target and none
    for (int trial = 0; trial < 300; ++trial) {
        const uint32_t cols = 1 + uint32_t(rng() % 40), rows = 1 + uint32_t(rng() % 40);
        const uint32_t per_thousand[6] = {500, 100, 10, 2, 900, 0};
        const uint32_t density = per_thousand[trial % 6];
        std::vector<uint8_t> m(size_t(cols) * rows);
        for (auto& b : m) b = rng() % 1000 < density ? uint8_t(1 + rng() % 255) : uint8_t(0);
        if (trial % 6 == 3) m[rng() % m.size()] = 0xFF;
        one(m, cols, rows);
    }
    // the cell as stored
    CHECK(!dist_valid(kDistNone, 0xFFFFFFFFu) && dist_valid(0, 0) && !dist_valid(1, 0) && dist_valid(5, 5) && !dist_valid(6, 5));
    CHECK(dist_valid(2u * 32767u * 32767u, 0xFFFFFFFFu));
    // the workspace: g, then the two stacks, 16-byte aligned, nothing for a refused shape
    CHECK(dist_workspace_bytes(0, 5) == 0 && dist_workspace_bytes(5, 0) == 0 && dist_workspace_bytes(32769, 1) == 0 && dist_workspace_bytes(1, 32769) == 0);
    for (uint64_t cols : {1ull, 7ull, 64ull, 65ull, 32768ull})
        for (uint64_t rows : {1ull, 63ull, 64ull, 65ull, 32768ull}) {
            const DistWorkspace w = dist_workspace(cols, rows);
            const size_t stack = size_t((rows + kDistLines - 1) / kDistLines) * kDistLines * cols * 2;
            CHECK(w.off_s % 16 == 0 && w.off_t % 16 == 0 && w.bytes % 16 == 0);
            CHECK(w.off_s >= cols * rows * 2 && w.off_t >= w.off_s + stack && w.bytes >= w.off_t + stack && w.bytes < w.off_t + stack + 16);
            CHECK(dist_workspace_bytes(cols, rows) == w.bytes);
        }
    if (failures) {
        std::printf("%ld of %ld checks FAILED\n", failures, checks);
        return 1;
    }
    std::printf("%ld checks passed\n", checks);
    return 0;
}
