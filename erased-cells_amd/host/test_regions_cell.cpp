// test_regions_cell.cpp — csrc/ec_regions_cell.hpp alone, under a plain C++ compiler: the phases of ec_regions as the kernels run
// them (tiles, seams, flatten, sizes, numbers, the stored cell), with small tiles so that small rasters have many seams, against a
// flood fill in raster order.
//   (a) sequentially, on plain words: EVERY mask of every shape up to 4 x 4, and random class rasters up to 40 x 40 with masks, both
//       connectivities, both numberings, several sieves and tile shapes.  Also with loads that are STALE on purpose — a load returns
//       any value the word has held — which may cost rounds and must not cost an answer.  And the workspace's layout, and ec_regions'
//       refusals in the order include/erased_cells.h states.
//   (b) the seam unions on std::atomic words from up to 16 std::threads in shuffled order: the same answers, and every loop's step
//       count under the bound the header states.
// Built plainly, with -fsanitize=address,undefined, and with -fsanitize=thread for (b).
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <thread>
#include <vector>

#include "ec_regions_cell.hpp"

using namespace ecd;

static std::atomic<long> checks{0}, failures{0};
#define CHECK(c)                                                                          \
    do {                                                                                  \
        ++checks;                                                                         \
        if (!(c)) {                                                                       \
            if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Answer {
    std::vector<uint32_t> label;
    uint64_t k = 0;
    bool operator==(const Answer& o) const { return k == o.k && label == o.label; }
};

// the rule, by flood fill from every unvisited valid cell in raster order
template <typename W>
static Answer flood(const RegRaster<W>& r, bool eight, bool dense, uint64_t min_cells) {
    const uint32_t n = r.cols * r.rows;
    std::vector<int64_t> root(n, -1);
    Answer a;
    a.label.assign(n, 0);
    for (uint32_t s = 0; s < n; ++s) {
        if (!r.valid(s) || root[s] >= 0) continue;
        std::vector<uint32_t> cells{s};
        root[s] = s;
        for (size_t q = 0; q < cells.size(); ++q) {
            const int64_t y = cells[q] / r.cols, x = cells[q] % r.cols;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((dy == 0 && dx == 0) || (!eight && dy != 0 && dx != 0)) continue;
                    const int64_t yy = y + dy, xx = x + dx;
                    if (yy < 0 || xx < 0 || yy >= int64_t(r.rows) || xx >= int64_t(r.cols)) continue;
                    const uint32_t j = uint32_t(yy * r.cols + xx);
                    if (root[j] >= 0 || !r.joined(cells[q], j)) continue;
                    root[j] = s;
                    cells.push_back(j);
                }
        }
        if (cells.size() < min_cells) continue;
        ++a.k;
        for (uint32_t c : cells) a.label[c] = dense ? uint32_t(a.k) : s + 1;
    }
    return a;
}

struct PlainWords {
    std::vector<uint32_t>& w;
    uint32_t load(uint32_t i) { return w[i]; }
    uint32_t fetch_min(uint32_t i, uint32_t v) {
        const uint32_t old = w[i];
        w[i] = std::min(old, v);
        return old;
    }
    void lower(uint32_t i, uint32_t v) { fetch_min(i, v); }
};
struct StaleWords {  // a load returns any value the word has held; the fetch_min acts on the word
    std::vector<std::vector<uint32_t>>& held;
    uint32_t load(uint32_t i) { return held[i][rng() % held[i].size()]; }
    uint32_t fetch_min(uint32_t i, uint32_t v) {
        const uint32_t old = held[i].back();
        if (v < old) held[i].push_back(v);
        return old;
    }
    void lower(uint32_t i, uint32_t v) { fetch_min(i, v); }
};
struct AtomicWords {
    std::atomic<uint32_t>* w;
    uint32_t load(uint32_t i) { return w[i].load(std::memory_order_relaxed); }
    uint32_t fetch_min(uint32_t i, uint32_t v) {  // C++17 has no fetch_min: the loop is one
        uint32_t old = w[i].load(std::memory_order_relaxed);
        while (v < old && !w[i].compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
        return old;
    }
    void lower(uint32_t i, uint32_t v) { fetch_min(i, v); }
};

// phase 1 as k_regions_tiles runs it: a union-find over the tile's local indices, then the global index of the local root
template <typename W>
static std::vector<uint32_t> tiles_phase(const RegRaster<W>& r, uint32_t tw, uint32_t th, bool eight) {
    std::vector<uint32_t> parent(size_t(r.cols) * r.rows);
    for (uint32_t y0 = 0; y0 < r.rows; y0 += th)
        for (uint32_t x0 = 0; x0 < r.cols; x0 += tw) {
            std::vector<uint32_t> words(tw * th);
            for (uint32_t li = 0; li < tw * th; ++li) words[li] = li;
            PlainWords p{words};
            uint32_t loads = 0;
            for (uint32_t li = 0; li < tw * th; ++li) {
                const uint32_t x = x0 + li % tw, y = y0 + li / tw;
                if (x >= r.cols || y >= r.rows) continue;
                const uint32_t links = reg_tile_links(r, y, x, tw, th, eight);
                if (links & kRegLinkW) CHECK(reg_unite(p, li, li - 1, loads) <= reg_unite_bound(li, li - 1));
                if (links & kRegLinkN) CHECK(reg_unite(p, li, li - tw, loads) <= reg_unite_bound(li, li - tw));
                if (links & kRegLinkNW) CHECK(reg_unite(p, li, li - tw - 1, loads) <= reg_unite_bound(li, li - tw - 1));
                if (links & kRegLinkNE) CHECK(reg_unite(p, li, li - tw + 1, loads) <= reg_unite_bound(li, li - tw + 1));
            }
            for (uint32_t li = 0; li < tw * th; ++li) {
                const uint32_t x = x0 + li % tw, y = y0 + li / tw;
                if (x >= r.cols || y >= r.rows) continue;
                uint32_t steps = 0;
                const uint32_t root = reg_find(p, li, steps);
                CHECK(steps <= reg_find_bound(li));
                parent[y * r.cols + x] = (y0 + root / tw) * r.cols + x0 + root % tw;
                CHECK(parent[y * r.cols + x] <= y * r.cols + x);
            }
        }
    return parent;
}

// the cells the seam kernel gives a lane to: every tile's last row and last column
static std::vector<uint32_t> border_cells(uint32_t cols, uint32_t rows, uint32_t tw, uint32_t th) {
    std::vector<uint32_t> cells;
    for (uint32_t y = 0; y < rows; ++y)
        for (uint32_t x = 0; x < cols; ++x)
            if ((x + 1) % tw == 0 || (y + 1) % th == 0) cells.push_back(y * cols + x);
    return cells;
}

// phases 3 and 4 over the joined parents
template <typename W>
static Answer finish(const RegRaster<W>& r, std::vector<uint32_t> parent, bool dense, uint64_t min_cells) {
    const uint32_t n = r.cols * r.rows, need = min_cells > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(min_cells);
    std::vector<uint32_t> count(n, 0);
    PlainWords p{parent};
    for (uint32_t i = 0; i < n; ++i) {
        if (!r.valid(i)) continue;
        uint32_t steps = 0;
        const uint32_t root = reg_find(p, i, steps);
        CHECK(steps <= reg_find_bound(i));
        parent[i] = root;
        ++count[root];
    }
    Answer a;
    for (uint32_t i = 0; i < n; ++i) {
        if (!r.valid(i) || parent[i] != i) continue;
        const bool kept = reg_kept(count[i], need);
        a.k += kept;
        if (dense) count[i] = kept ? uint32_t(a.k) : 0u;
    }
    a.label.resize(n);
    for (uint32_t i = 0; i < n; ++i) a.label[i] = reg_label(r.valid(i), parent[i], count[parent[i]], dense, need);
    return a;
}

enum Mode { PLAIN, STALE, THREADS };

template <typename W>
static std::vector<uint32_t> seams_phase(const RegRaster<W>& r, std::vector<uint32_t> parent, uint32_t tw, uint32_t th, bool eight, Mode mode,
                                         unsigned threads) {
    std::vector<uint32_t> cells = border_cells(r.cols, r.rows, tw, th);
    for (size_t k = cells.size(); k > 1; --k) std::swap(cells[k - 1], cells[rng() % k]);  // no order is promised
    const auto bound = [&](uint32_t i) { return reg_unite_bound(i, i + r.cols + 1); };
    if (mode == PLAIN) {
        PlainWords p{parent};
        for (uint32_t i : cells) {
            uint32_t loads = 0;
            CHECK(reg_seam_unite(p, r, i / r.cols, i % r.cols, tw, th, eight, loads) <= bound(i));
        }
        return parent;
    }
    if (mode == STALE) {
        std::vector<std::vector<uint32_t>> held(parent.size());
        for (size_t i = 0; i < parent.size(); ++i) held[i] = {uint32_t(i), parent[i]};  // "i" is stale from the start where parent[i] < i
        StaleWords p{held};
        for (uint32_t i : cells) {
            uint32_t loads = 0;
            CHECK(reg_seam_unite(p, r, i / r.cols, i % r.cols, tw, th, eight, loads) <= bound(i));
        }
        for (size_t i = 0; i < parent.size(); ++i) parent[i] = held[i].back();
        return parent;
    }
    std::vector<std::atomic<uint32_t>> words(parent.size());
    for (size_t i = 0; i < parent.size(); ++i) words[i].store(parent[i], std::memory_order_relaxed);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            AtomicWords p{words.data()};
            for (size_t k = t; k < cells.size(); k += threads) {
                const uint32_t i = cells[k];
                uint32_t loads = 0;
                const uint32_t rounds = reg_seam_unite(p, r, i / r.cols, i % r.cols, tw, th, eight, loads);
                CHECK(rounds <= bound(i));
                CHECK(loads <= 5 * uint64_t(rounds) * 2 * reg_find_bound(i + r.cols + 1));  // five joins at most, two finds a round
            }
        });
    for (std::thread& t : pool) t.join();
    for (size_t i = 0; i < parent.size(); ++i) {
        parent[i] = words[i].load(std::memory_order_relaxed);
        CHECK(parent[i] <= i);
    }
    return parent;
}

struct Shape {
    uint32_t tw, th;
    Mode mode;
};

// one raster under several tile shapes: the flood fill's answers are made once
template <typename W>
static void one_raster(const std::vector<W>& src, const std::vector<uint8_t>& mask, bool use_src, bool use_mask, uint32_t cols, uint32_t rows,
                       const std::vector<Shape>& shapes, unsigned threads) {
    const RegRaster<W> r{use_src ? src.data() : nullptr, use_mask ? mask.data() : nullptr, cols, rows};
    const uint64_t sieves[] = {0, 2, 5, uint64_t(cols) * rows + 1, ~uint64_t(0)};
    for (int eight = 0; eight < 2; ++eight) {
        std::vector<Answer> want;
        for (int dense = 0; dense < 2; ++dense)
            for (uint64_t min_cells : sieves) want.push_back(flood(r, eight != 0, dense != 0, min_cells));
        for (const Shape& s : shapes) {
            const std::vector<uint32_t> joined = seams_phase(r, tiles_phase(r, s.tw, s.th, eight != 0), s.tw, s.th, eight != 0, s.mode, threads);
            size_t k = 0;
            for (int dense = 0; dense < 2; ++dense)
                for (uint64_t min_cells : sieves) CHECK(finish(r, joined, dense != 0, min_cells) == want[k++]);
        }
    }
}

static void every_small_mask() {
    const std::vector<Shape> shapes = {{1, 1, PLAIN}, {2, 2, PLAIN}, {3, 2, PLAIN}, {2, 3, PLAIN}, {2, 2, STALE}};
    for (uint32_t rows = 1; rows <= 4; ++rows)
        for (uint32_t cols = 1; cols <= 4; ++cols)
            for (uint32_t bits = 0; bits < (1u << (rows * cols)); ++bits) {
                std::vector<uint8_t> mask(rows * cols), none;
                for (uint32_t i = 0; i < rows * cols; ++i) mask[i] = (bits >> i) & 1u ? uint8_t(1 + i) : uint8_t(0);
                one_raster<uint8_t>(none, mask, false, true, cols, rows, shapes, 1);
            }
}

template <typename W>
static void random_rasters(int count, Mode mode) {
    for (int k = 0; k < count; ++k) {
        const uint32_t cols = 1 + rng() % 40, rows = 1 + rng() % 40, n = cols * rows;
        const uint32_t classes = 1 + rng() % 3, fill = 30 + rng() % 60;
        std::vector<W> src(n);
        std::vector<uint8_t> mask(n);
        for (uint32_t i = 0; i < n; ++i) {
            src[i] = W(W(rng() % classes) << (8 * (sizeof(W) - 1)));  // classes that differ only in the top byte
            mask[i] = rng() % 100 < fill;
        }
        const uint32_t tw = 1 + rng() % 9, th = 1 + rng() % 9;
        const unsigned threads = 1 + unsigned(rng() % 16);
        one_raster<W>(src, mask, true, k % 3 != 0, cols, rows, {{tw, th, mode}}, threads);
        one_raster<W>(src, mask, false, true, cols, rows, {{tw, th, mode}}, threads);
    }
}

// one region whose chains cross every seam: a serpentine, its root in the first tile
static void serpentine(Mode mode) {
    const uint32_t cols = 37, rows = 39;
    std::vector<uint8_t> mask(cols * rows, 0), none;
    for (uint32_t y = 0; y < rows; ++y)
        for (uint32_t x = 0; x < cols; ++x)
            mask[y * cols + x] = y % 2 == 0 || x == ((y / 2) % 2 == 0 ? cols - 1 : 0);
    for (uint32_t t = 1; t <= 8; ++t) one_raster<uint8_t>(none, mask, false, true, cols, rows, {{t, 9 - t, mode}}, 16);
}

static void layout() {
    CHECK(reg_workspace_bytes(0, 5) == 0 && reg_workspace_bytes(5, 0) == 0 && reg_workspace_bytes(kRegMaxSide + 1, 1) == 0);
    CHECK(reg_workspace_bytes(1, uint64_t(1) << 63) == 0);
    const RegWorkspace w = reg_workspace(3, 5);
    CHECK(w.off_count == 64 && w.off_sums == 128 && w.bytes == 144);
    const RegWorkspace big = reg_workspace(kRegMaxSide, kRegMaxSide);
    CHECK(big.off_count == (size_t(1) << 32) && big.bytes == (size_t(1) << 33) + (size_t(1) << 30) / kRegScanCells * 4);
    CHECK(reg_tiles(1, kRegTileW) == 1 && reg_tiles(kRegTileW + 1, kRegTileW) == 2 && reg_scan_blocks(kRegScanCells + 1) == 2);
}

// ec_regions' refusals.  Addresses are plain integers, never dereferenced.
static const void* at(uint64_t a) { return reinterpret_cast<const void*>(uintptr_t(a)); }
static bool says(const ecv::Refusal& r, const char* text, bool bad_type = false) {
    return r.why && std::string_view(r.why) == text && r.bad_type == bad_type;
}

static void refusals() {
    // 10 x 10 cells of 2 bytes: src 200 bytes at S, src_mask 100 at V, dst 400 at D, dst_mask 100 at E, n_regions 8 at C, the workspace W at K
    const uint64_t S = 0x10000, V = 0x11000, D = 0x20000, E = D + 400, C = 0x30000, K = 0x40000, FAR = uint64_t(1) << 40, W = reg_workspace_bytes(10, 10);
    const void* far = at(FAR);
    auto call = [](const void* src, const void* mask, const void* dst, const void* dm, const void* count, const void* ws) {
        return regions_refusal(2, src, mask, 10, 10, 8, true, dst, dm, count, ws);
    };
    CHECK(W == 816);
    CHECK(!call(at(S), at(V), at(D), at(E), at(C), at(K)) && !call(at(S), nullptr, at(D), nullptr, nullptr, nullptr));
    CHECK(!call(at(S), at(V), nullptr, at(E), nullptr, nullptr) && !call(at(S), at(V), nullptr, nullptr, at(C), nullptr));
    CHECK(!regions_refusal(0, nullptr, at(V), 10, 10, 4, true, at(D), at(E), at(C), at(K)));  // the mask form: no src, no cell type
    // the order: each call is wrong in everything that comes later as well
    const char* const side = "cols and rows must be within 1 .. EC_REGIONS_MAX_SIDE";
    CHECK(says(regions_refusal(0, at(S + 1), nullptr, 0, 10, 5, false, nullptr, nullptr, nullptr, at(K + 1)), side));
    CHECK(says(regions_refusal(0, at(S + 1), nullptr, 10, 0, 5, false, nullptr, nullptr, nullptr, at(K + 1)), side));
    CHECK(says(regions_refusal(0, at(S + 1), nullptr, 10, 10, 5, false, nullptr, nullptr, nullptr, at(K + 1)), "bad cell type", true));
    CHECK(says(regions_refusal(0, nullptr, nullptr, 10, 10, 5, false, nullptr, nullptr, nullptr, at(K + 1)), "connectivity is neither 4 nor 8"));
    CHECK(says(regions_refusal(0, nullptr, nullptr, 10, 10, 6, false, nullptr, nullptr, nullptr, at(K + 1)), "connectivity is neither 4 nor 8"));
    CHECK(says(regions_refusal(0, nullptr, nullptr, 10, 10, 4, false, nullptr, nullptr, nullptr, at(K + 1)), "numbering is neither EC_REGIONS_ROOT nor EC_REGIONS_DENSE"));
    CHECK(says(regions_refusal(0, nullptr, nullptr, 10, 10, 8, false, nullptr, nullptr, nullptr, at(K + 1)), "numbering is neither EC_REGIONS_ROOT nor EC_REGIONS_DENSE"));
    CHECK(says(call(nullptr, nullptr, nullptr, nullptr, nullptr, at(K + 1)), "src and src_mask are both NULL"));
    CHECK(says(call(at(S + 1), nullptr, nullptr, nullptr, nullptr, at(K + 1)), "dst, dst_mask and n_regions are all NULL"));
    CHECK(says(call(at(S + 1), nullptr, at(S + 2), at(S), at(S + 4), at(S + 8)), "src is not aligned to its cell type"));
    CHECK(says(call(at(S), nullptr, at(S + 2), at(S), at(S + 4), at(S + 8)), "dst is not aligned to its cell type"));
    CHECK(says(call(at(S), nullptr, at(S), at(S), at(S + 4), at(S + 8)), "n_regions is not aligned to 8 bytes"));
    CHECK(says(call(at(S), nullptr, at(S), at(S), at(S), at(S + 8)), "the workspace is not aligned to 16 bytes"));
    CHECK(says(call(at(S), at(S), at(S), at(S), at(S), at(S)), "dst overlaps src"));
    CHECK(says(call(far, at(V), at(V), at(V), at(V), at(V)), "dst overlaps src_mask"));
    CHECK(says(call(at(S), at(S), at(D), at(S), at(S), at(S)), "dst_mask overlaps src"));
    CHECK(says(call(far, at(V), at(D), at(V), at(V), at(V)), "dst_mask overlaps src_mask"));
    CHECK(says(call(at(S), at(S), at(D), at(D), at(S), at(S)), "n_regions overlaps src"));
    CHECK(says(call(far, at(V), at(D), at(D), at(V), at(V)), "n_regions overlaps src_mask"));
    CHECK(says(call(at(S), at(S), at(D), at(D), at(D), at(S)), "the workspace overlaps src"));
    CHECK(says(call(far, at(V), at(D), at(D), at(D), at(V)), "the workspace overlaps src_mask"));
    CHECK(says(call(at(S), at(V), at(D), at(D), at(D), at(D)), "dst_mask overlaps dst"));
    CHECK(says(call(at(S), at(V), at(D), at(E), at(D), at(D)), "n_regions overlaps dst"));
    CHECK(says(call(at(S), at(V), at(D), at(E), at(E), at(E - 16)), "n_regions overlaps dst_mask"));  // the workspace on dst, dst_mask and n_regions
    CHECK(says(call(at(S), at(V), at(D), at(E), at(C), at(E - 16)), "the workspace overlaps dst"));
    CHECK(says(call(at(S), at(V), at(D), at(C), at(C), at(C)), "n_regions overlaps dst_mask"));
    CHECK(says(call(at(S), at(V), at(D), at(C + 8), at(C), at(C)), "the workspace overlaps dst_mask"));
    CHECK(says(call(at(S), at(V), at(D), at(E), at(C), at(C)), "the workspace overlaps n_regions"));
    // each overlap by the least an aligned pointer allows, and the same two blocks touching
    CHECK(says(call(at(S), at(V), at(S + 196), nullptr, nullptr, nullptr), "dst overlaps src") && !call(at(S), at(V), at(S + 200), nullptr, nullptr, nullptr));
    CHECK(says(call(at(S), at(V), at(V + 96), nullptr, nullptr, nullptr), "dst overlaps src_mask") && !call(at(S), at(V), at(V + 100), nullptr, nullptr, nullptr));
    CHECK(!call(at(S), nullptr, at(V + 96), nullptr, nullptr, nullptr));  // ... which is no input without a mask
    CHECK(says(call(at(S), at(V), nullptr, at(S + 199), nullptr, nullptr), "dst_mask overlaps src") && !call(at(S), at(V), nullptr, at(S + 200), nullptr, nullptr));
    CHECK(says(call(at(S), at(V), nullptr, at(V + 99), nullptr, nullptr), "dst_mask overlaps src_mask") && !call(at(S), at(V), nullptr, at(V + 100), nullptr, nullptr));
    CHECK(says(call(at(S), at(V), nullptr, nullptr, at(S + 192), nullptr), "n_regions overlaps src") && !call(at(S), at(V), nullptr, nullptr, at(S + 200), nullptr));
    CHECK(says(call(at(S), at(V), nullptr, nullptr, at(V), nullptr), "n_regions overlaps src_mask") && !call(at(S), at(V), nullptr, nullptr, at(V - 8), nullptr));
    CHECK(says(call(at(S), at(V), at(D), nullptr, nullptr, at(S - W + 16)), "the workspace overlaps src") && !call(at(S), at(V), at(D), nullptr, nullptr, at(S - W)));
    CHECK(says(call(at(S), at(V), at(D), nullptr, nullptr, at(V - W + 16)), "the workspace overlaps src_mask") && !call(at(S), at(V), at(D), nullptr, nullptr, at(V - W)));
    CHECK(says(call(at(S), at(V), at(D), at(D + 399), nullptr, nullptr), "dst_mask overlaps dst") && !call(at(S), at(V), at(D), at(D + 400), nullptr, nullptr));
    CHECK(says(call(at(S), at(V), at(D), nullptr, at(D + 392), nullptr), "n_regions overlaps dst") && !call(at(S), at(V), at(D), nullptr, at(D + 400), nullptr));
    CHECK(says(call(at(S), at(V), nullptr, at(E), at(E + 96), nullptr), "n_regions overlaps dst_mask") && !call(at(S), at(V), nullptr, at(E), at(E + 104), nullptr) &&
          !call(at(S), at(V), nullptr, at(E), at(E - 8), nullptr));
    CHECK(says(call(at(S), at(V), at(D), nullptr, nullptr, at(D - W + 16)), "the workspace overlaps dst") && !call(at(S), at(V), at(D), nullptr, nullptr, at(D - W)));
    CHECK(says(call(at(S), at(V), nullptr, at(E), nullptr, at(E - W + 16)), "the workspace overlaps dst_mask") && !call(at(S), at(V), nullptr, at(E), nullptr, at(E - W)));
    CHECK(says(call(at(S), at(V), nullptr, nullptr, at(C), at(C - W + 16)), "the workspace overlaps n_regions") && !call(at(S), at(V), nullptr, nullptr, at(C), at(C - W)) &&
          !call(at(S), at(V), nullptr, nullptr, at(C), at(C + 16)));
    // the largest shape, and one past it: 2^30 cells of 8 bytes, every product in 64 bits
    const uint64_t M = kRegMaxSide, N = M * M, WS = reg_workspace_bytes(M, M);
    auto big = [&](uint64_t cols, uint64_t rows, const void* dst, const void* dm, const void* ws) {
        return regions_refusal(8, far, at(FAR + 8 * N), cols, rows, 4, true, dst, dm, nullptr, ws);
    };
    CHECK(WS > 8 * N);
    CHECK(!big(M, M, at(FAR + 9 * N), at(FAR + 13 * N), at(FAR + 14 * N)) && !big(M, M, at(FAR + 9 * N), at(FAR + 13 * N), at(FAR - WS)));
    CHECK(says(big(M, M, at(FAR + 8 * N - 4), nullptr, nullptr), "dst overlaps src") && says(big(M, M, at(FAR + 9 * N - 4), nullptr, nullptr), "dst overlaps src_mask"));
    CHECK(says(big(M, M, at(FAR + 9 * N), at(FAR + 13 * N - 1), nullptr), "dst_mask overlaps dst"));
    CHECK(says(big(M, M, at(FAR + 9 * N), at(FAR + 13 * N), at(FAR - WS + 16)), "the workspace overlaps src"));
    CHECK(says(big(M, M, at(FAR + 9 * N), at(FAR + 13 * N), at(FAR + 14 * N - 16)), "the workspace overlaps dst_mask"));
    CHECK(says(big(M + 1, M, far, far, far), side) && says(big(M, M + 1, far, far, far), side) && says(big(1, uint64_t(1) << 63, far, far, far), side));
}

int main(int argc, char** argv) {
    const bool threads_only = argc > 1 && std::string_view(argv[1]) == "threads";
    if (!threads_only) {
        layout();
        refusals();
        every_small_mask();
        random_rasters<uint8_t>(60, PLAIN);
        random_rasters<uint16_t>(30, PLAIN);
        random_rasters<uint32_t>(30, PLAIN);
        random_rasters<uint64_t>(30, PLAIN);
        random_rasters<uint8_t>(60, STALE);
        serpentine(PLAIN);
        serpentine(STALE);
    }
    random_rasters<uint8_t>(threads_only ? 40 : 120, THREADS);
    random_rasters<uint64_t>(threads_only ? 10 : 30, THREADS);
    serpentine(THREADS);
    std::printf("%ld checks passed, %ld failed\n", checks.load() - failures.load(), failures.load());
    return failures.load() == 0 ? 0 : 1;
}
