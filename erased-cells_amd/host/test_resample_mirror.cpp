// test_resample_mirror.cpp — CellBuffer::window / MaskedCellBuffer::window with a ResampleAlg of the C++ host mirror (needs an MI355X):
// they agree with ec_window_resample called directly, the default and NearestNeighbour stay ec_window, and u16 cells match the rule of
// include/erased_cells.h worked out here in integers (for cells this small the f64 steps of the rule are exact until the division, so
// the answer is the exact weighted mean rounded half away from zero).
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "erased_cells.hpp"

using namespace erased_cells;

static int g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)
#define CHECK_THROWS(T, expr)                                                          \
    do {                                                                               \
        ++g_checks;                                                                    \
        bool threw_ = false;                                                           \
        try { (void)(expr); } catch (const T&) { threw_ = true; }                      \
        if (!threw_) {                                                                 \
            std::fprintf(stderr, "%s:%d: expected %s from %s\n", __FILE__, __LINE__, #T, #expr); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct Tap {
    size_t c;
    uint64_t w;
};
static std::vector<Tap> taps(ResampleAlg alg, size_t j, size_t win, size_t out) {
    std::vector<Tap> t;
    if (alg == ResampleAlg::Average) {
        const size_t g = std::gcd(win, out);
        win /= g;
        out /= g;
        const size_t lo = j * win, hi = lo + win;
        for (size_t c = lo / out; c <= (hi - 1) / out; ++c) t.push_back({c, std::min((c + 1) * out, hi) - std::max(c * out, lo)});
    } else {
        const size_t v = (2 * j + 1) * win + out, k = v / (2 * out), f = v % (2 * out);
        t.push_back({k == 0 ? 0 : std::min(k - 1, win - 1), 2 * out - f});
        if (f) t.push_back({std::min(k, win - 1), f});
    }
    return t;
}

// (value, valid) of every output cell; m empty: no mask
static void expect(ResampleAlg alg, const std::vector<uint16_t>& a, const std::vector<bool>& m, size_t cols, size_t x0, size_t y0, size_t w,
                   size_t h, size_t ow, size_t oh, std::vector<uint16_t>* v, std::vector<bool>* ok) {
    v->assign(ow * oh, 0);
    ok->assign(ow * oh, false);
    for (size_t i = 0; i < oh; ++i)
        for (size_t j = 0; j < ow; ++j) {
            uint64_t num = 0, den = 0;
            for (const Tap& y : taps(alg, i, h, oh))
                for (const Tap& x : taps(alg, j, w, ow)) {
                    const size_t at = (y0 + y.c) * cols + x0 + x.c;
                    if (m.empty() || m[at]) {
                        num += y.w * x.w * a[at];
                        den += y.w * x.w;
                    }
                }
            if (den) {
                (*v)[i * ow + j] = static_cast<uint16_t>((2 * num + den) / (2 * den));
                (*ok)[i * ow + j] = true;
            }
        }
}

int main() {
    try {
        init(0);
        const size_t cols = 97, rows = 23;
        std::vector<uint16_t> a(cols * rows);
        std::vector<bool> m(cols * rows);
        for (size_t i = 0; i < a.size(); ++i) {
            a[i] = static_cast<uint16_t>(mix(7 ^ i));
            m[i] = mix(~7ull ^ i) % 100 < 60;
        }
        const CellBuffer buf = CellBuffer::from_vec(a);
        const MaskedCellBuffer mb(CellBuffer::from_vec(a), Mask::new_(m));
        const size_t geoms[][6] = {{3, 1, 40, 8, 20, 4}, {0, 0, 97, 23, 31, 7}, {5, 2, 35, 7, 14, 3}, {64, 15, 33, 8, 47, 21},
                                   {2, 2, 64, 2, 1, 2}, {96, 22, 1, 1, 3, 2}, {1, 0, 33, 7, 11, 7}};
        for (const ResampleAlg alg : {ResampleAlg::Bilinear, ResampleAlg::Average})
            for (const auto& g : geoms) {
                const std::pair<size_t, size_t> at{g[0], g[1]}, win{g[2], g[3]}, out{g[4], g[5]};
                std::vector<uint16_t> v;
                std::vector<bool> ok;
                expect(alg, a, {}, cols, g[0], g[1], g[2], g[3], g[4], g[5], &v, &ok);
                const CellBuffer got = buf.window(cols, at, win, out, alg);
                CHECK(got.cell_type() == CellType::UInt16 && got.to_vec<uint16_t>() == v);
                // the C ABI, called directly into a buffer of the mirror
                CellBuffer raw = CellBuffer::with_defaults(out.first * out.second, CellType::UInt16);
                check(ec_window_resample(static_cast<int32_t>(alg), EC_U16, buf.ptr(), nullptr, cols, rows, g[0], g[1], g[2], g[3], g[4], g[5], raw.ptr(),
                                         nullptr, current_stream()));
                CHECK(raw.to_vec<uint16_t>() == v);
                expect(alg, a, m, cols, g[0], g[1], g[2], g[3], g[4], g[5], &v, &ok);
                const MaskedCellBuffer mgot = mb.window(cols, at, win, out, alg);
                CHECK(mgot.to_vec<uint16_t>() == v && mgot.mask().to_vec() == ok);
            }
        // the default and NearestNeighbour are window() as it was
        const std::pair<size_t, size_t> at{3, 1}, win{40, 8}, out{20, 4};
        const auto base = buf.window(cols, at, win, out).to_vec<uint16_t>();
        CHECK(buf.window(cols, at, win, out, std::nullopt).to_vec<uint16_t>() == base);
        CHECK(buf.window(cols, at, win, out, ResampleAlg::NearestNeighbour).to_vec<uint16_t>() == base);
        CHECK(mb.window(cols, at, win, out, ResampleAlg::NearestNeighbour).to_vec<uint16_t>() == base);
        CHECK(buf.window(cols, at, win, win, ResampleAlg::Average).to_vec<uint16_t>() == buf.window(cols, at, win).to_vec<uint16_t>());
        // algorithms the library lacks, and an average beyond the cap, are refused by the library
        CHECK_THROWS(Error, buf.window(cols, at, win, out, ResampleAlg::Cubic));
        CHECK_THROWS(Error, mb.window(cols, at, win, out, ResampleAlg::Gauss));
        CHECK_THROWS(Error, buf.window(cols, {0, 0}, {65, 1}, std::pair<size_t, size_t>{1, 1}, ResampleAlg::Average));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    std::printf("resample mirror: %d checks passed\n", g_checks);
    return 0;
}
