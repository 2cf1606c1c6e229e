// test_window_mirror.cpp — CellBuffer::window / put_window, their masked forms and RasterBand::read_cells(window, window_size, size,
// e_resample_alg) of the C++ host mirror (needs an MI355X).  Expected cells are computed here on the host, by index, with the integer
// resampling rule of include/erased_cells.h; with TEST_DATA_DIR set, also on the reference's Landsat fixtures.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "erased_cells.hpp"
#include "raster_io.hpp"

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
static size_t src_index(size_t j, size_t w, size_t out) { return ((2 * j + 1) * w) / (2 * out); }

template <typename T>
static std::vector<T> cut(const std::vector<T>& a, size_t cols, size_t x0, size_t y0, size_t w, size_t h, size_t ow, size_t oh) {
    std::vector<T> out(ow * oh);
    for (size_t i = 0; i < oh; ++i)
        for (size_t j = 0; j < ow; ++j) out[i * ow + j] = a[(y0 + src_index(i, h, oh)) * cols + x0 + src_index(j, w, ow)];
    return out;
}

template <typename T>
static void window_tests(uint64_t seed) {
    const size_t cols = 197, rows = 59;
    std::vector<T> a(cols * rows);
    std::vector<bool> m(cols * rows);
    for (size_t i = 0; i < a.size(); ++i) {
        a[i] = static_cast<T>(mix(seed ^ i));
        m[i] = mix(~seed ^ i) & 1;
    }
    const CellBuffer buf = CellBuffer::from_vec(a);
    const size_t geoms[][6] = {{3, 2, 170, 50, 170, 50}, {0, 0, cols, rows, cols, rows}, {196, 58, 1, 1, 1, 1}, {5, 1, 33, 57, 33, 57},
                               {4, 4, 180, 48, 90, 24}, {1, 3, 147, 49, 63, 21}, {7, 0, 40, 20, 100, 50}, {0, 9, 197, 30, 50, 1}};
    for (const auto& g : geoms) {
        const size_t x0 = g[0], y0 = g[1], w = g[2], h = g[3], ow = g[4], oh = g[5];
        CHECK(buf.window(cols, {x0, y0}, {w, h}, {{ow, oh}}).template to_vec<T>() == cut(a, cols, x0, y0, w, h, ow, oh));
    }
    CHECK(buf.window(cols, {9, 9}, {20, 5}).template to_vec<T>() == cut(a, cols, 9, 9, 20, 5, 20, 5));  // size defaults to window_size
    CHECK(buf.window(cols, {cols, rows}, {0, 0}).len() == 0);
    CHECK_THROWS(Error, buf.window(cols, {190, 0}, {8, 1}));
    CHECK_THROWS(Error, buf.window(cols, {0, 0}, {8, 1}, {{0, 1}}));

    // paste: the whole destination equals the host's slice assignment
    CellBuffer dst = CellBuffer::from_vec(a);
    std::vector<T> exp = a, tile(45 * 13);
    for (size_t i = 0; i < tile.size(); ++i) tile[i] = static_cast<T>(mix(seed + 77 + i));
    dst.put_window(cols, {151, 44}, {45, 13}, CellBuffer::from_vec(tile));
    for (size_t r = 0; r < 13; ++r)
        for (size_t c = 0; c < 45; ++c) exp[(44 + r) * cols + 151 + c] = tile[r * 45 + c];
    CHECK(dst.template to_vec<T>() == exp);
    CHECK(dst.window(cols, {151, 44}, {45, 13}).template to_vec<T>() == tile);
    dst.put_window(cols, {151, 44}, {45, 13}, buf.window(cols, {151, 44}, {45, 13}));  // cut from the original, paste back
    CHECK(dst.template to_vec<T>() == a);
    CHECK_THROWS(std::logic_error, dst.put_window(cols, {0, 0}, {45, 12}, CellBuffer::from_vec(tile)));

    // values and mask in one launch
    MaskedCellBuffer mb(CellBuffer::from_vec(a), Mask::new_(m));
    const MaskedCellBuffer part = mb.window(cols, {11, 5}, {150, 40}, {{60, 80}});
    const std::vector<bool> em = cut(m, cols, 11, 5, 150, 40, 60, 80);
    size_t n_true = 0;
    for (bool b : em) n_true += b;
    CHECK(part.buffer().template to_vec<T>() == cut(a, cols, 11, 5, 150, 40, 60, 80));
    CHECK(part.mask().to_vec() == em);
    CHECK(part.counts() == std::make_pair(n_true, em.size() - n_true));
    mb.put_window(cols, {2, 1}, {60, 80 / 2}, part.window(60, {0, 0}, {60, 40}));
    std::vector<T> ea = a;
    std::vector<bool> emask = m;
    const std::vector<T> pa = cut(a, cols, 11, 5, 150, 40, 60, 80);
    for (size_t r = 0; r < 40; ++r)
        for (size_t c = 0; c < 60; ++c) {
            ea[(1 + r) * cols + 2 + c] = pa[r * 60 + c];
            emask[(1 + r) * cols + 2 + c] = em[r * 60 + c];
        }
    CHECK(mb.buffer().template to_vec<T>() == ea);
    CHECK(mb.mask().to_vec() == emask);
}

static void fixture_tests(const std::string& dir) {
    const RasterBand b5 = RasterBand::open(dir + "/L8-Elkton-VA-B5.tiff");
    const auto size = b5.size();
    const std::vector<uint16_t> cells = b5.read_cells().to_vec<uint16_t>();
    CHECK(b5.read_cells({0, 0}, size, size, std::nullopt).to_vec<uint16_t>() == cells);  // src/gdal/rasterband.rs:27-33
    CHECK(b5.read_cells({0, 0}, size, size, ResampleAlg::NearestNeighbour).to_vec<uint16_t>() == cells);
    CHECK(b5.read_cells({37, 21}, {101, 64}, {101, 64}).to_vec<uint16_t>() == cut(cells, size.first, 37, 21, 101, 64, 101, 64));
    const std::pair<size_t, size_t> half{size.first / 2, size.second / 2};
    CHECK(b5.read_cells({0, 0}, size, half).to_vec<uint16_t>() == cut(cells, size.first, 0, 0, size.first, size.second, half.first, half.second));
    CHECK_THROWS(Error, b5.read_cells({0, 0}, size, half, ResampleAlg::Bilinear));
    CHECK_THROWS(Error, b5.read_cells({-1, 0}, {4, 4}, {4, 4}));
    CHECK_THROWS(Error, b5.read_cells({0, 0}, {size.first + 1, 4}, {4, 4}));

    const RasterBand nd = RasterBand::open(dir + "/L8-Elkton-VA-B5-nd.tiff");
    const std::vector<uint16_t> ndc = nd.read_cells().to_vec<uint16_t>();
    size_t x_lo = size.first, x_hi = 0, y_lo = size.second, y_hi = 0, found = 0;
    for (size_t i = 0; i < ndc.size(); ++i)
        if (ndc[i] == 0) {  // the band's nodata value
            ++found;
            x_lo = std::min(x_lo, i % size.first), x_hi = std::max(x_hi, i % size.first);
            y_lo = std::min(y_lo, i / size.first), y_hi = std::max(y_hi, i / size.first);
        }
    CHECK(found == 4 && nd.no_data_value() == 0.0);
    const size_t w = x_hi + 1 - x_lo, h = y_hi + 1 - y_lo;
    const MaskedCellBuffer win = nd.read_cells_masked({static_cast<long long>(x_lo), static_cast<long long>(y_lo)}, {w, h}, {w, h});
    CHECK(win.counts() == std::make_pair(w * h - 4, size_t(4)));
    CHECK(win.buffer().to_vec<uint16_t>() == cut(ndc, size.first, x_lo, y_lo, w, h, w, h));
    CHECK(nd.read_cells_masked({0, 0}, size, size).counts() == nd.read_cells_masked().counts());
}

int main() {
    const char* dd = std::getenv("TEST_DATA_DIR");
    try {
        init(0);
        window_tests<uint8_t>(1);
        window_tests<uint16_t>(2);
        window_tests<int32_t>(3);
        window_tests<uint64_t>(4);
        if (dd) fixture_tests(dd);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    std::printf("window mirror: %d checks passed%s\n", g_checks, dd ? " (incl. GDAL fixture tests)" : "");
    return 0;
}
