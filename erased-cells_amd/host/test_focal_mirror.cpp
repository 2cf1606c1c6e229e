// test_focal_mirror.cpp — CellBuffer::focal / convolve (and their _whole forms), MaskedCellBuffer::focal / convolve and Mask::dilate /
// erode of the C++ host mirror (needs an MI355X) on cells whose answer can be worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstdlib>

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

using Bits = std::vector<bool>;

int main() {
    try {
        init(0);
        {  // a 4 x 3 raster of u8 cells, 3 x 3 footprints clipped at the edges
            const CellBuffer a = CellBuffer::from_vec<uint8_t>({1, 2, 3, 4,  //
                                                                5, 6, 7, 8,  //
                                                                9, 10, 11, 12});
            const CellBuffer sum = a.focal(4, EC_FOCAL_SUM);
            CHECK(sum.cell_type() == CellType::Float64);
            CHECK(sum.to_vec<double>() == std::vector<double>({14, 24, 30, 22, 33, 54, 63, 45, 30, 48, 54, 38}));
            CHECK(a.focal(4, EC_FOCAL_MEAN).to_vec<double>() ==
                  std::vector<double>({3.5, 4.0, 5.0, 5.5, 5.5, 6.0, 7.0, 7.5, 7.5, 8.0, 9.0, 9.5}));
            const CellBuffer mx = a.focal(4, EC_FOCAL_MAX, {1, 0});
            CHECK(mx.cell_type() == CellType::UInt8 && mx.to_vec<uint8_t>() == std::vector<uint8_t>({2, 3, 4, 4, 6, 7, 8, 8, 10, 11, 12, 12}));
            CHECK(a.focal(4, EC_FOCAL_MIN, {0, 1}).to_vec<uint8_t>() == std::vector<uint8_t>({1, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8}));
            CHECK(a.focal(4, EC_FOCAL_SUM, {0, 0}).to_vec<double>() == a.convert(CellType::Float64).to_vec<double>());
            const MaskedCellBuffer whole = a.focal_whole(4, EC_FOCAL_SUM);   // only the two interior cells have their whole footprint
            CHECK(whole.mask().to_vec() == Bits({0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0}));
            CHECK(whole.buffer().to_vec<double>() == std::vector<double>({0, 0, 0, 0, 0, 54, 63, 0, 0, 0, 0, 0}));
            // a horizontal gradient: weight [dy][dx] meets cell (i - ry + dy, j - rx + dx)
            const std::vector<double> grad = {-1.0, 0.0, 1.0};
            CHECK(a.convolve(4, grad, {1, 0}).to_vec<double>() == std::vector<double>({2, 2, 2, -3, 6, 2, 2, -7, 10, 2, 2, -11}));
            const MaskedCellBuffer g = a.convolve_whole(4, grad, {1, 0});
            CHECK(g.mask().to_vec() == Bits({0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0}));
            const std::vector<double> box = {0.5, 0.5, 0.5};
            CHECK(a.convolve(4, box, {1, 0}, true).to_vec<double>() == std::vector<double>({1.5, 2, 3, 3.5, 5.5, 6, 7, 7.5, 9.5, 10, 11, 11.5}));
        }
        {  // masked: a hole is filled from its neighbours, a NaN under a cleared mask byte leaves no trace
            const CellBuffer f = CellBuffer::from_vec<double>({1.0, NAN, 3.0, 4.0, 5.0, 6.0});
            const MaskedCellBuffer m(f.clone(), Mask::new_({true, false, true, true, false, false}));
            const MaskedCellBuffer s = m.focal(3, EC_FOCAL_SUM);
            CHECK(s.mask().to_vec() == Bits({1, 1, 1, 1, 1, 1}));
            CHECK(s.buffer().to_vec<double>() == std::vector<double>({5, 8, 3, 5, 8, 3}));
            const MaskedCellBuffer mean = m.focal(3, EC_FOCAL_MEAN, {0, 0});
            CHECK(mean.mask().to_vec() == Bits({1, 0, 1, 1, 0, 0}) && mean.buffer().to_vec<double>() == std::vector<double>({1, 0, 3, 4, 0, 0}));
            const MaskedCellBuffer w = m.focal(3, EC_FOCAL_MAX, {1, 0}, true);
            CHECK(w.mask().to_vec() == Bits({0, 0, 0, 0, 0, 0}));
            CHECK(m.focal(3, EC_FOCAL_MIN, {1, 1}).buffer().to_vec<double>() == std::vector<double>({1, 1, 3, 1, 1, 3}));
            const MaskedCellBuffer c = m.convolve(3, {1.0, 2.0, 1.0}, {1, 0}, true);
            CHECK(c.buffer().to_vec<double>() == std::vector<double>({1.0, 2.0, 3.0, 4.0, 4.0, 0.0}));
            CHECK(c.mask().to_vec() == Bits({1, 1, 1, 1, 1, 0}));
        }
        {  // -0.0 sorts before +0.0 and a positive NaN last: the total order of ec_min_max
            const CellBuffer z = CellBuffer::from_vec<double>({0.0, -0.0, NAN});
            const std::vector<double> mn = z.focal(3, EC_FOCAL_MIN).to_vec<double>(), mx = z.focal(3, EC_FOCAL_MAX).to_vec<double>();
            CHECK(std::signbit(mn[0]) && std::signbit(mn[1]) && std::signbit(mn[2]) && mn[2] == 0.0);
            CHECK(!std::signbit(mx[0]) && mx[0] == 0.0 && std::isnan(mx[1]) && std::isnan(mx[2]));
        }
        {  // dilate and erode on a 5 x 3 mask; closing keeps every set cell
            const Mask m = Mask::new_({0, 0, 0, 0, 0,  //
                                       0, 1, 0, 0, 1,  //
                                       0, 0, 0, 0, 1});
            CHECK(m.dilate(5).to_vec() == Bits({1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}));
            CHECK(m.dilate(5, {1, 0}).to_vec() == Bits({0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1}));
            CHECK(m.erode(5, {0, 1}).to_vec() == Bits({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}));  // column 4: rows 1 and 2 are set, row 0 is not
            CHECK(m.dilate(5, {0, 0}).to_vec() == m.to_vec());
            const std::vector<bool> closed = m.dilate(5, {1, 1}).erode(5, {1, 1}).to_vec(), was = m.to_vec();
            for (size_t i = 0; i < was.size(); ++i) CHECK(!was[i] || closed[i]);
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer a = CellBuffer::from_vec<uint8_t>({1, 2, 3, 4});
            bool threw = false;
            try { a.focal(2, static_cast<ec_focal_op>(4)); } catch (const Error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { a.focal(2, EC_FOCAL_SUM, {8, 0}); } catch (const Error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { a.focal(3, EC_FOCAL_SUM); } catch (const std::logic_error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { a.convolve(2, {1.0, 1.0}, {1, 0}); } catch (const std::logic_error&) { threw = true; }
            CHECK(threw);
            CHECK(CellBuffer::from_vec<uint8_t>({}).focal(0, EC_FOCAL_MAX).len() == 0);
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
