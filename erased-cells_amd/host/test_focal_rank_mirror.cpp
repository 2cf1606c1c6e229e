// test_focal_rank_mirror.cpp — CellBuffer::focal_rank / focal_median / focal_majority (and their _whole forms) and the MaskedCellBuffer
// forms of the C++ host mirror (needs an MI355X) on cells whose answer can be worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
using U8 = std::vector<uint8_t>;

int main() {
    try {
        init(0);
        {  // a 4 x 3 raster of u8 cells with one outlier, 3 x 3 footprints clipped at the edges
            const CellBuffer a = CellBuffer::from_vec<uint8_t>({5, 1, 9, 3,  //
                                                                7, 2, 8, 4,  //
                                                                6, 0, 200, 3});
            const CellBuffer lo = a.focal_median(4), hi = a.focal_median(4, {1, 1}, EC_RANK_UPPER);
            CHECK(lo.cell_type() == CellType::UInt8 && lo.len() == 12);
            // (0, 0): 5 1 7 2 -> 1 2 5 7: lower 2, upper 5.  (1, 1): 0 1 2 5 6 7 8 9 200 -> 6 both ways: the outlier is gone.
            // (1, 2): 0 1 2 3 3 4 8 9 200 -> 3.  (2, 3): 8 4 200 3 -> 3 4 8 200: lower 4, upper 8
            CHECK(lo.to_vec<uint8_t>()[0] == 2 && hi.to_vec<uint8_t>()[0] == 5);
            CHECK(lo.to_vec<uint8_t>()[5] == 6 && hi.to_vec<uint8_t>()[5] == 6 && lo.to_vec<uint8_t>()[6] == 3 && hi.to_vec<uint8_t>()[6] == 3);
            CHECK(lo.to_vec<uint8_t>()[11] == 4 && hi.to_vec<uint8_t>()[11] == 8);
            // the two ends are focal MIN and MAX, whatever the method
            CHECK(a.focal_rank(4, {0, 1}, EC_RANK_UPPER, {2, 1}).to_vec<uint8_t>() == a.focal(4, EC_FOCAL_MIN, {2, 1}).to_vec<uint8_t>());
            CHECK(a.focal_rank(4, {7, 7}, EC_RANK_LOWER, {1, 0}).to_vec<uint8_t>() == a.focal(4, EC_FOCAL_MAX, {1, 0}).to_vec<uint8_t>());
            // 9/10 at the corner: 2.7 -> lower position 2 (5), upper 3 (7)
            CHECK(a.focal_rank(4, {9, 10}).to_vec<uint8_t>()[0] == 5 && a.focal_rank(4, {9, 10}, EC_RANK_UPPER).to_vec<uint8_t>()[0] == 7);
            CHECK(a.focal_median(4, {0, 0}).to_vec<uint8_t>() == a.to_vec<uint8_t>());
            const MaskedCellBuffer whole = a.focal_median_whole(4);   // only the two interior cells have their whole footprint
            CHECK(whole.mask().to_vec() == Bits({0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0}));
            CHECK(whole.buffer().to_vec<uint8_t>() == U8({0, 0, 0, 0, 0, 6, 3, 0, 0, 0, 0, 0}));
            CHECK(a.focal_rank_whole(4, {1, 1}, EC_RANK_LOWER, {1, 0}).buffer().to_vec<uint8_t>() == U8({0, 9, 9, 0, 0, 8, 8, 0, 0, 200, 200, 0}));
            // masked: with (0, 0) and (1, 1) masked out the corner's taps are 1 7 — r follows the clipped count, 2
            const MaskedCellBuffer m(a.clone(), Mask::new_({0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1}));
            CHECK(m.focal_median(4).buffer().to_vec<uint8_t>()[0] == 1 && m.focal_median(4, {1, 1}, EC_RANK_UPPER).buffer().to_vec<uint8_t>()[0] == 7);
            CHECK(m.focal_median(4).mask().to_vec() == Bits({1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}));
            CHECK(m.focal_rank(4, {1, 2}, EC_RANK_LOWER, {0, 0}).mask().to_vec() == Bits({0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1}));
            CHECK(m.focal_median(4, {1, 1}, EC_RANK_LOWER, true).mask().to_vec() == Bits({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}));   // both interior footprints hold a hole
        }
        {  // the majority: the least of the classes that tie, a strict majority, clipped corners
            const CellBuffer c = CellBuffer::from_vec<uint8_t>({1, 1, 2, 2,  //
                                                                3, 1, 2, 3,  //
                                                                3, 3, 2, 2});
            const U8 got = c.focal_majority(4).to_vec<uint8_t>();
            // (1, 1): three each of 1, 2 and 3 -> 1.  (1, 2): five 2s.  (0, 0): 1 1 3 1 -> 1.  (2, 0): 3 1 3 3 -> 3.  (0, 3): 2 2 2 3 -> 2
            CHECK(got[5] == 1 && got[6] == 2 && got[0] == 1 && got[8] == 3 && got[3] == 2);
            CHECK(c.focal_majority(4, {0, 0}).to_vec<uint8_t>() == c.to_vec<uint8_t>());
            const MaskedCellBuffer w = c.focal_majority_whole(4);
            CHECK(w.mask().to_vec() == Bits({0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0}) && w.buffer().to_vec<uint8_t>() == U8({0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0}));
            // with the three 1s of (1, 1)'s footprint masked out, 2 and 3 tie at three: the least, 2
            const MaskedCellBuffer m(c.clone(), Mask::new_({0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1}));
            const MaskedCellBuffer mm = m.focal_majority(4);
            CHECK(mm.buffer().to_vec<uint8_t>()[5] == 2 && mm.mask().to_vec()[5] && mm.mask().to_vec()[0]);
            CHECK(m.focal_majority(4, {1, 1}, true).mask().to_vec() == Bits({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
        }
        {  // "equal" is equal bits: -0.0 and 0.0 are different keys; the total order puts -0.0 first and a positive NaN last
            const CellBuffer z = CellBuffer::from_vec<double>({0.0, -0.0, -0.0, NAN, 1.0});
            const std::vector<double> mj = z.focal_majority(5, {2, 0}).to_vec<double>();
            CHECK(mj[2] == 0.0 && std::signbit(mj[2]));   // -0.0 twice, every other key once
            CHECK(mj[0] == 0.0 && std::signbit(mj[0]));   // 0.0 -0.0 -0.0
            CHECK(mj[4] == 0.0 && std::signbit(mj[4]));   // -0.0 nan 1.0, one each: the least key
            const std::vector<double> md = z.focal_median(5, {2, 0}).to_vec<double>();
            CHECK(md[2] == 0.0 && !std::signbit(md[2]));  // -0.0 -0.0 0.0 1.0 nan: the middle one is +0.0
            CHECK(std::isnan(z.focal_rank(5, {1, 1}, EC_RANK_LOWER, {1, 0}).to_vec<double>()[4]));   // the greatest of nan 1.0
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer a = CellBuffer::from_vec<uint8_t>({1, 2, 3, 4});
            bool threw = false;
            try { a.focal_median(2, {4, 4}); } catch (const Error&) { threw = true; }   // 81 taps
            CHECK(threw);
            threw = false;
            try { a.focal_majority(2, {7, 2}); } catch (const Error&) { threw = true; }  // 75 taps
            CHECK(threw);
            threw = false;
            try { a.focal_rank(2, {3, 2}); } catch (const Error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { a.focal_rank(2, {1, 2}, static_cast<ec_rank_method>(2)); } catch (const Error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { a.focal_majority(3); } catch (const std::logic_error&) { threw = true; }
            CHECK(threw);
            CHECK(CellBuffer::from_vec<uint8_t>({}).focal_median(0).len() == 0 && CellBuffer::from_vec<uint8_t>({}).focal_majority(0).len() == 0);
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
