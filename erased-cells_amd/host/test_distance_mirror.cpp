// test_distance_mirror.cpp — Mask::distance and Mask::within of the C++ host mirror (needs an MI355X) on cells whose answer can be
// worked out by hand.
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
using U32 = std::vector<uint32_t>;

int main() {
    try {
        init(0);
        {  // a 4 x 3 mask with targets at (0, 0) and (2, 3)
            const Mask m = Mask::new_({1, 0, 0, 0,  //
                                       0, 0, 0, 0,  //
                                       0, 0, 0, 1});
            const MaskedCellBuffer sq = m.distance(4, std::numeric_limits<double>::infinity(), true);
            CHECK(sq.cell_type() == CellType::UInt32 && sq.len() == 12);
            CHECK(sq.buffer().to_vec<uint32_t>() == U32({0, 1, 4, 4,  //
                                                        1, 2, 2, 1,  //
                                                        4, 4, 1, 0}));
            CHECK(sq.mask().to_vec() == Bits({1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}));
            const MaskedCellBuffer d = m.distance(4);
            CHECK(d.cell_type() == CellType::Float64);
            const std::vector<double> dv = d.buffer().to_vec<double>();
            CHECK(dv[0] == 0.0 && dv[1] == 1.0 && dv[2] == 2.0 && dv[5] == std::sqrt(2.0) && dv[11] == 0.0);
            // the greatest distance is inclusive
            const MaskedCellBuffer near = m.distance(4, 1.0, true);
            CHECK(near.mask().to_vec() == Bits({1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1}));
            CHECK(near.buffer().to_vec<uint32_t>() == U32({0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0}));
            CHECK(m.within(4, 1.4).to_vec() == Bits({1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1}));
            CHECK(m.within(4, 1.5).to_vec() == Bits({1, 1, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1}));
            CHECK(m.within(4, 0).to_vec() == Bits({1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}));
            CHECK(m.within(4, 2).to_vec() == Bits({1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}));
        }
        {  // within(sqrt 2 rounded up) is the 3 x 3 dilation, within(1) the 4-neighbourhood
            const Mask m = Mask::new_({0, 0, 0, 0, 0,  //
                                       0, 0, 1, 0, 0,  //
                                       0, 0, 0, 0, 0});
            CHECK(m.within(5, 1.4143) == m.dilate(5));
            CHECK(m.within(5, 1).to_vec() == Bits({0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0}));
        }
        {  // no target: every cell invalid, zero bits
            const Mask none = Mask::fill(6, false);
            const MaskedCellBuffer d = none.distance(3);
            CHECK(d.mask().to_vec() == Bits({0, 0, 0, 0, 0, 0}));
            for (double v : d.buffer().to_vec<double>()) CHECK(v == 0.0 && !std::signbit(v));
            CHECK(none.within(3, 100).to_vec() == Bits({0, 0, 0, 0, 0, 0}));
        }
        {  // max_sq_of is floor(d^2), exactly
            CHECK(Mask::max_sq_of(0) == 0 && Mask::max_sq_of(1) == 1 && Mask::max_sq_of(1.5) == 2 && Mask::max_sq_of(50) == 2500);
            // the double nearest to the root of 2 lies above it: its square reaches 2, the next double below does not
            CHECK(Mask::max_sq_of(std::sqrt(2.0)) == 2 && Mask::max_sq_of(std::nextafter(std::sqrt(2.0), 0.0)) == 1);
            CHECK(Mask::max_sq_of(65535.5) == 4294901760u && Mask::max_sq_of(65536) == EC_DISTANCE_UNLIMITED);
            CHECK(Mask::max_sq_of(std::numeric_limits<double>::infinity()) == EC_DISTANCE_UNLIMITED);
        }
        {  // refusals
            const Mask m = Mask::new_({1, 0, 0, 1});
            bool threw = false;
            try { m.distance(3); } catch (const std::logic_error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { m.within(2, -1); } catch (const Error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { m.within(2, NAN); } catch (const Error&) { threw = true; }
            CHECK(threw);
            CHECK(Mask::fill(0, false).distance(0).len() == 0 && Mask::fill(0, false).within(0, 1).len() == 0);
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
