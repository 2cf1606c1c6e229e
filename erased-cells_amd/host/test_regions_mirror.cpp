// test_regions_mirror.cpp — regions and sieve of the C++ host mirror (needs an MI355X) on cells whose answer can be worked out by hand.
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
using I32 = std::vector<int32_t>;

int main() {
    try {
        init(0);
        {  // a U whose arms meet only in the last row, and a diagonal pair
            const Mask m = Mask::new_({1, 0, 1, 0, 0,  //
                                       1, 0, 1, 0, 1,  //
                                       1, 1, 1, 1, 0});
            auto [four, k4] = m.regions(5);
            CHECK(k4 == 2 && four.cell_type() == CellType::Int32);
            CHECK(four.buffer().to_vec<int32_t>() == I32({1, 0, 1, 0, 0, 1, 0, 1, 0, 2, 1, 1, 1, 1, 0}));
            CHECK(four.mask().to_vec() == Bits({1, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 0}));
            auto [eight, k8] = m.regions(5, 8);
            CHECK(k8 == 1 && eight.buffer().to_vec<int32_t>() == I32({1, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 0}));
            auto [root, kr] = m.regions(5, 4, 0, EC_REGIONS_ROOT);
            CHECK(kr == 2 && root.buffer().to_vec<int32_t>() == I32({1, 0, 1, 0, 0, 1, 0, 1, 0, 10, 1, 1, 1, 1, 0}));
            // the sieve drops the single cell; the dense numbers close up
            auto [big, kb] = m.regions(5, 4, 2);
            CHECK(kb == 1 && big.mask().to_vec() == Bits({1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0}));
            CHECK(m.sieve(5, 2).to_vec() == Bits({1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0}));
            CHECK(m.sieve(5, 2, 8) == m && m.sieve(5, 100).to_vec() == Bits(15, false));
        }
        {  // classes: equal bits; the row end does not wrap
            const CellBuffer c = CellBuffer::from_vec<uint16_t>({7, 7, 9,  //
                                                                 9, 7, 9});
            auto [lab, k] = c.regions(3);
            CHECK(k == 3 && lab.buffer().to_vec<int32_t>() == I32({1, 1, 2, 3, 1, 2}));
            const MaskedCellBuffer mc(c.clone(), Mask::new_({1, 0, 1, 1, 1, 1}));
            auto [ml, mk] = mc.regions(3);
            CHECK(mk == 4 && ml.buffer().to_vec<int32_t>() == I32({1, 0, 2, 3, 4, 2}));
            const MaskedCellBuffer s = mc.sieve(3, 2);
            CHECK(s.mask().to_vec() == Bits({0, 0, 1, 0, 0, 1}) && s.buffer() == c);
            // the labels are a zone raster
            const std::vector<Stats> z = c.zonal_stats(lab.buffer(), static_cast<int32_t>(k) + 1);
            CHECK(z[0].count == 0 && z[1].count == 3 && z[2].count == 2 && z[3].count == 1);
        }
        {  // refusals and the empty raster
            const Mask m = Mask::new_({1, 0, 0, 1});
            bool threw = false;
            try { m.regions(3); } catch (const std::logic_error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { m.regions(2, 6); } catch (const Error&) { threw = true; }
            CHECK(threw);
            CHECK(Mask::fill(0, false).regions(0).second == 0 && Mask::fill(0, false).sieve(0, 3).len() == 0);
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
