// test_compare_mirror.cpp — CellBuffer::compare / MaskedCellBuffer::compare / select / or_else / sharded compare of the C++ host
// mirror (needs an MI355X) on cells whose answer can be worked out by hand.
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
        {  // ndvi > 0.3, qa == 4, nir < red
            const CellBuffer ndvi = CellBuffer::from_vec<double>({0.1, 0.3, 0.31, -0.0, NAN});
            CHECK(ndvi.compare(EC_CMP_GT, CellValue(0.3)).to_vec() == Bits({false, false, true, false, true}));  // a positive NaN is above +inf
            CHECK(ndvi.compare(EC_CMP_LT, CellValue(0.0)).to_vec() == Bits({false, false, false, true, false})); // -0.0 < +0.0
            const CellBuffer qa = CellBuffer::from_vec<uint8_t>({4, 5, 4, 0});
            CHECK(qa.compare(EC_CMP_EQ, CellValue(int32_t(4))).to_vec() == Bits({true, false, true, false}));
            const CellBuffer nir = CellBuffer::from_vec<uint16_t>({10, 20, 30}), red = CellBuffer::from_vec<int16_t>({11, 20, -1, 7});
            CHECK(nir.compare(EC_CMP_LT, red).to_vec() == Bits({true, false, false}));                           // zip-truncated
            CHECK(nir.compare(EC_CMP_GE, red).to_vec() == Bits({false, true, true}));
        }
        {  // the union decides: u64 2^53 + 1 against i64 2^53 is Equal (Float64), i64 against i64 is not
            const uint64_t big = (uint64_t(1) << 53) + 1;
            const CellBuffer u = CellBuffer::from_vec<uint64_t>({big}), i = CellBuffer::from_vec<int64_t>({int64_t(1) << 53});
            CHECK(u.compare(EC_CMP_EQ, i).to_vec() == Bits({true}));
            CHECK(CellBuffer::from_vec<int64_t>({int64_t(big)}).compare(EC_CMP_EQ, i).to_vec() == Bits({false}));
        }
        {  // masked: a cell that is not valid satisfies no predicate
            const MaskedCellBuffer a(CellBuffer::from_vec<float>({1.f, 2.f, 3.f, 4.f}), Mask::new_({true, false, true, true}));
            const MaskedCellBuffer b(CellBuffer::from_vec<uint8_t>({0, 0, 9, 0}), Mask::new_({true, true, true, false}));
            CHECK(a.compare(EC_CMP_GT, b).to_vec() == Bits({true, false, false, false}));
            CHECK(a.compare(EC_CMP_NE, CellValue(1.0f)).to_vec() == Bits({false, false, true, true}));
            // cloud fill: a where a is valid, else b with b's validity
            const MaskedCellBuffer f = a.or_else(b);
            CHECK(f.cell_type() == CellType::Float32 && f.to_vec<float>() == std::vector<float>({1.f, 0.f, 3.f, 4.f}));
            CHECK(f.mask().to_vec() == Bits({true, true, true, true}));
            const MaskedCellBuffer g = b.or_else(a);
            CHECK(g.to_vec<float>() == std::vector<float>({0.f, 0.f, 9.f, 4.f}) && g.mask().to_vec() == Bits({true, true, true, true}));
        }
        {  // select: cells picked by a mask, moved by width; all true / all false are copies
            const CellBuffer a = CellBuffer::from_vec<int32_t>({1, 2, 3, 4, 5}), b = CellBuffer::from_vec<int32_t>({-1, -2, -3, -4, -5});
            CHECK(select(Mask::new_({true, false, false, true, true}), a, b).to_vec<int32_t>() == std::vector<int32_t>({1, -2, -3, 4, 5}));
            CHECK(select(Mask::fill(5, true), a, b) == a && select(Mask::fill(5, false), a, b) == b);
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer a = CellBuffer::from_vec<uint8_t>({1});
            bool threw = false;
            try { a.compare(static_cast<ec_cmp>(7), a); } catch (const Error&) { threw = true; }
            CHECK(threw);
        }
        {  // sharded over the one GPU listed three times, against the whole-raster call
            std::vector<uint16_t> v(3 * 7 * 11);
            std::vector<float> w(v.size());
            for (size_t i = 0; i < v.size(); ++i) { v[i] = static_cast<uint16_t>((i * 2654435761u) >> 16); w[i] = float((i * 40503u) & 0xffff); }
            sharded::ShardGroup group({0, 0, 0}, EC_GROUP_HOST_COMBINE);
            const auto sv = sharded::ShardedCellBuffer::scatter(group, v, 21, 11), sw = sharded::ShardedCellBuffer::scatter(group, w, 21, 11);
            const std::vector<uint8_t> cut = sv.compare(EC_CMP_LE, sw).to_vec<uint8_t>();
            const Bits whole = CellBuffer::from_vec(v).compare(EC_CMP_LE, CellBuffer::from_vec(w)).to_vec();
            CHECK(Bits(cut.begin(), cut.end()) == whole);
            const std::vector<uint8_t> cut_s = sv.compare(EC_CMP_GT, CellValue(uint16_t(30000))).to_vec<uint8_t>();
            CHECK(Bits(cut_s.begin(), cut_s.end()) == CellBuffer::from_vec(v).compare(EC_CMP_GT, CellValue(uint16_t(30000))).to_vec());
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
