// test_reclass_mirror.cpp — classify() and reclassify() of the C++ host mirror, whole-buffer and masked (needs an MI355X), on cells
// whose answer can be worked out by hand, composed with zonal_stats() into a histogram, and against the C ABI called directly.
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

int main() {
    try {
        init(0);
        {  // NDVI into four classes; 0.2f, 0.4f and 0.6f lie just ABOVE the Float64 breaks 0.2, 0.4, 0.6: the union case
            const std::vector<float> v = {-0.5f, 0.2f, 0.25f, 0.4f, 0.59f, 0.6f, 0.9f, NAN, -NAN, -0.0f};
            const CellBuffer ndvi = CellBuffer::from_vec(v);
            const std::vector<double> edges = {0.2, 0.4, 0.6};
            const CellBuffer cls = ndvi.classify(edges);
            CHECK(cls.cell_type() == CellType::UInt8);
            CHECK(cls.to_vec<uint8_t>() == std::vector<uint8_t>({0, 1, 1, 2, 2, 3, 3, 3, 0, 0}));
            CHECK(ndvi.classify(edges, true).to_vec<uint8_t>() == std::vector<uint8_t>({0, 1, 1, 2, 2, 3, 3, 3, 0, 0}));  // no cell ties with an f64 break
            CHECK(ndvi.classify(std::vector<float>{0.2f, 0.4f, 0.6f}).to_vec<uint8_t>() == std::vector<uint8_t>({0, 1, 1, 2, 2, 3, 3, 3, 0, 0}));
            CHECK(ndvi.classify(std::vector<float>{0.2f, 0.4f, 0.6f}, true).to_vec<uint8_t>() == std::vector<uint8_t>({0, 0, 1, 1, 2, 2, 3, 3, 0, 0}));
            // a histogram by composition
            const std::vector<Stats> per_class = ndvi.zonal_stats(cls, 4);
            CHECK(per_class[0].count == 3 && per_class[1].count == 2 && per_class[2].count == 2 && per_class[3].count == 3);
            // a dropped class through MaskedCellBuffer; the NaNs hidden by the mask leave no trace
            const Bits valid_cells = {true, true, true, true, true, true, true, false, false, true};
            const MaskedCellBuffer masked(ndvi.clone(), Mask::new_(valid_cells));
            const CellValue nodata(int16_t(-1));
            const ReclassTable table(CellType::Float32, edges, std::vector<int16_t>{10, 20, -1, 40}, false, Bits{true, true, false, true}, &nodata);
            CHECK(table.drops() && table.has_nodata() && table.record().n_reached == 3 && table.result_type() == CellType::Int16);
            const MaskedCellBuffer out = masked.reclassify(table);
            CHECK(out.to_vec<int16_t>() == std::vector<int16_t>({10, 20, 20, -1, -1, 40, 40, -1, -1, 10}));
            CHECK(out.mask().to_vec() == Bits({true, true, true, false, false, true, true, false, false, true}));
            // against the C ABI called directly
            CellBuffer raw(CellType::Int16, v.size());
            Mask raw_mask(v.size());
            check(ec_reclass(EC_F32, ndvi.ptr(), masked.mask().ptr(), v.size(), EC_I16, table.ptr(), raw.ptr(), raw_mask.ptr(), current_stream()));
            CHECK(raw.to_vec<int16_t>() == out.to_vec<int16_t>() && raw_mask.to_vec() == out.mask().to_vec());
        }
        {  // a u8 raster with breaks out of its reach; a u64 cell 2^53 + 1 against u64 and f64 breaks
            const CellBuffer b = CellBuffer::from_vec<uint8_t>({0, 1, 254, 255});
            CHECK(b.classify(std::vector<double>{-1.5, 0.2, 0.7, 255.0, 300.0}).to_vec<uint8_t>() == std::vector<uint8_t>({1, 3, 3, 4}));
            const ReclassTable far(CellType::UInt8, std::vector<double>{1e9}, std::vector<uint8_t>{7, 9});
            CHECK(far.record().n_reached == 0 && b.reclassify(far).to_vec<uint8_t>() == std::vector<uint8_t>({7, 7, 7, 7}));
            const CellBuffer big = CellBuffer::from_vec<uint64_t>({9007199254740992ull, 9007199254740993ull, 9007199254740994ull});
            CHECK(big.classify(std::vector<uint64_t>{9007199254740993ull}).to_vec<uint8_t>() == std::vector<uint8_t>({0, 1, 1}));
            CHECK(big.classify(std::vector<double>{9007199254740992.0}, true).to_vec<uint8_t>() == std::vector<uint8_t>({0, 0, 1}));
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer v = CellBuffer::from_vec<uint8_t>({1, 2});
            const CellValue nd(uint8_t(0));
            int threw = 0;
            try { v.classify(std::vector<double>{}); } catch (const Error&) { ++threw; }
            try { v.classify(std::vector<double>{2.0, 1.0}); } catch (const Error&) { ++threw; }
            try { v.classify(std::vector<double>{1.0, NAN}); } catch (const Error&) { ++threw; }
            try { ReclassTable(CellType::UInt8, std::vector<uint8_t>{1}, std::vector<uint8_t>{1}); } catch (const Error&) { ++threw; }
            try { v.reclassify(ReclassTable(CellType::UInt16, std::vector<uint8_t>{1}, std::vector<uint8_t>{0, 1})); } catch (const Error&) { ++threw; }
            try { v.reclassify(ReclassTable(CellType::UInt8, std::vector<uint8_t>{1}, std::vector<uint8_t>{0, 1}, false, {}, &nd)); } catch (const Error&) { ++threw; }
            CHECK(threw == 6);
        }
        std::printf("ok: %d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
