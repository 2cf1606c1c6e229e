// test_cast_mirror.cpp — CellBuffer::cast / to_scaled, MaskedCellBuffer::cast / to_scaled and the sharded cast of the C++ host
// mirror (needs an MI355X) on cells whose answer can be worked out by hand.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

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

int main() {
    try {
        init(0);
        const double inf = std::numeric_limits<double>::infinity();
        {  // the storing rule and Rust's `as`, float to integer
            const CellBuffer f = CellBuffer::from_vec<double>({0.5, 1.5, 2.5, -0.5, -2.5, 0.49999999999999994, NAN, 300.0, -inf, 254.5});
            CHECK(f.cast(CellType::UInt8).to_vec<uint8_t>() == std::vector<uint8_t>({1, 2, 3, 0, 0, 1, 0, 255, 0, 255}));
            CHECK(f.cast(CellType::UInt8, EC_CAST_AS).to_vec<uint8_t>() == std::vector<uint8_t>({0, 1, 2, 0, 0, 0, 0, 255, 0, 254}));
            CHECK(f.cast(CellType::Int8).to_vec<int8_t>() == std::vector<int8_t>({1, 2, 3, -1, -3, 1, 0, 127, -128, 127}));
            const CellBuffer big = CellBuffer::from_vec<double>({9223372036854775808.0, -9223372036854775808.0, 18446744073709551616.0});
            CHECK(big.cast(CellType::Int64).to_vec<int64_t>() == std::vector<int64_t>({INT64_MAX, INT64_MIN, INT64_MAX}));
            CHECK(big.cast(CellType::UInt64).to_vec<uint64_t>() == std::vector<uint64_t>({uint64_t(1) << 63, 0, UINT64_MAX}));
        }
        {  // integer to integer: clamped exactly (no detour through f64), or the low bits
            const int64_t odd = (int64_t(1) << 53) + 1;
            const CellBuffer i = CellBuffer::from_vec<int64_t>({odd, -1, 300, -300});
            CHECK(i.cast(CellType::UInt64).to_vec<uint64_t>() == std::vector<uint64_t>({uint64_t(odd), 0, 300, 0}));
            CHECK(i.cast(CellType::UInt64, EC_CAST_AS).to_vec<uint64_t>() == std::vector<uint64_t>({uint64_t(odd), UINT64_MAX, 300, uint64_t(-300)}));
            CHECK(i.cast(CellType::UInt8).to_vec<uint8_t>() == std::vector<uint8_t>({255, 0, 255, 0}));
            CHECK(i.cast(CellType::UInt8, EC_CAST_AS).to_vec<uint8_t>() == std::vector<uint8_t>({1, 255, 44, 212}));
            CHECK(i.cast(CellType::Float32).to_vec<float>() == std::vector<float>({9007199254740992.0f, -1.0f, 300.0f, -300.0f}));
        }
        {  // a pair that fits is convert, in either mode
            const CellBuffer u = CellBuffer::from_vec<uint8_t>({0, 7, 255});
            CHECK(u.cast(CellType::Float64) == u.convert(CellType::Float64) && u.cast(CellType::Int16, EC_CAST_AS) == u.convert(CellType::Int16));
        }
        {  // scaled: i16 by 10000 with a nodata value; two roundings, never an fma
            const CellBuffer ndvi = CellBuffer::from_vec<double>({0.12344, -0.5, 0.99996, NAN, 7.0});
            CHECK(ndvi.to_scaled(CellType::Int16, 10000.0, 0.0).to_vec<int16_t>() == std::vector<int16_t>({1234, -5000, 10000, 0, 32767}));
            const MaskedCellBuffer m(ndvi.clone(), Mask::new_({true, true, false, false, true}));
            CHECK(m.to_scaled(CellType::Int16, 10000.0, 0.0, CellValue(int16_t(-9999))).to_vec<int16_t>() ==
                  std::vector<int16_t>({1234, -5000, -9999, -9999, 32767}));
            const MaskedCellBuffer c = m.cast(CellType::Int8);
            CHECK(c.cell_type() == CellType::Int8 && c.to_vec<int8_t>() == std::vector<int8_t>({0, -1, 1, 0, 7}));
            CHECK(c.mask().to_vec() == std::vector<bool>({true, true, false, false, true}));
            CHECK(CellBuffer::from_vec<double>({0.1}).to_scaled(CellType::Float64, 10.0, -1.0).to_vec<double>() == std::vector<double>({0.0}));
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer a = CellBuffer::from_vec<double>({1.0});
            bool threw = false;
            try { a.cast(CellType::UInt8, static_cast<ec_cast_mode>(2)); } catch (const Error&) { threw = true; }
            CHECK(threw);
            threw = false;
            try { a.to_scaled(CellType::UInt8, NAN, 0.0); } catch (const Error&) { threw = true; }
            CHECK(threw);
            const CellValue wrong(int32_t(-9999));
            const MaskedCellBuffer m(a.clone(), Mask::new_({true}));
            threw = false;
            try { m.to_scaled(CellType::Int16, 1.0, 0.0, wrong); } catch (const Error&) { threw = true; }
            CHECK(threw);
        }
        {  // sharded over the one GPU listed three times, against the whole-raster call
            std::vector<float> w(3 * 7 * 11);
            for (size_t i = 0; i < w.size(); ++i) w[i] = float(int((i * 40503u) & 0xffff) - 32768) / 64.0f;
            sharded::ShardGroup group({0, 0, 0}, EC_GROUP_HOST_COMBINE);
            const auto sw = sharded::ShardedCellBuffer::scatter(group, w, 21, 11);
            const CellBuffer whole = CellBuffer::from_vec(w);
            CHECK(sw.cast(CellType::Int8).to_vec<int8_t>() == whole.cast(CellType::Int8).to_vec<int8_t>());
            CHECK(sw.cast(CellType::UInt16, EC_CAST_AS).to_vec<uint16_t>() == whole.cast(CellType::UInt16, EC_CAST_AS).to_vec<uint16_t>());
            CHECK(sw.to_scaled(CellType::Int16, 100.0, 0.5).to_vec<int16_t>() == whole.to_scaled(CellType::Int16, 100.0, 0.5).to_vec<int16_t>());
            std::vector<uint8_t> mb(w.size());
            std::vector<bool> mv(w.size());
            for (size_t i = 0; i < w.size(); ++i) mv[i] = (mb[i] = uint8_t((i * 7u) % 3u != 0));
            const auto sm = sharded::ShardedCellBuffer::scatter(group, mb, 21, 11);
            const CellValue nd(int16_t(-9999));
            const MaskedCellBuffer mw(whole.clone(), Mask::new_(mv));
            CHECK(sw.to_scaled(CellType::Int16, 100.0, 0.5, &sm, &nd).to_vec<int16_t>() == mw.to_scaled(CellType::Int16, 100.0, 0.5, nd).to_vec<int16_t>());
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
