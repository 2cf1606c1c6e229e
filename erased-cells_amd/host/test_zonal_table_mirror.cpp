// test_zonal_table_mirror.cpp — zonal_table() and lookup() of the C++ host mirror, whole-buffer, masked and sharded (needs an MI355X), on
// hand-checkable cells, with more than 256 zones, and against the C ABI called directly.
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
        {  // twelve cells, zones 0, 1 and 300, one foreign id (301), one NaN under a cleared mask byte
            const std::vector<float> v = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f, NAN, 10.f, 11.f, 12.f};
            const std::vector<uint16_t> z = {0, 0, 1, 1, 300, 300, 0, 301, 1, 300, 1, 0};
            const Bits valid = {true, true, true, true, true, true, true, true, false, true, true, true};
            const CellBuffer values = CellBuffer::from_vec(v), zones = CellBuffer::from_vec(z);
            const MaskedCellBuffer masked(values.clone(), Mask::new_(valid));
            const std::vector<ec_stats> st = masked.zonal_table(zones, 301);
            CHECK(st.size() == 301);
            CHECK(st[0].count == 4 && st[0].sum == 22.0 && st[0].mean == 5.5);       // 1 2 7 12
            CHECK(st[1].count == 3 && st[1].sum == 18.0 && st[1].mean == 6.0);       // 3 4 11; the NaN is hidden
            CHECK(st[300].count == 3 && st[300].sum == 21.0 && st[300].mean == 7.0); // 5 6 10; the 8 belongs to no zone
            CHECK(st[0].stddev == std::sqrt((20.25 + 12.25 + 2.25 + 42.25) / 4.0));
            CHECK(st[2].count == 0 && st[2].sum == 0.0 && std::isnan(st[2].mean) && st[299].count == 0);
            const Stats first(st[0]);                                                 // one row as the mirror's Stats
            CHECK(first.count == 4 && first.mean == 5.5);
            const std::vector<ec_stats> open = values.zonal_table(zones, 301);        // unmasked: the NaN reaches zone 1 and nothing else
            CHECK(open[0].sum == 22.0 && open[300].sum == 21.0 && open[1].count == 4 && std::isnan(open[1].mean));
            // against the C ABI called directly
            std::vector<ec_stats> raw(301);
            check(ec_zonal_table_compute(EC_F32, values.ptr(), masked.mask().ptr(), EC_U16, zones.ptr(), v.size(), 301, raw.data(), current_stream()));
            CHECK(std::memcmp(raw.data(), st.data(), raw.size() * sizeof(ec_stats)) == 0);
            // the way back, through a table longer than ec_zonal_broadcast takes
            std::vector<double> means(301, -1.0);
            means[0] = st[0].mean, means[1] = st[1].mean, means[300] = st[300].mean;
            const MaskedCellBuffer back = zones.lookup(CellBuffer::from_vec(means));
            CHECK(back.cell_type() == CellType::Float64);
            CHECK(back.to_vec<double>() == std::vector<double>({5.5, 5.5, 6.0, 6.0, 7.0, 7.0, 5.5, 0.0, 6.0, 7.0, 6.0, 5.5}));
            CHECK(back.mask().to_vec() == Bits({true, true, true, true, true, true, true, false, true, true, true, true}));
        }
        {  // negative ids and ids at n_zones belong to no zone; a sum that truncates: 2^70 with 1.5s in one zone
            const CellBuffer values = CellBuffer::from_vec<int16_t>({-3, 5, 7, 9, -11});
            const std::vector<ec_stats> a = values.zonal_table(CellBuffer::from_vec<int32_t>({-1, 1, 2, 1, INT32_MIN}), 2);
            CHECK(a[0].count == 0 && a[1].count == 2 && a[1].sum == 14.0);
            const CellBuffer big = CellBuffer::from_vec<double>({0.0, std::ldexp(1.0, 70), 1.5, 1.5, 1.5, 3.0});
            const std::vector<ec_stats> t = big.zonal_table(CellBuffer::from_vec<int32_t>({9, 400, 400, 400, 400, 7}), 401);
            CHECK(t[400].count == 4 && t[400].sum == std::ldexp(1.0, 70) && t[7].sum == 3.0 && t[9].count == 1 && t[9].sum == 0.0);   // the pivot is cell 0's 0.0
        }
        {  // refusals come back as errors, before any launch; the first family keeps its own
            const CellBuffer v = CellBuffer::from_vec<uint8_t>({1, 2}), z = CellBuffer::from_vec<uint8_t>({0, 1}), zl = CellBuffer::from_vec<uint8_t>({0}),
                             zf = CellBuffer::from_vec<float>({0.f, 1.f});
            int threw = 0;
            try { v.zonal_table(z, 0); } catch (const Error&) { ++threw; }
            try { v.zonal_table(z, EC_ZONAL_TABLE_MAX_ZONES + 1); } catch (const Error&) { ++threw; }
            try { v.zonal_table(zl, 2); } catch (const Error&) { ++threw; }
            try { v.zonal_table(zf, 2); } catch (const Error&) { ++threw; }
            try { zf.lookup(v); } catch (const Error&) { ++threw; }
            try { v.zonal_stats(z, 257); } catch (const Error&) { ++threw; }
            CHECK(threw == 6);
            CHECK(v.zonal_table(z, 257).size() == 257);
        }
        {  // sharded over the one GPU listed three times, against the whole-raster call: 700 zones
            std::vector<int16_t> v(3 * 7 * 11);
            std::vector<uint16_t> z(v.size());
            std::vector<uint8_t> m(v.size());
            for (size_t i = 0; i < v.size(); ++i) {
                v[i] = static_cast<int16_t>((i * 2654435761u) >> 16);
                z[i] = static_cast<uint16_t>(((i / 5) % 7) * 100);  // 0, 100 .. 600
                m[i] = (i * 7) % 3 != 0;
            }
            sharded::ShardGroup group({0, 0, 0}, EC_GROUP_HOST_COMBINE);
            using SB = sharded::ShardedCellBuffer;
            const SB sv = SB::scatter(group, v, 21, 11), sz = SB::scatter(group, z, 21, 11), sm = SB::scatter(group, m, 21, 11);
            const CellBuffer bv = CellBuffer::from_vec(v), bz = CellBuffer::from_vec(z);
            const MaskedCellBuffer qv(bv.clone(), Mask::new_(Bits(m.begin(), m.end())));
            const std::vector<ec_stats> whole = bv.zonal_table(bz, 700), cut = sv.zonal_table(sz, 700);
            const std::vector<ec_stats> mwhole = qv.zonal_table(bz, 700), mcut = sv.zonal_table(sz, 700, &sm);
            CHECK(std::memcmp(whole.data(), cut.data(), whole.size() * sizeof(ec_stats)) == 0);     // kind 0: the cut does not matter
            CHECK(std::memcmp(mwhole.data(), mcut.data(), whole.size() * sizeof(ec_stats)) == 0);
            CHECK(whole[600].count > 0 && whole[599].count == 0 && mcut[600].count < whole[600].count);
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
