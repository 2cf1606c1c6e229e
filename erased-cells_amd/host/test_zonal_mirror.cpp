// test_zonal_mirror.cpp — zonal_stats() and broadcast() of the C++ host mirror, whole-buffer, masked and sharded (needs an MI355X), on
// cells whose answer can be worked out by hand and against the C ABI called directly.
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
        {  // twelve cells, three zones, one foreign id (255), one NaN under a cleared mask byte
            const std::vector<float> v = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f, NAN, 10.f, 11.f, 12.f};
            const std::vector<uint8_t> z = {0, 0, 1, 1, 2, 2, 0, 255, 1, 2, 1, 0};
            const Bits valid = {true, true, true, true, true, true, true, true, false, true, true, true};
            const CellBuffer values = CellBuffer::from_vec(v), zones = CellBuffer::from_vec(z);
            const MaskedCellBuffer masked(values.clone(), Mask::new_(valid));
            const std::vector<Stats> st = masked.zonal_stats(zones, 3);
            CHECK(st.size() == 3);
            CHECK(st[0].count == 4 && st[0].sum == 22.0 && st[0].mean == 5.5);   // 1 2 7 12
            CHECK(st[1].count == 3 && st[1].sum == 18.0 && st[1].mean == 6.0);   // 3 4 11; the NaN is hidden
            CHECK(st[2].count == 3 && st[2].sum == 21.0 && st[2].mean == 7.0);   // 5 6 10; the 8 belongs to no zone
            CHECK(st[0].stddev == std::sqrt((20.25 + 12.25 + 2.25 + 42.25) / 4.0));
            const std::vector<Stats> open = values.zonal_stats(zones, 3);         // unmasked: the NaN reaches zone 1 and nothing else
            CHECK(open[0].sum == 22.0 && open[2].sum == 21.0 && open[1].count == 4 && std::isnan(open[1].mean));
            const std::vector<Stats> four = masked.zonal_stats(zones, 4);         // an empty zone: the empty record's figures
            CHECK(four[3].count == 0 && four[3].sum == 0.0 && std::isnan(four[3].mean) && four[2].sum == 21.0);
            // against the C ABI called directly
            std::vector<ec_stats> raw(3);
            check(ec_zonal_stats_compute(EC_F32, values.ptr(), masked.mask().ptr(), EC_U8, zones.ptr(), v.size(), 3, raw.data(), current_stream()));
            for (int k = 0; k < 3; ++k)
                CHECK(raw[k].count == st[k].count && std::memcmp(&raw[k].sum, &st[k].sum, 8) == 0 && std::memcmp(&raw[k].stddev, &st[k].stddev, 8) == 0);
            // the way back: the anomaly against the zone's mean
            const std::vector<double> means = {st[0].mean, st[1].mean, st[2].mean};
            const MaskedCellBuffer back = zones.broadcast(CellBuffer::from_vec(means));
            CHECK(back.cell_type() == CellType::Float64);
            CHECK(back.to_vec<double>() == std::vector<double>({5.5, 5.5, 6.0, 6.0, 7.0, 7.0, 5.5, 0.0, 6.0, 7.0, 6.0, 5.5}));
            CHECK(back.mask().to_vec() == Bits({true, true, true, true, true, true, true, false, true, true, true, true}));
        }
        {  // negative ids and ids at n_zones belong to no zone; u16 and i32 zone rasters
            const CellBuffer values = CellBuffer::from_vec<int16_t>({-3, 5, 7, 9, -11});
            const std::vector<Stats> a = values.zonal_stats(CellBuffer::from_vec<int32_t>({-1, 1, 2, 1, INT32_MIN}), 2);
            CHECK(a[0].count == 0 && a[1].count == 2 && a[1].sum == 14.0);
            const std::vector<Stats> b = values.zonal_stats(CellBuffer::from_vec<uint16_t>({0, 1, 65535, 1, 0}), 2);
            CHECK(b[0].count == 2 && b[0].sum == -14.0 && b[1].sum == 14.0);
        }
        {  // refusals come back as errors, before any launch
            const CellBuffer v = CellBuffer::from_vec<uint8_t>({1, 2}), z = CellBuffer::from_vec<uint8_t>({0, 1}), zl = CellBuffer::from_vec<uint8_t>({0}),
                             zf = CellBuffer::from_vec<float>({0.f, 1.f});
            int threw = 0;
            try { v.zonal_stats(z, 0); } catch (const Error&) { ++threw; }
            try { v.zonal_stats(z, 257); } catch (const Error&) { ++threw; }
            try { v.zonal_stats(zl, 2); } catch (const Error&) { ++threw; }
            try { v.zonal_stats(zf, 2); } catch (const Error&) { ++threw; }
            try { zf.broadcast(v); } catch (const Error&) { ++threw; }
            CHECK(threw == 5);
        }
        {  // sharded over the one GPU listed three times, against the whole-raster call
            std::vector<int16_t> v(3 * 7 * 11);
            std::vector<uint8_t> z(v.size()), m(v.size());
            for (size_t i = 0; i < v.size(); ++i) {
                v[i] = static_cast<int16_t>((i * 2654435761u) >> 16);
                z[i] = static_cast<uint8_t>((i / 5) % 7);  // 5 and 6: foreign for five zones
                m[i] = (i * 7) % 3 != 0;
            }
            sharded::ShardGroup group({0, 0, 0}, EC_GROUP_HOST_COMBINE);
            using SB = sharded::ShardedCellBuffer;
            const SB sv = SB::scatter(group, v, 21, 11), sz = SB::scatter(group, z, 21, 11), sm = SB::scatter(group, m, 21, 11);
            const CellBuffer bv = CellBuffer::from_vec(v), bz = CellBuffer::from_vec(z);
            const MaskedCellBuffer qv(bv.clone(), Mask::new_(Bits(m.begin(), m.end())));
            const std::vector<Stats> whole = bv.zonal_stats(bz, 5), cut = sv.zonal_stats(sz, 5);
            const std::vector<Stats> mwhole = qv.zonal_stats(bz, 5), mcut = sv.zonal_stats(sz, 5, &sm);
            for (int k = 0; k < 5; ++k) {  // kind 0: the cut does not matter to the count and the sum
                CHECK(cut[k].count == whole[k].count && cut[k].sum == whole[k].sum && cut[k].min == whole[k].min && cut[k].max == whole[k].max);
                CHECK(mcut[k].count == mwhole[k].count && mcut[k].sum == mwhole[k].sum && mcut[k].count < whole[k].count);
            }
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
