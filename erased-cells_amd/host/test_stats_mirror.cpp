// test_stats_mirror.cpp — CellBuffer::stats / MaskedCellBuffer::stats / sharded::ShardedCellBuffer::stats of the C++ host mirror (needs an
// MI355X) on cells whose answer can be worked out by hand, and against ec_stats_device + ec_stats_fold called directly.
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

int main() {
    try {
        init(0);
        {  // 2 4 4 4 5 5 7 9: mean 5, population stddev 2
            const Stats st = CellBuffer::from_vec<uint8_t>({2, 4, 4, 4, 5, 5, 7, 9}).stats();
            CHECK(st.count == 8 && st.sum == 40.0 && st.mean == 5.0 && st.stddev == 2.0);
            CHECK(st.min == CellValue(uint8_t(2)) && st.max == CellValue(uint8_t(9)));
        }
        {  // a masked-out NaN contributes nothing; the pivot keeps the variance of 1e9-offset cells
            const MaskedCellBuffer mb(CellBuffer::from_vec<double>({1e9 + 1.0, NAN, 1e9 + 3.0}), Mask::new_({true, false, true}));
            const Stats ms = mb.stats();
            CHECK(ms.count == 2 && ms.mean == 1e9 + 2.0 && ms.stddev == 1.0 && ms.sum == 2e9 + 4.0);
            CHECK(ms.min == CellValue(1e9 + 1.0) && ms.max == CellValue(1e9 + 3.0));
        }
        {  // nothing counted: the sentinels, sum 0, NaN mean and stddev
            const Stats e = CellBuffer(CellType::Int16, 0).stats();
            CHECK(e.count == 0 && e.sum == 0.0 && std::isnan(e.mean) && std::isnan(e.stddev));
            CHECK(e.min == CellValue(int16_t(32767)) && e.max == CellValue(int16_t(-32768)));
        }
        {  // the C ABI directly: one record on the device, downloaded, folded on the host
            std::vector<int32_t> v(100000);
            long long sum = 0;
            for (size_t i = 0; i < v.size(); ++i) { v[i] = static_cast<int32_t>(i % 1001) - 500; sum += v[i]; }
            const CellBuffer buf = CellBuffer::from_vec(v);
            void* rec_dev = nullptr;
            check(ec_alloc(&rec_dev, sizeof(ec_moments)));
            check(ec_stats_device(EC_I32, buf.ptr(), nullptr, buf.len(), rec_dev, current_stream()));
            ec_moments rec;
            check(ec_download(&rec, rec_dev, sizeof rec, current_stream()));
            check(ec_free(rec_dev));
            CHECK(rec.count == v.size() && rec.kind == 0 && rec.dtype == EC_I32 && rec.u.i.sum == sum && rec.reserved == 0);
            ec_stats folded;
            check(ec_stats_fold(&rec, 1, &folded));
            const Stats st = buf.stats();
            CHECK(st.count == folded.count && st.sum == folded.sum && st.mean == folded.mean && st.stddev == folded.stddev);
            CHECK(st.min == CellValue(folded.min) && st.max == CellValue(folded.max) && st.min == CellValue(int32_t(-500)));
        }
        {  // sharded over the one GPU listed three times: exact integers do not depend on the cut
            std::vector<uint16_t> v(3 * 7 * 11);
            for (size_t i = 0; i < v.size(); ++i) v[i] = static_cast<uint16_t>((i * 2654435761u) >> 16);
            const Stats whole = CellBuffer::from_vec(v).stats();
            sharded::ShardGroup group({0, 0, 0}, EC_GROUP_HOST_COMBINE);
            const Stats cut = sharded::ShardedCellBuffer::scatter(group, v, 21, 11).stats();
            CHECK(cut.count == whole.count && cut.sum == whole.sum && cut.min == whole.min && cut.max == whole.max);
            CHECK(cut.mean == whole.mean && cut.stddev == whole.stddev);  // integer records add exactly
            // masked: every third cell hidden, on both sides
            std::vector<uint8_t> m(v.size());
            std::vector<bool> mb(v.size());
            for (size_t i = 0; i < v.size(); ++i) mb[i] = (m[i] = i % 3 != 0) != 0;
            const Stats mwhole = MaskedCellBuffer(CellBuffer::from_vec(v), Mask::new_(mb)).stats();
            const sharded::ShardedCellBuffer sm = sharded::ShardedCellBuffer::scatter(group, m, 21, 11);
            const Stats mcut = sharded::ShardedCellBuffer::scatter(group, v, 21, 11).stats(&sm);
            CHECK(mcut.count == mwhole.count && mcut.count == v.size() - v.size() / 3 && mcut.sum == mwhole.sum);
            CHECK(mcut.mean == mwhole.mean && mcut.stddev == mwhole.stddev && mcut.min == mwhole.min && mcut.max == mwhole.max);
        }
        std::printf("%d checks passed\n", g_checks);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
