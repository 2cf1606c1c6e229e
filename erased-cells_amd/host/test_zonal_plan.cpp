// test_zonal_plan.cpp — csrc/ec_zonal_plan.hpp and the refusals of csrc/ec_zonal_table_plan.hpp alone, under a plain C++17
// compiler (and, as test_zonal_plan_san, under the address and
// undefined-behaviour sanitizers): the LDS layout of a workgroup's tables for every n_zones (no two slots overlap, everything
// inside `bytes`, 8-byte slots 8-byte aligned), the workspace size against the most workgroups a reduction launches, where a
// partial goes, and the refusals in the order include/erased_cells.h states.  Needs no GPU and nothing from the library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "ec_zonal_plan.hpp"
#include "ec_zonal_table_plan.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

using namespace ecz;

// every slot of every table of the layout as [first byte, one past the last), 8- or 4-byte slots
static std::vector<std::pair<uint32_t, uint32_t>> slots(const LdsLayout& l, int32_t nz, int kind) {
    std::vector<std::pair<uint32_t, uint32_t>> s;
    auto table = [&](uint32_t off, int entries, uint32_t width) {
        for (int k = 0; k < entries; ++k) s.emplace_back(off + uint32_t(k) * width, off + uint32_t(k + 1) * width);
    };
    table(l.off_count, nz, 8);
    table(l.off_kmin, nz, 8);
    table(l.off_kmax, nz, 8);
    if (kind == 0) {
        table(l.off_sum, nz, 8);
        table(l.off_sq_lo, nz, 8);
        table(l.off_sq_hi, nz, 4);
    } else {
        table(l.off_s1, nz * kWaves, 8);  // wave w's entry z: (w * nz + z)
        table(l.off_s2, nz * kWaves, 8);
    }
    return s;
}

int main() {
    static_assert(kBlock == kWave * kWaves && kMaxZones == 256, "the launch constants");
    for (int kind = 0; kind < 2; ++kind)
        for (int32_t nz = 1; nz <= kMaxZones; ++nz) {
            const LdsLayout l = lds_layout(nz, kind);
            const auto s = slots(l, nz, kind);
            std::vector<uint8_t> owner(l.bytes, 0);  // a byte two slots claim shows; a slot past `bytes` is an out-of-bounds write here
            for (const auto& r : s) {
                CHECK(r.first < r.second && r.second <= l.bytes);
                CHECK((r.second - r.first == 4 ? r.first % 4 : r.first % 8) == 0);
                for (uint32_t b = r.first; b < r.second; ++b) {
                    CHECK(owner[b] == 0);
                    owner[b] = 1;
                }
            }
            CHECK(l.bytes % 8 == 0 && l.bytes <= 24u * 1024u);  // four workgroups per CU stay far inside 160 KiB, one inside 64 KiB
            CHECK(l.bytes == (kind == 0 ? ((uint32_t(nz) * 44u + 7u) & ~7u) : uint32_t(nz) * (24u + 16u * kWaves)));
        }
    CHECK(lds_layout(256, 1).bytes == 22528 && lds_layout(256, 0).bytes == 11264);

    // the workspace: a partial per zone for each of the most workgroups a reduction launches, and every partial inside it
    CHECK(workspace_bytes(0) == 0 && workspace_bytes(-1) == 0 && workspace_bytes(257) == 0);
    for (int32_t nz = 1; nz <= kMaxZones; ++nz) {
        CHECK(workspace_bytes(nz) == size_t(nz) * size_t(ecd::kMaxReduceBlocks) * kPartialBytes);
        CHECK(workspace_bytes(nz) % 64 == 0);
        for (unsigned grid : {1u, 2u, 1024u, unsigned(ecd::kMaxReduceBlocks)}) {
            CHECK(ecd::reduce_cap(1 << 20, kPerCu, 0) <= size_t(ecd::kMaxReduceBlocks));
            const size_t last = partial_index(nz - 1, grid - 1, grid);
            CHECK((last + 1) * kPartialBytes <= workspace_bytes(nz));
            CHECK(partial_index(0, 0, grid) == 0 && partial_index(nz - 1, 0, grid) == size_t(nz - 1) * grid);
        }
    }
    {  // partials of one grid never collide
        const unsigned grid = 7;
        std::vector<uint8_t> seen(size_t(5) * grid, 0);
        for (int32_t z = 0; z < 5; ++z)
            for (unsigned b = 0; b < grid; ++b) {
                CHECK(!seen[partial_index(z, b, grid)]);
                seen[partial_index(z, b, grid)] = 1;
            }
    }

    // the refusals and their order: each call below is wrong in everything that comes later as well
    char mem[4096];
    const void *P = mem, *M = mem + 1024, *Z = mem + 2048;
    char* far = reinterpret_cast<char*>(uintptr_t(1) << 40);  // never dereferenced: addresses far from `mem`
    void *OUT = far, *WS = far + (size_t(1) << 30);
    bool bad = false;
    auto why = [&](int32_t nz, size_t cell, int zt, const void* p, const void* m, const void* z, size_t n, uint64_t max_cells, const void* out,
                   const void* ws, bool caller_ws = true) {
        const ecv::Refusal r = stats_refusal(nz, cell, zt, p, m, z, n, max_cells, out, nz > 0 ? size_t(nz) * kRecordBytes : 0, ws, caller_ws);
        bad = r.bad_type;
        return r.why ? r.why : "";
    };
    CHECK(!*why(4, 2, 0, P, M, Z, 100, 0, OUT, WS) && !bad);
    CHECK(!*why(256, 8, 6, P, nullptr, Z, 100, 0, OUT, WS) && !*why(1, 1, 1, P, M, Z, 100, 0, OUT, WS));
    CHECK(std::strstr(why(0, 0, 3, nullptr, nullptr, nullptr, 100, 1, nullptr, nullptr), "n_zones") && !bad);
    CHECK(std::strstr(why(257, 0, 3, nullptr, nullptr, nullptr, 100, 1, nullptr, nullptr), "n_zones") && !bad);
    CHECK(std::strstr(why(-5, 2, 0, P, M, Z, 100, 0, OUT, WS), "n_zones"));
    CHECK(std::strstr(why(4, 0, 3, nullptr, nullptr, nullptr, 100, 1, nullptr, nullptr), "bad dtype") && bad);
    for (int zt = -1; zt < 12; ++zt) {
        const bool ok = zt == 0 || zt == 1 || zt == 6;
        CHECK(valid_zone_type(zt) == ok && (zone_size(zt) != 0) == ok);
        if (!ok) CHECK(std::strstr(why(4, 2, zt, nullptr, nullptr, nullptr, 100, 1, nullptr, nullptr), "zone raster's type") && bad);
    }
    CHECK(std::strstr(why(4, 2, 0, nullptr, M, Z, 100, 1, OUT, WS), "null pointer") && !bad);
    CHECK(std::strstr(why(4, 2, 0, P, M, nullptr, 100, 1, OUT, WS), "null pointer"));
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 1, nullptr, WS), "null pointer"));
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 1, OUT, nullptr), "null pointer"));
    CHECK(!*why(4, 2, 0, nullptr, nullptr, nullptr, 0, 1, OUT, WS));            // n == 0: no cells, no cell pointers
    CHECK(std::strstr(why(4, 2, 0, nullptr, nullptr, nullptr, 0, 1, nullptr, WS), "null pointer"));
    CHECK(!*why(4, 2, 0, P, M, Z, 100, 0, OUT, nullptr, false));                // the pool's workspace: not the caller's to give
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 99, P, P), "more cells"));     // the bound before the overlaps
    CHECK(!*why(4, 2, 0, P, M, Z, 100, 100, OUT, WS));
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 0, mem + 199, WS), "records overlap an input"));       // the last value byte
    CHECK(!*why(4, 2, 0, P, M, Z, 100, 0, mem + 200, WS));
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 0, mem + 1024 - 255, WS), "records overlap an input"));  // its last byte on the mask's first
    CHECK(!*why(4, 2, 0, P, nullptr, Z, 100, 0, mem + 1024 - 255, WS));                                   // ... which is no input without a mask
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 0, mem + 2048 + 99, WS), "records overlap an input"));
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 0, OUT, mem + 2048 + 99), "workspace overlaps an input"));
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 0, OUT, reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(P) - workspace_bytes(4) + 1)), "workspace overlaps an input"));
    CHECK(!*why(4, 2, 0, P, M, Z, 100, 0, OUT, static_cast<const char*>(OUT) + 256));
    CHECK(std::strstr(why(4, 2, 0, P, M, Z, 100, 0, OUT, static_cast<const char*>(OUT) + 255), "records overlap the workspace"));

    // the broadcast
    auto bwhy = [&](int32_t nz, size_t cell, int zt, const void* z, const void* t, size_t n, const void* dst, const void* dm) {
        const ecv::Refusal r = broadcast_refusal(nz, cell, zt, z, t, n, dst, dm);
        bad = r.bad_type;
        return r.why ? r.why : "";
    };
    CHECK(!*bwhy(4, 2, 0, Z, P, 100, OUT, nullptr) && !*bwhy(4, 2, 0, Z, P, 100, OUT, WS));
    CHECK(std::strstr(bwhy(0, 0, 3, nullptr, nullptr, 100, nullptr, nullptr), "n_zones"));
    CHECK(std::strstr(bwhy(4, 0, 3, nullptr, nullptr, 100, nullptr, nullptr), "bad dtype") && bad);
    CHECK(std::strstr(bwhy(4, 2, 3, nullptr, nullptr, 100, nullptr, nullptr), "zone raster's type") && bad);
    CHECK(!*bwhy(4, 2, 0, nullptr, nullptr, 0, nullptr, nullptr));  // nothing to do
    CHECK(std::strstr(bwhy(4, 2, 0, nullptr, P, 100, OUT, nullptr), "null pointer") && std::strstr(bwhy(4, 2, 0, Z, nullptr, 100, OUT, nullptr), "null pointer") &&
          std::strstr(bwhy(4, 2, 0, Z, P, 100, nullptr, nullptr), "null pointer"));
    CHECK(std::strstr(bwhy(4, 1, 0, Z, P, (size_t(kMaxTiles) + 1) * kBlock * kBroadcastU * 16, OUT, nullptr), "tiles"));
    CHECK(std::strstr(bwhy(4, 2, 0, Z, P, 100, mem + 2048 + 99, nullptr), "dst overlaps"));
    CHECK(std::strstr(bwhy(4, 2, 0, Z, P, 100, mem + 7, nullptr), "dst overlaps"));  // the table: 4 cells of 2 bytes
    CHECK(!*bwhy(4, 2, 0, Z, P, 100, mem + 8, nullptr));
    CHECK(std::strstr(bwhy(4, 2, 0, Z, P, 100, OUT, mem + 2048), "dst_mask overlaps an input"));
    CHECK(std::strstr(bwhy(4, 2, 0, Z, P, 100, OUT, far + 199), "dst_mask overlaps dst") && !*bwhy(4, 2, 0, Z, P, 100, OUT, far + 200));
    CHECK(broadcast_cpl(1, 1) == 16 && broadcast_cpl(1, 4) == 4 && broadcast_cpl(8, 1) == 2 && broadcast_cpl(2, 2) == 8);
    CHECK(broadcast_tiles(0, 16) == 0 && broadcast_tiles(16 * kBlock * kBroadcastU, 16) == 1 && broadcast_tiles(16 * kBlock * kBroadcastU + 16, 16) == 2);

    // the table family: the same head and tail with its own cap and cap text, the kind's bound and text, the two alignments
    auto twhy = [&](int32_t nz, size_t cell, int kind, int zt, const void* p, const void* m, const void* z, size_t n, uint64_t max_cells, const void* out,
                    const void* ws, bool caller_ws = true) {
        const ecv::Refusal r = ezt::table_refusal(nz, cell, kind, zt, p, m, z, n, max_cells, out, ws, caller_ws);
        bad = r.bad_type;
        return r.why ? r.why : "";
    };
    static_assert(ezt::kMaxZones == 1 << 24, "the cap");
    CHECK(!*twhy(4, 2, 0, 0, P, M, Z, 100, 100, OUT, WS) && !bad);
    CHECK(!*twhy(257, 8, 1, 6, P, nullptr, Z, 100, 100, OUT, WS) && !*twhy(ezt::kMaxZones, 1, 0, 1, P, M, Z, 100, 100, OUT, far + (size_t(2) << 30)));
    CHECK(std::strstr(why(257, 2, 0, P, M, Z, 100, 0, OUT, WS), "EC_ZONAL_MAX_ZONES (256)"));  // the first family's cap and text stay its own
    CHECK(std::strstr(twhy(0, 0, 1, 3, nullptr, nullptr, nullptr, 100, 1, mem + 1, mem + 2), "EC_ZONAL_TABLE_MAX_ZONES (16777216)") && !bad);
    CHECK(std::strstr(twhy(ezt::kMaxZones + 1, 0, 1, 3, nullptr, nullptr, nullptr, 100, 1, nullptr, nullptr), "EC_ZONAL_TABLE_MAX_ZONES (16777216)") && !bad);
    CHECK(std::strstr(twhy(-5, 2, 0, 0, P, M, Z, 100, 100, OUT, WS), "n_zones"));
    CHECK(std::strstr(twhy(4, 0, 1, 3, nullptr, nullptr, nullptr, 100, 1, nullptr, nullptr), "bad dtype") && bad);
    CHECK(std::strstr(twhy(4, 2, 1, 3, nullptr, nullptr, nullptr, 100, 1, nullptr, nullptr), "zone raster's type") && bad);
    CHECK(std::strstr(twhy(4, 2, 1, 0, nullptr, M, Z, 100, 1, mem + 1, mem + 2), "null pointer") && !bad);
    CHECK(std::strstr(twhy(4, 2, 1, 0, P, M, nullptr, 100, 1, mem + 1, mem + 2), "null pointer"));
    CHECK(std::strstr(twhy(4, 2, 1, 0, P, M, Z, 100, 1, nullptr, mem + 2), "null pointer"));
    CHECK(std::strstr(twhy(4, 2, 1, 0, P, M, Z, 100, 1, mem + 1, nullptr), "null pointer"));
    CHECK(!*twhy(4, 2, 0, 0, nullptr, nullptr, nullptr, 0, 0, OUT, WS));  // n == 0: no cells, no cell pointers; a bound of 0 is a bound here
    CHECK(std::strstr(twhy(4, 2, 0, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, WS), "null pointer"));
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 99, mem + 1, mem + 2), "more cells than one exact record covers"));  // the bound before the alignments
    CHECK(std::strstr(twhy(4, 4, 1, 0, P, M, Z, 100, 99, mem + 1, mem + 2), "more than 2^32 cells"));
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 0, OUT, WS), "more cells"));  // no "0 = none" in this family
    CHECK(!*twhy(4, 2, 0, 0, P, M, Z, 100, 100, mem + 1, nullptr, false));         // the pool's forms: host records of any alignment, no workspace to give
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 99, mem + 1, nullptr, false), "more cells"));
    char* base = mem + (16 - reinterpret_cast<uintptr_t>(mem) % 16) % 16;  // 16-byte aligned, inside the values
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 100, base + 1, base + 2), "records are not 16-byte aligned"));  // the alignments before the overlaps
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 100, base, base + 2), "workspace is not 16-byte aligned"));
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 100, base, base), "records overlap an input"));
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 100, OUT, base), "workspace overlaps an input"));
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 100, OUT, base + 1024), "workspace overlaps an input"));  // the mask
    CHECK(!*twhy(4, 2, 0, 0, P, nullptr, Z, 100, 100, OUT, base + 1024));                                       // ... which is no input without one
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 100, base + 2048, WS), "records overlap an input"));      // the zone ids
    CHECK(!*twhy(4, 2, 0, 0, P, M, Z, 100, 100, OUT, static_cast<const char*>(OUT) + 256));                     // 4 records of 64 bytes
    CHECK(std::strstr(twhy(4, 2, 0, 0, P, M, Z, 100, 100, OUT, static_cast<const char*>(OUT) + 240), "records overlap the workspace"));
    CHECK(ezt::workspace_bytes(0, 4) == 192 && ezt::workspace_bytes(1, 4) == 320);
    CHECK(!*twhy(4, 2, 0, 0, P, M, Z, 100, 100, OUT, static_cast<const char*>(OUT) - 192));                     // kind 0: 4 entries of 6 words
    CHECK(std::strstr(twhy(4, 4, 1, 0, P, M, Z, 100, 100, OUT, static_cast<const char*>(OUT) - 192), "records overlap the workspace"));  // kind 1: 10 words
    CHECK(!*twhy(4, 4, 1, 0, P, M, Z, 100, 100, OUT, static_cast<const char*>(OUT) - 320));

    // the lookup: the broadcast's refusals under the table family's cap
    auto lwhy = [&](int32_t nz, size_t cell, int zt, const void* z, const void* t, size_t n, const void* dst, const void* dm) {
        const ecv::Refusal r = ezt::lookup_refusal(nz, cell, zt, z, t, n, dst, dm);
        bad = r.bad_type;
        return r.why ? r.why : "";
    };
    CHECK(!*lwhy(4, 2, 0, Z, P, 100, OUT, nullptr) && !*lwhy(257, 2, 0, Z, P, 100, OUT, WS) && !*lwhy(ezt::kMaxZones, 1, 6, Z, P, 100, OUT, WS));
    CHECK(std::strstr(bwhy(257, 2, 0, Z, P, 100, OUT, WS), "EC_ZONAL_MAX_ZONES (256)"));
    CHECK(std::strstr(lwhy(0, 0, 3, nullptr, nullptr, 100, nullptr, nullptr), "EC_ZONAL_TABLE_MAX_ZONES (16777216)") && !bad);
    CHECK(std::strstr(lwhy(ezt::kMaxZones + 1, 0, 3, nullptr, nullptr, 100, nullptr, nullptr), "EC_ZONAL_TABLE_MAX_ZONES (16777216)"));
    CHECK(std::strstr(lwhy(4, 0, 3, nullptr, nullptr, 100, nullptr, nullptr), "bad dtype") && bad);
    CHECK(std::strstr(lwhy(4, 2, 3, nullptr, nullptr, 100, nullptr, nullptr), "zone raster's type") && bad);
    CHECK(!*lwhy(4, 2, 0, nullptr, nullptr, 0, nullptr, nullptr) && !bad);  // nothing to do
    CHECK(std::strstr(lwhy(4, 2, 0, nullptr, P, 100, OUT, nullptr), "null pointer") && std::strstr(lwhy(4, 2, 0, Z, nullptr, 100, OUT, nullptr), "null pointer") &&
          std::strstr(lwhy(4, 2, 0, Z, P, 100, nullptr, nullptr), "null pointer"));
    CHECK(std::strstr(lwhy(4, 1, 0, Z, P, (size_t(kMaxTiles) + 1) * kBlock * kBroadcastU * 16, Z, Z), "tiles"));  // the tiles before the overlaps
    CHECK(std::strstr(lwhy(4, 2, 0, Z, P, 100, mem + 2048 + 99, mem + 2048), "dst overlaps"));
    CHECK(std::strstr(lwhy(4, 2, 0, Z, P, 100, mem + 7, nullptr), "dst overlaps"));  // the table: 4 cells of 2 bytes
    CHECK(!*lwhy(4, 2, 0, Z, P, 100, mem + 8, nullptr));
    CHECK(std::strstr(lwhy(300, 2, 0, Z, P, 100, mem + 599, nullptr), "dst overlaps") && !*lwhy(300, 2, 0, Z, P, 100, mem + 600, nullptr));  // 300 cells
    CHECK(std::strstr(lwhy(4, 2, 0, Z, P, 100, OUT, mem + 2048), "dst_mask overlaps an input"));
    CHECK(std::strstr(lwhy(4, 2, 0, Z, P, 100, OUT, far + 199), "dst_mask overlaps dst") && !*lwhy(4, 2, 0, Z, P, 100, OUT, far + 200));

    std::printf("%d checks passed\n", g_checks);
    return 0;
}
