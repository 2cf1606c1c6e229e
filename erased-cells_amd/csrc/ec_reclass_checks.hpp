// ec_reclass_checks.hpp — the refusals of the reclassification (include/erased_cells.h: ec_reclass_table_build, ec_reclass) and
// their order, in plain C++ over ec_reclass_plan.hpp (the thresholds, the record, the tiles) and ec_refusal.hpp (the refusal value,
// the table of overlaps).  The builder is here because it refuses or writes the whole record, never a part.
//
// Self-contained like ec_reclass_plan.hpp: no HIP include; host/test_reclass_plan.cpp runs these very functions under the address
// and undefined-behaviour sanitizers.
#pragma once

#include "ec_reclass_plan.hpp"
#include "ec_refusal.hpp"

namespace ecr {

// ec_reclass_table_build: why it refuses, or nothing with *out written — every byte of it.  The order is the header's.  A refusal
// writes nothing to *out.
inline ecv::Refusal build(int t, int bt, const void* breaks, int32_t n_breaks, int32_t right, int dt, const ec_value* values, const uint8_t* valid,
                          const ec_value* nodata, ec_reclass_table* out) {
    if (n_breaks < 1 || n_breaks > kMaxBreaks) return {"n_breaks is not within 1 .. EC_RECLASS_MAX_BREAKS (255)"};
    if (right != 0 && right != 1) return {"right is not 0 or 1"};
    if (!ecl::valid(t) || !ecl::valid(bt) || !ecl::valid(dt)) return {"bad dtype", true};
    if (!breaks || !values || !out) return {"null pointer"};
    for (int32_t c = 0; c <= n_breaks; ++c)
        if (values[c].dtype != dt) return {"a class value is not of the output's dtype"};
    if (nodata && nodata->dtype != dt) return {"the nodata value is not of the output's dtype"};
    ec_reclass_table tab;
    memset(&tab, 0, sizeof tab);
    const char* why = with_pair(t, bt, [&](auto tt, auto bb) -> const char* {
        using T = decltype(tt);
        using BT = decltype(bb);
        BT b[kMaxBreaks];
        memcpy(b, breaks, size_t(n_breaks) * sizeof(BT));
        if (const char* w = breaks_refusal<T, BT>(b, n_breaks)) return w;
        tab.n_reached = thresholds<T, BT>(b, n_breaks, right != 0, tab.thr);
        return nullptr;
    });
    if (why) return {why};
    tab.t = t;
    tab.dt = dt;
    tab.n_breaks = n_breaks;
    const size_t w = ecl::size_of(dt);
    for (int32_t c = 0; c <= n_breaks; ++c) tab.value_bits[c] = low_bytes(values[c], w);
    bool drops = false;
    for (int32_t c = 0; c < kSlots; ++c) {
        tab.valid[c] = c <= n_breaks ? (valid ? valid[c] != 0 : 1) : 0;
        drops = drops || (c <= n_breaks && !tab.valid[c]);
    }
    tab.flags = (nodata ? uint32_t(EC_RECLASS_HAS_NODATA) : 0u) | (drops ? uint32_t(EC_RECLASS_DROPS) : 0u);
    tab.nodata_bits = nodata ? low_bytes(*nodata, w) : 0;
    memcpy(out, &tab, sizeof tab);
    return {};
}

// Why ec_reclass refuses a call, or nothing; the header's order.  cell_size / out_size: bytes of a cell of t / dt, 0 for a bad code.
// n == 0 passes whatever the pointers are.
inline ecv::Refusal reclass_refusal(size_t cell_size, size_t out_size, const void* src, const void* mask, size_t n, const void* table, const void* dst,
                                    const void* dst_mask) {
    if (cell_size == 0 || out_size == 0) return {"bad dtype", true};
    if (n == 0) return {};
    if (!src || !table || !dst) return {"null pointer"};
    if (ecv::misaligned(table, 16)) return {"table_dev is not 16-byte aligned"};
    if (tiles(n, cpl(cell_size, out_size)) > kMaxTiles) return {"more than 2^31 - 1 tiles"};
    const ecv::Span out{dst, n * out_size}, out_mask{dst_mask, n}, cells{src, n * cell_size}, valid{mask, n}, tab{table, size_t(EC_RECLASS_TABLE_BYTES)};
    const ecv::OverlapRow rows[] = {{out, cells, "dst overlaps an input (the operation is not in-place)"}, {out_mask, cells, "dst_mask overlaps an input"},
                                    {out, valid, "dst overlaps an input (the operation is not in-place)"}, {out_mask, valid, "dst_mask overlaps an input"},
                                    {out, tab, "dst overlaps an input (the operation is not in-place)"},   {out_mask, tab, "dst_mask overlaps an input"},
                                    {out, out_mask, "dst_mask overlaps dst"}};
    return {ecv::first_overlap(rows)};
}

}  // namespace ecr
