// test_reduce_plan.cpp — reduce_plan() (csrc/ec_reduce_plan.hpp) against the three launchers' own arithmetic that it replaced.
//
// The FROZEN SPECIFICATION below is the host arithmetic of launch_min_max, first_diff_w and ec_mask_counts_device as they stood at
// commit 2293c0e, with the helpers they called (aligned16, aligned_to, reduce_head of ec_runtime.hpp, reduce_cap of ec_abi.hip), copied
// line for line; only the kernel launches are replaced by recording what they were given, and tuning() / device_cus() / cache_plan()
// are stand-ins that return the swept values.  It is not to be edited with the library.
//
// What this does NOT exercise: the glue in ec_abi.hip that feeds reduce_plan() — plan_reduction, residue(mask, 16 / sizeof(T)), the
// values of kScanShape, `direct = aligned && single` in launch_min_max.  The sweep below restates it; a slip there is for the GPU
// position tests (tests/test_gpu_reduction_positions.py) to catch.
//
// A stand-alone program: links nothing from the library; also built with -fsanitize=address,undefined (make test_reduce_plan_san).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "ec_reduce_plan.hpp"

// ------------------------------------------------------------------ stand-ins for the process state the parent's formulas read
namespace frozen {

struct Tuning {
    int reduce_bpc = 0;
    int unaligned_vector = 1;
};
static Tuning g_tuning;
static Tuning& tuning() { return g_tuning; }
static int g_cus = 256;
static int device_cus() { return g_cus; }
static unsigned g_policy = 0;
static unsigned cache_plan(const size_t*, int n) { return g_policy & ((1u << n) - 1u); }

constexpr int kReduceU = 8;
constexpr int kMaxReduceBlocks = 4096;
constexpr int kRBlock = 512;
constexpr int kBlock = 256;

// ---- ec_runtime.hpp at 2293c0e
inline bool aligned16(const void* a, const void* b, const void* c) {
    return tuning().unaligned_vector ||
           ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}
inline bool aligned_to(const void* a, size_t bytes) {
    return tuning().unaligned_vector || reinterpret_cast<uintptr_t>(a) % bytes == 0;
}
inline unsigned reduce_head(const void* p, size_t cell_size, size_t n) {
    if (!tuning().unaligned_vector) return 0;
    const size_t h = ((16 - reinterpret_cast<uintptr_t>(p) % 16) % 16) / cell_size;
    return h <= n ? static_cast<unsigned>(h) : 0u;
}
// ---- ec_abi.hip at 2293c0e
static int reduce_cap(int per_cu) {
    const int knob = tuning().reduce_bpc;
    const long cap = long(device_cus()) * (knob > 0 ? knob : per_cu);
    return static_cast<int>(cap < kMaxReduceBlocks ? cap : kMaxReduceBlocks);
}

struct Launch {
    bool launched = false;  // a partials kernel was launched
    bool al = false;
    unsigned grid = 0;      // what the finalize kernel is told
    bool has_hp = false;    // the kernel takes a head | policy word
    unsigned hp = 0;
    bool direct = false;    // the kernel was handed the result pointer
};

// launch_min_max<T> with sizeof(T) = SZ, launch shape (U, BLOCK, per_cu); `resident` = what resident_per_cu() answered
template <size_t SZ>
static Launch launch_min_max(const void* p, const uint8_t* mask, size_t n, int U, int BLOCK, int resident) {
    Launch out;
    unsigned grid = 0;
    if (n > 0) {
        const bool al = aligned16(p, p, p) && (!mask || aligned_to(mask, 16 / SZ));
        const int cap = reduce_cap(8);  // the cell-wise kernel: 256-thread workgroups
        out.launched = true;
        out.al = al;
        if (al) {
            const unsigned head = reduce_head(p, SZ, n);
            const size_t groups = (n - head) / (16 / SZ);
            const int cap2 = reduce_cap(resident);
            size_t tiles = (groups + size_t(BLOCK) * U - 1) / (size_t(BLOCK) * U);
            if (tiles < 1) tiles = 1;
            grid = static_cast<unsigned>(tiles < size_t(cap2) ? tiles : size_t(cap2));
            const bool direct = grid == 1;  // one workgroup: it writes the result itself
            const size_t stream_bytes[2] = {n * SZ, mask ? n : 0};
            const unsigned hp = head | (cache_plan(stream_bytes, 2) << 8);  // leading cells + load policy
            out.has_hp = true;
            out.hp = hp;
            out.direct = direct;
        } else {
            size_t blocks = (n + kBlock - 1) / kBlock;
            grid = static_cast<unsigned>(blocks < size_t(cap) ? blocks : size_t(cap));
        }
    }
    out.grid = grid;
    return out;
}

// first_diff_w<W> with sizeof(W) = SZ (ec_first_difference returns before it for n == 0)
template <size_t SZ>
static Launch first_diff_w(const void* l, const void* r, size_t n) {
    Launch out;
    const int cap = reduce_cap(4);
    const bool al = aligned16(l, r, r);
    const unsigned head = al ? reduce_head(l, SZ, n) : 0u;
    size_t tiles = al ? ((n - head) / (16 / SZ) + size_t(kRBlock) * kReduceU - 1) / (size_t(kRBlock) * kReduceU) : (n + kRBlock - 1) / kRBlock;
    if (tiles < 1) tiles = 1;
    const unsigned grid = static_cast<unsigned>(tiles < size_t(cap) ? tiles : size_t(cap));
    const size_t stream_bytes[2] = {n * SZ, n * SZ};
    out.launched = true;
    out.al = al;
    out.has_hp = true;
    out.hp = head | (cache_plan(stream_bytes, 2) << 8);
    out.grid = grid;
    return out;
}

static Launch mask_counts_device(const uint8_t* m, size_t n) {
    Launch out;
    unsigned grid = 0;
    if (n > 0) {
        const int cap = reduce_cap(4);
        const bool al = aligned_to(m, 16);
        const unsigned head = al ? reduce_head(m, 1, n) : 0u;
        size_t tiles = al ? ((n - head) / 16 + size_t(kRBlock) * kReduceU - 1) / (size_t(kRBlock) * kReduceU) : (n + kRBlock - 1) / kRBlock;
        if (tiles < 1) tiles = 1;
        grid = static_cast<unsigned>(tiles < size_t(cap) ? tiles : size_t(cap));
        const bool direct = grid == 1;  // one workgroup: it writes the result itself
        const size_t stream_bytes[1] = {n};
        out.launched = true;
        out.al = al;
        out.has_hp = true;
        out.hp = head | (cache_plan(stream_bytes, 1) << 8);
        out.direct = direct;
    }
    out.grid = grid;
    return out;
}

}  // namespace frozen

// ------------------------------------------------------------------ the sweep
static long g_checked = 0, g_failed = 0;

static unsigned residue(const void* p, size_t mod) { return static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) % mod); }

// `direct_needs_aligned`: k_min_max_partials_cellwise has no result pointer, so launch_min_max hands it out only with the vector kernel
static void compare(const char* what, const frozen::Launch& want, const ecd::ReducePlan& got, bool has_direct, bool direct_needs_aligned,
                    unsigned off0, unsigned off1, size_t cell, size_t n, int shape, int per_cu) {
    ++g_checked;
    bool ok = got.grid == want.grid;
    if (want.launched) {
        const unsigned head = want.has_hp ? (want.hp & 0xffu) : 0u;
        ok = ok && got.aligned == want.al && got.head == head;
        if (want.has_hp) ok = ok && got.head_policy == want.hp;
        if (has_direct) ok = ok && (direct_needs_aligned ? got.aligned && got.single : got.single) == want.direct;
    }
    if (!ok && ++g_failed <= 20)
        std::printf("MISMATCH %s off0=%u off1=%u cell=%zu n=%zu shape=%d per_cu=%d bpc=%d cus=%d uv=%d policy=%u: want {al %d grid %u hp %#x direct %d} "
                    "got {al %d head %u grid %u hp %#x single %d}\n",
                    what, off0, off1, cell, n, shape, per_cu, frozen::g_tuning.reduce_bpc, frozen::g_cus, frozen::g_tuning.unaligned_vector,
                    frozen::g_policy, int(want.al), want.grid, want.hp, int(want.direct), int(got.aligned), got.head, got.grid, got.head_policy,
                    int(got.single));
}

struct Shape { int u, block, per_cu; };
static const Shape kShapes[5] = {{8, 512, 4}, {16, 512, 4}, {8, 256, 8}, {8, 1024, 2}, {4, 512, 4}};  // reduce_shape 0..4 (launch_min_max)

template <size_t SZ>
static void sweep_cell_size(std::mt19937_64& rng) {
    alignas(64) static unsigned char cells[128], other[128];  // addresses only: nothing is read through them
    const size_t cpl = 16 / SZ;
    for (int shape = 0; shape < 5; ++shape)
        for (int bpc : {0, 1, 100})
            for (int cus : {1, 8, 256})
                for (int uv : {0, 1})
                    for (unsigned off0 = 0; off0 < 32; ++off0) {
                        frozen::g_tuning.reduce_bpc = bpc;
                        frozen::g_tuning.unaligned_vector = uv;
                        frozen::g_cus = cus;
                        const Shape sh = kShapes[shape];
                        const size_t tile = size_t(sh.block) * sh.u * cpl;
                        const size_t cap = size_t(frozen::reduce_cap(sh.per_cu));
                        const size_t cw_cap = size_t(frozen::reduce_cap(8)) * frozen::kBlock;
                        const size_t head = ((16 - off0 % 16) % 16) / SZ;
                        size_t ns[] = {0, 1, 2, 3, cpl - 1, cpl, cpl + 1, head > 0 ? head - 1 : 0, head, head + 1, head + cpl, 255, 256, 257, 511, 512, 513,
                                       tile - 1, tile, tile + 1, tile + head, 2 * tile + tile / 2 + 3, cap * tile - 1, cap * tile, cap * tile + 1,
                                       cap * tile + head + cpl, (cap + 3) * tile + 5, cw_cap - 1, cw_cap, cw_cap + 1, cw_cap + 3 * frozen::kBlock,
                                       size_t(rng() % ((cap + 4) * tile)), size_t(rng() % ((cap + 4) * tile)), size_t(rng() % (2 * tile)),
                                       size_t(rng() % (cw_cap + 1024)), size_t(rng() % 64)};
                        for (size_t n : ns) {
                            const unsigned off1 = unsigned(rng() % 32);
                            frozen::g_policy = unsigned(rng() % 4);  // every combination of the two streams' bits comes up for every shape
                            const int resident = 1 + int(rng() % sh.per_cu);  // resident_per_cu() answers 1 .. per_cu
                            const void* p = cells + off0;
                            const uint8_t* q = other + off1;
                            // ---- min/max, plain and masked, every launch shape
                            for (const uint8_t* mask : {static_cast<const uint8_t*>(nullptr), q}) {
                                const unsigned pol = frozen::g_policy & 3u;
                                const ecd::ReduceShape rs = {sh.block, sh.u, resident, frozen::kBlock, 8};
                                const ecd::ReducePlan pl = ecd::reduce_plan(residue(p, 16), mask ? residue(mask, cpl) : 0u, SZ, n, rs, cus, bpc, uv != 0, pol);
                                compare(mask ? "min_max(masked)" : "min_max", frozen::launch_min_max<SZ>(p, mask, n, sh.u, sh.block, resident), pl, true, true,
                                        off0, off1, SZ, n, shape, resident);
                            }
                            if (shape != 0) continue;  // first difference and the counts run the default shape only
                            const ecd::ReduceShape rs = {frozen::kRBlock, frozen::kReduceU, 4, frozen::kRBlock, 4};
                            if (n > 0) {
                                const ecd::ReducePlan pl = ecd::reduce_plan(residue(p, 16), residue(q, 16), SZ, n, rs, cus, bpc, uv != 0, frozen::g_policy & 3u);
                                compare("first_diff", frozen::first_diff_w<SZ>(p, q, n), pl, false, false, off0, off1, SZ, n, shape, 4);
                            }
                            if (SZ == 1) {
                                const ecd::ReducePlan pl = ecd::reduce_plan(residue(p, 16), 0u, 1, n, rs, cus, bpc, uv != 0, frozen::g_policy & 1u);
                                compare("mask_counts", frozen::mask_counts_device(static_cast<const uint8_t*>(p), n), pl, true, false, off0, off1, SZ, n,
                                        shape, 4);
                            }
                        }
                    }
}

int main() {
    std::mt19937_64 rng(0x5EED2293ull);
    sweep_cell_size<1>(rng);
    sweep_cell_size<2>(rng);
    sweep_cell_size<4>(rng);
    sweep_cell_size<8>(rng);
    std::printf("%ld plans compared, %ld differ\n", g_checked, g_failed);
    if (g_failed || g_checked < 100000) return 1;
    std::printf("all checks passed\n");
    return 0;
}
