// ec_launch_split.hpp — how many workgroups one launch may hold, and how a job of more tiles is cut into launches.
// Self-contained (no HIP, no library header), like ec_reduce_plan.hpp: host/test_launch_split.cpp checks it on the CPU.
//
// A dispatch packet carries its grid in WORK-ITEMS as a 32-bit field, so one launch of kLanes-lane workgroups holds at most
// (2^32 - 1) / kLanes of them.  The runtime does not refuse a larger grid: hipLaunchKernel returns hipSuccess and the device runs
// grid * kLanes mod 2^32 work-items — a launch of 2^24 + 1 workgroups of 256 ran ONE workgroup and left every other tile unwritten
// (measured on gfx950 under ROCm 7.2, DESIGN.md "Launches past 2^24 workgroups").  Nothing in the library may therefore hand
// more than kMaxGroups workgroups to one launch:
//   * the one-workgroup-per-tile families whose documented limit is 2^31 - 1 tiles (focal, focal_rank, composite, composite_rank,
//     reclass, zonal broadcast, resample) issue several launches on the same stream, launch k covering the tiles
//     [first, first + count) of part(tiles, k); the kernels take `first` as an argument (two_front_tile(first), ec_tile.hpp);
//   * the streaming families (binops, maps, one-pass trees) refuse such a call on the host (check_groups, ec_runtime.hpp): they
//     reach the limit only at 64 GiB or more of one stream.
#pragma once

#include <stdint.h>

namespace ecs {

constexpr uint64_t kLanes = 256;                             // kBlock: every tiled kernel of the library launches workgroups of 256 lanes
constexpr uint64_t kMaxGroups = 0xFFFFFFFFull / kLanes;      // 16 777 215 = 2^24 - 1

struct Part {
    uint64_t first, count;  // the tiles [first, first + count) of one launch; 1 <= count <= cap
};

// launches a job of `tiles` tiles takes; 0 for no tiles
constexpr uint64_t launches(uint64_t tiles, uint64_t cap = kMaxGroups) { return tiles / cap + (tiles % cap != 0 ? 1 : 0); }

// launch k (k < launches(tiles, cap)) of the job: every launch but the last is full
constexpr Part part(uint64_t tiles, uint64_t k, uint64_t cap = kMaxGroups) {
    return Part{k * cap, tiles - k * cap < cap ? tiles - k * cap : cap};
}

static_assert(kMaxGroups * kLanes <= 0xFFFFFFFFull && (kMaxGroups + 1) * kLanes > 0xFFFFFFFFull, "the largest grid whose work-items fit 32 bits");
static_assert(launches(0) == 0 && launches(1) == 1 && launches(kMaxGroups) == 1 && launches(kMaxGroups + 1) == 2, "launch count");
static_assert(launches(0x7fffffffull) == 129, "the documented 2^31 - 1 tiles take 129 launches");
static_assert(part(kMaxGroups + 2, 1).first == kMaxGroups && part(kMaxGroups + 2, 1).count == 2, "the last launch takes the rest");

}  // namespace ecs
