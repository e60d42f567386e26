// The maximum of a 64-bit key over the 64 lanes of a wave, for the farthest-point samplers (fps_euclid.hip, fps_grid.hip): four
// DPP steps and four lane reads, against six __shfl_xor steps, which compile to ds_bpermute pairs.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;

// max(v, v of the lane the DPP control names), all 64 lanes active.  CTRL: 0xB1 quad_perm [1,0,3,2] (lane ^ 1), 0x4E quad_perm
// [2,3,0,1] (lane ^ 2), 0x141 row_half_mirror (7 - lane inside 8 lanes), 0x140 row_mirror (15 - lane inside a row of 16).
template <int CTRL>
__device__ __forceinline__ u64 dpp_max(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, false);
    const u64 o = ((u64)hi << 32) | lo;
    return o > v ? o : v;
}
template <int LANE>
__device__ __forceinline__ u64 read_lane(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, LANE);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), LANE);
    return ((u64)hi << 32) | lo;
}
// the wave's maximum, the same in every lane: four DPP steps make every row of 16 lanes uniform (pairs, quads, halves, the row),
// then the four rows meet in scalar registers
__device__ __forceinline__ u64 wave_max(u64 v) {
    v = dpp_max<0xB1>(v);
    v = dpp_max<0x4E>(v);
    v = dpp_max<0x141>(v);
    v = dpp_max<0x140>(v);
    const u64 a = read_lane<0>(v), b = read_lane<16>(v), c = read_lane<32>(v), d = read_lane<48>(v);
    const u64 ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

}  // namespace
