// Arithmetic of voxel-grid subsampling (voxel.hip behind dc_voxel_subsample), shared with the g++ host-check build
// (tests/hostcheck_voxel) like knn_grid_math.h.  No HIP types, no LDS, no wave intrinsics, no atomics.
//
// One representative per occupied cell of edge `size`: what torch_cluster.grid_cluster / torch_geometric.nn.voxel_grid followed by
// consecutive_cluster compute, with every rule fixed so that a numpy restatement (tests/voxel_restate.py) reproduces the bits:
//   finite    a point takes part iff its three coordinates are finite (dcgrid::finite3); the others belong to no cell, are never
//             picked and get cluster -1
//   origin    o_b of cloud b: the fp32 per-axis minimum over the cloud's OWN finite points (not over the batch: a cloud's result
//             does not depend on its batch-mates), or the caller's origin
//   cell      per axis t = floorf(fl(fl(p - o) / s)), s the axis' fp32 edge length: the subtraction and the DIVISION each rounded
//             to fp32 once (no product with a reciprocal, which rounds differently on a cell face)
//   range     a finite point whose t is not strictly inside (-2^20, 2^20) on some axis marks its cloud as overflowing (the call
//             raises); within range the three cells, biased by 2^20, pack into 63 bits -- the all-ones word is no cell
//   key       the representative of a cell is the member with the smallest 64-bit key (bits(d2) << 32) | local index
//               pick = centre: d2 = (dx*dx + dy*dy) + dz*dz (dcgrid::dist2, no contraction) to the cell centre
//                              fl(fl(fl((float)t + 0.5f) * s) + o); d2 is non-negative, so its bit pattern orders as an unsigned
//                              integer, +inf sorts last, and it cannot be NaN for finite inputs; ties go to the lower index
//               pick = first:  d2 bits are 0: the member with the lowest index
//   order     the representatives of a cloud in ascending row order (`rows` is a stable subset of the rows);
//             cluster[i] = optr[b] + rank of i's cell among the cloud's representatives, so rows[cluster[i]] is i's representative
// A minimum over integer keys does not depend on the order of its operands: neither the hash layout nor the launch shape nor the
// grouping of clouds can reach the result.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "knn_grid_math.h"

namespace dcvox {

constexpr int AXIS_BITS = 21;
constexpr float AXIS_LIMIT = 1048576.0f;      // 2^20: |t| must stay below it
constexpr int AXIS_BIAS = 1 << 20;
constexpr uint64_t EMPTY = ~(uint64_t)0;      // no cell (a packed cell has bit 63 clear), and no representative yet
enum { PICK_CENTRE = 0, PICK_FIRST = 1 };

// the four fp32 operations of the rules, each rounded once
#if defined(__HIP_DEVICE_COMPILE__)
DC_HD float sub_rn(float a, float b) { return __fsub_rn(a, b); }
DC_HD float div_rn(float a, float b) { return __fdiv_rn(a, b); }
DC_HD float mul_rn(float a, float b) { return __fmul_rn(a, b); }
DC_HD float add_rn(float a, float b) { return __fadd_rn(a, b); }
#else
DC_HD float sub_rn(float a, float b) { const float r = a - b; return r; }
DC_HD float div_rn(float a, float b) { const float r = a / b; return r; }
DC_HD float mul_rn(float a, float b) { const float r = a * b; return r; }
DC_HD float add_rn(float a, float b) { const float r = a + b; return r; }
#endif

DC_HD float cell_axis(float p, float o, float s) { return floorf(div_rn(sub_rn(p, o), s)); }
DC_HD bool in_range(float t) { return fabsf(t) < AXIS_LIMIT; }                    // false for NaN and +-inf as well
DC_HD float centre_axis(float t, float o, float s) { return add_rn(mul_rn(add_rn(t, 0.5f), s), o); }

DC_HD uint64_t pack(float tx, float ty, float tz) {                               // in-range cells only
    const uint64_t x = (uint64_t)((int)tx + AXIS_BIAS), y = (uint64_t)((int)ty + AXIS_BIAS), z = (uint64_t)((int)tz + AXIS_BIAS);
    return (z << (2 * AXIS_BITS)) | (y << AXIS_BITS) | x;
}

DC_HD uint32_t float_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
DC_HD uint64_t rep_key(float d2, uint32_t local) { return ((uint64_t)float_bits(d2) << 32) | (uint64_t)local; }

// A point of a cloud: does it take part, its packed cell, the key it bids for the cell with.
struct Bid {
    bool finite, overflow;                    // overflow: finite, but outside the packable range (cell and key are then unset)
    uint64_t cell, key;
};
DC_HD Bid bid(float x, float y, float z, const float* o, const float* s, int pick, uint32_t local) {
    Bid r;
    r.finite = dcgrid::finite3(x, y, z);
    r.overflow = false;
    r.cell = r.key = EMPTY;
    if (!r.finite) return r;
    const float tx = cell_axis(x, o[0], s[0]), ty = cell_axis(y, o[1], s[1]), tz = cell_axis(z, o[2], s[2]);
    if (!(in_range(tx) && in_range(ty) && in_range(tz))) {
        r.overflow = true;
        return r;
    }
    r.cell = pack(tx, ty, tz);
    float d2 = 0.f;
    if (pick == PICK_CENTRE)
        d2 = dcgrid::dist2(x, y, z, centre_axis(tx, o[0], s[0]), centre_axis(ty, o[1], s[1]), centre_axis(tz, o[2], s[2]));
    r.key = rep_key(d2, local);
    return r;
}

}  // namespace dcvox
