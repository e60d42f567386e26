// Arithmetic of the transported interpolation of tangent-vector features between two clouds (interp_transport.hip), shared with
// the g++ host-check build (tests/hostcheck_vector_interp) like interp_math.h / connection_math.h.  No HIP types, no LDS, no wave
// intrinsics.
//
// What is being restated: deltaconv/geometry/connection.py:6-47 (build_transport) composed with torch_geometric.nn.knn_interpolate
// -- every neighbour's vector is carried into the frame of the target point (dcconn::transport) and then weighted as
// knn_interpolate weights it (dcinterp::coef).  Vector fields as in ell_math.h: rows 2i, 2i+1 hold the two coefficients at point i.
// Only the VALUES are differentiated (bwd4 below); frames, normals and positions are constants.
//
// Every rule is fixed so that a numpy restatement (tests/vector_interp_restate.py) reproduces the bits:
//   table     slot e = q * k + s of query row q (pair b, nr = rptr[b+1] - rptr[b]) holds M = c * R, four fp32 products:
//             c = dcinterp::coef (w_s / den in the forward's den bits; exactly 1.0f for the only valid slot of a query, which keeps
//             R's bits), R = dcconn::transport(target frame of q, source frame of rptr[b] + idx[e]).  A row in no pair and a slot
//             with idx outside [0, nr) hold four +0.0f.  Frames are indexed by the ABSOLUTE rows qptr / rptr name.
//   forward   au = av = 0; slots s = 0 .. k-1 in order, invalid ones skipped (validity comes from idx, never from M):
//             au = (au + M00*v0) + M01*v1, av = (av + M10*v0) + M11*v1 with v0 / v1 rows 2j, 2j+1 of the source values,
//             j = rptr[b] + idx: the slot and operation order of dcconn::transport_sum_fwd.  No valid slot: zeros.
//   backward  of source row r: its in-edges (the lists of dc_knn_cross_transpose, unchanged) in ascending edge id,
//             du = (du + M00*g0) + M10*g1, dw = (dw + M01*g0) + M11*g1 with g0 / g1 rows 2 (e/k - edge_base) and the next; an edge
//             whose row falls outside the call's g (or whose entry falls outside the call's table) is skipped.
// Every product and sum is one fp32 rounding (dcinterp::mul_rn / add_rn), no contraction.
#pragma once
#include <stdint.h>

#include "connection_math.h"
#include "interp_math.h"

namespace dcvinterp {
using dcconn::R4;
using dcinterp::add_rn;
using dcinterp::load4;
using dcinterp::mul_rn;

DC_HD R4 zero_entry() { return R4{0.f, 0.f, 0.f, 0.f}; }

// Slot s of query row q (absolute) whose pair starts at reference row rbase and holds nr reference rows.
DC_HD R4 entry_in_pair(long long q, int s, long long rbase, long long nr, int k, const int* idx, const float* d2, const float* tn,
                       const float* tx, const float* ty, const float* sn, const float* sx, int non_oriented) {
    const long long j = idx[q * k + s];
    if (!dcinterp::valid_slot(j, nr)) return zero_entry();
    const float c = dcinterp::coef(nr, k, idx + q * k, d2 + q * k, s);
    const long long r = rbase + j;
    const R4 R = dcconn::transport(dcconn::ld3(tn + 3 * q), dcconn::ld3(tx + 3 * q), dcconn::ld3(ty + 3 * q), dcconn::ld3(sn + 3 * r),
                                   dcconn::ld3(sx + 3 * r), non_oriented);
    return R4{mul_rn(c, R.r00), mul_rn(c, R.r01), mul_rn(c, R.r10), mul_rn(c, R.r11)};
}

// The table entry of slot e = q * k + s of the call: four +0.0f for a row outside every pair and for an invalid slot.  HOST-SIDE
// wrapper (tests/hostcheck_vector_interp): it finds the pair by bisection.  The kernel takes its pair from the grid and calls
// entry_in_pair itself (with nr cut to int32's range, which no idx can exceed), and never visits a row outside every pair.
DC_HD R4 entry(const int64_t* qptr, const int64_t* rptr, int B, int k, const int* idx, const float* d2, const float* tn,
               const float* tx, const float* ty, const float* sn, const float* sx, int non_oriented, long long e) {
    const long long q = e / k;
    const int b = dcinterp::pair_of(qptr, B, q);
    if (b < 0) return zero_entry();
    return entry_in_pair(q, (int)(e - q * k), rptr[b], rptr[b + 1] - rptr[b], k, idx, d2, tn, tx, ty, sn, sx, non_oriented);
}

// Channels c0 .. c0+nc-1 (nc in 1 .. 4) of one query: v [2 Nr, ldv] the rows of ITS reference cloud, idx [k] / M [k] its slots.
// vec: v + c0 is 16-byte aligned in every row and nc = 4.  ou / ov [4] receive nc values each (rows 2q, 2q+1 of the output).
DC_HD void fwd4(const float* v, long long ldv, long long nr, int k, const int* idx, const R4* M, int c0, int nc, bool vec, float* ou,
                float* ov) {
    float au[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < k; ++s) {
        const long long j = idx[s];
        if (!dcinterp::valid_slot(j, nr)) continue;
        const R4 m = M[s];                    // one 16-byte load, the same address on every channel group of the query
        float v0[4], v1[4];
        load4(v + (2 * j) * ldv + c0, nc, vec, v0);
        load4(v + (2 * j + 1) * ldv + c0, nc, vec, v1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            au[c] = add_rn(add_rn(au[c], mul_rn(m.r00, v0[c])), mul_rn(m.r01, v1[c]));
            av[c] = add_rn(add_rn(av[c], mul_rn(m.r10, v0[c])), mul_rn(m.r11, v1[c]));
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ou[c] = au[c];
        ov[c] = av[c];
    }
}

// Channels c0 .. c0+nc-1 of one source row's gradient: its in-edges tedge [n] in ascending order, g [2 rows, ldg] the gradient of
// the call's query rows, query row of edge e = e / k - edge_base, table entry e - edge_base * k of tmat [tmat_rows] (a slice of a
// store-wide table starts at the call's first query row).  An edge whose row falls outside [0, rows) or whose entry falls outside
// the table is skipped.  vec: g + c0 is 16-byte aligned in every row and nc = 4.  du / dw [4] receive nc values each.
DC_HD void bwd4(const float* g, long long ldg, long long rows, int k, long long edge_base, const int64_t* tedge, const R4* tmat,
                long long tmat_rows, long long n, int c0, int nc, bool vec, float* du, float* dw) {
    float au[4] = {0.f, 0.f, 0.f, 0.f}, aw[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;                      // in-edges whose loads fly together; the sum itself stays in list order
    for (long long t0 = 0; rows > 0 && tmat_rows > 0 && t0 < n; t0 += U) {
        R4 m[U];
        float g0[U][4], g1[U][4];
        bool in[U];
        const float* gr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long t = t0 + u < n ? t0 + u : n - 1;             // (clamped: an unconditional load, masked below)
            const long long e = tedge[t];
            const long long row = (e >> 32 ? e / k : (long long)((unsigned)e / (unsigned)k)) - edge_base;
            const long long at = e - edge_base * k;
            in[u] = t0 + u < n && row >= 0 && row < rows && at >= 0 && at < tmat_rows;
            m[u] = tmat[in[u] ? at : 0];
            gr[u] = g + (in[u] ? 2 * row : 0) * ldg + c0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load4(gr[u], nc, vec, g0[u]);
            load4(gr[u] + ldg, nc, vec, g1[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                au[ch] = in[u] ? add_rn(add_rn(au[ch], mul_rn(m[u].r00, g0[u][ch])), mul_rn(m[u].r10, g1[u][ch])) : au[ch];
                aw[ch] = in[u] ? add_rn(add_rn(aw[ch], mul_rn(m[u].r01, g0[u][ch])), mul_rn(m[u].r11, g1[u][ch])) : aw[ch];
            }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        du[ch] = au[ch];
        dw[ch] = aw[ch];
    }
}

}  // namespace dcvinterp
