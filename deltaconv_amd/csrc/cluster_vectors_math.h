// Arithmetic of the pooling of tangent-vector features over the cells of a cluster vector (cluster_vectors.hip), shared with the
// g++ host-check build (tests/hostcheck_cluster_vectors) like cluster_math.h / pool_vectors_math.h.  No HIP types, no LDS, no wave
// intrinsics.
//
// What is being restated: cluster_math.h (torch_scatter.scatter over a cluster vector) for the VECTOR stream.  Vector fields as in
// ell_math.h: rows 2i, 2i+1 hold the two coefficients at point i in ITS frame, so before the members of a cell can be reduced
// each is carried into the cell's frame by parallel transport (deltaconv/geometry/connection.py:6-47, dcconn::transport), as
// pool_vectors_math.h does over a search.  Every point belongs to ONE cell, so the transport table is one 2 x 2 matrix per POINT
// (16 N bytes), not per slot.  The way down is a walk over the member lists and its backward a gather; the way up is a gather and
// its backward a walk.  Only the VALUES are differentiated.
//
// Every rule is fixed so that a numpy restatement (tests/cluster_vectors_restate.py) reproduces the bits:
//   cell      row i belongs to cell cl = cluster[i] iff 0 <= cl < M (dccl::in_cell)
//   rdown     entry i = dcconn::transport(target: the frame (n, x, y) of cell cl; source: the frame (n, x) of point i; non_oriented),
//             four +0.0f for a point without a cell
//   rup       entry i = dcconn::transport(target: the frame (n, x, y) of point i; source: the frame (n, x) of cell cl; non_oriented),
//             with the same zeros.  BUILT, not taken as the transpose of rdown: nothing here rests on R^T equalling the reverse
//             transport in fp32
//   mode      0 max, 2 sum, 3 mean (dcvpool::mode_ok; 1, min, has no vector analogue and is refused)
//   lists     the members of a cell in ASCENDING row order (dc_cluster_lists); a member outside [0, N) is skipped and not counted
//   sum       au = av = +0; per member i, R = rdown[i], v0 / v1 rows 2i, 2i+1: au = (au + R00*v0) + R01*v1,
//             av = (av + R10*v0) + R11*v1: the order of dcvpool::fwd4
//   mean      the sum, then ONE division per component by (float)cnt, cnt the members taken
//   max       per channel.  The key of a member is v0*v0 + v1*v1, two products and one sum, in the SOURCE frame.  The first member
//             is taken; a later one replaces it iff its key is strictly larger: ties keep the LOWER row; a later NaN key compares
//             false and is never taken, a first NaN stays.  The output is the winner's transported vector (R00*v0 + R01*v1,
//             R10*v0 + R11*v1): two products and one sum each, no zero start.  arg = the winner's ROW i, int32, per channel
//   empty     a cell without a member gets zeros, arg = -1
// The backward of the pooling is a gather, one term per point: cl = cluster[i], R = rdown[i], g0 / g1 rows 2cl, 2cl+1 of g:
//   du = R00*g0 + R10*g1, dw = R01*g0 + R11*g1, two products and one sum each -- always (sum); with g0, g1 each first divided by
//   (float)(cptr[cl+1] - cptr[cl]), every quotient rounded on its own (mean); where arg[cl,ch] == i, else +0.0f (max).  A point
//   without a cell gets zeros.
// The un-pooling: out[2i] = R00*x0 + R01*x1, out[2i+1] = R10*x0 + R11*x1 with R = rup[i] and x0 / x1 rows 2cl, 2cl+1; zeros for a
//   point without a cell.  It is the same gather with the matrix as it stands and no mode.
// Its backward: per cell the members in ascending order from du = dw = +0, R = rup[i], g0 / g1 rows 2i, 2i+1 of g:
//   du = (du + R00*g0) + R10*g1, dw = (dw + R01*g0) + R11*g1: the sum-mode walk through the transposed matrices.  An empty cell
//   gets zeros.
// Every product, sum and quotient is one fp32 rounding (dcinterp::mul_rn / add_rn), no contraction.
//
// Bounds against the same formulas in fp64 on the fp32 table (tests/test_cluster_vectors_host.py asserts them).  u = 2^-24 and
// gamma(k) = k u / (1 - k u): a term that passes through at most k roundings is off by at most gamma(k) of its magnitude.
//   sum       a member adds two products (one rounding each) and two additions; the first addition of a list is exact (+0 + p),
//             so the first term passes through 1 + (2 cnt - 1) roundings and every later one through fewer:
//             |out - out64| <= gamma(2 cnt) S, S = sum over the members of |R00 v0| + |R01 v1|  (to first order 2 cnt u S)
//   mean      one more rounding, the quotient's: gamma(2 cnt + 1) S / cnt
//   gather    two products and one sum: every term passes through two roundings: gamma(2) T, T = |R00 g0| + |R10 g1|
//             (2 u T to first order -- NOT the 3 u a count of the three operations suggests: the sum's rounding is shared)
//   mean bwd  the quotient first: three roundings per term, gamma(3) T with T on the exact quotients
//   unpool bwd  the sum's form over the L members of a cell: gamma(2 L) T
//   max       three roundings on non-negative terms put the fp32 key within [(1 - u)^2, (1 + u)^2] of the exact squared norm, so the
//             winner's exact key is at least (1 - u)^2 / (1 + u)^2 >= 1 - 4 u = 1 - 2^-22 of the largest: where the exact keys
//             differ by more than that, fp32 selects what fp64 selects.  The value is a gather: gamma(2) of that member's magnitude
#pragma once
#include <stdint.h>

#include "cluster_math.h"
#include "pool_vectors_math.h"

namespace dcclv {
using dccl::in_cell;
using dccl::MAX_ROWS;
using dccl::NO_ARG;
using dcconn::R4;
using dcinterp::add_rn;
using dcinterp::load4;
using dcinterp::mul_rn;
using dcvpool::mode_ok;
using dcvpool::MODE_MAX;
using dcvpool::MODE_MEAN;
using dcvpool::MODE_SUM;

// Table entry of point i: fine = the frames (normal, x, y) [N,3] of the points, coarse = those [M,3] of the cells.  to_cell: the
// direction "down" (into the cell's frame; the fine y-axes are not read), else "up" (into the point's; the coarse y-axes are not).
DC_HD R4 rotation(long long i, long long cl, long long m, const float* fn, const float* fx, const float* fy, const float* cn,
                  const float* cx, const float* cy, int to_cell, int non_oriented) {
    if (!in_cell(cl, m)) return R4{0.f, 0.f, 0.f, 0.f};
    if (to_cell)
        return dcconn::transport(dcconn::ld3(cn + 3 * cl), dcconn::ld3(cx + 3 * cl), dcconn::ld3(cy + 3 * cl), dcconn::ld3(fn + 3 * i),
                                 dcconn::ld3(fx + 3 * i), non_oriented);
    return dcconn::transport(dcconn::ld3(fn + 3 * i), dcconn::ld3(fx + 3 * i), dcconn::ld3(fy + 3 * i), dcconn::ld3(cn + 3 * cl),
                             dcconn::ld3(cx + 3 * cl), non_oriented);
}

// Channels c0 .. c0+nc-1 (nc in 1 .. 4) of one cell: v [2 points, ldv], mem [n] the cell's members in ascending order, R [points]
// the table.  TRANSPOSED: through R^T (the un-pooling's backward, mode MODE_SUM over rup); else the pooling over rdown.  vec:
// v + c0 is 16-byte aligned in every row and nc = 4.  ou / ov [4] receive nc values each (rows 2j, 2j+1 of the output), arg [4] the
// row each channel came from (max; -1 for an empty cell and in the other modes).  -> the number of members taken.
template <bool TRANSPOSED>
DC_HD long long walk4(const float* v, long long ldv, long long points, const int64_t* mem, long long n, const R4* R, int mode, int c0,
                      int nc, bool vec, float* ou, float* ov, int* arg) {
    float au[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f}, key[4] = {0.f, 0.f, 0.f, 0.f};
    int at[4] = {NO_ARG, NO_ARG, NO_ARG, NO_ARG};
    long long cnt = 0;
    constexpr int U = 4;                      // members whose loads fly together; the walk itself stays in list order
    for (long long t0 = 0; t0 < n; t0 += U) {
        R4 m[U];
        float v0[U][4], v1[U][4];
        long long row[U];
        bool in[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long j = mem[t0 + u < n ? t0 + u : n - 1];            // (clamped: an unconditional load, masked below)
            in[u] = t0 + u < n && j >= 0 && j < points;
            row[u] = in[u] ? j : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (points > 0) {
                m[u] = R[row[u]];             // one 16-byte load, the same address on every channel group of the cell
                load4(v + (2 * row[u]) * ldv + c0, nc, vec, v0[u]);
                load4(v + (2 * row[u] + 1) * ldv + c0, nc, vec, v1[u]);
            } else {
                m[u] = R4{0.f, 0.f, 0.f, 0.f};
                v0[u][0] = v0[u][1] = v0[u][2] = v0[u][3] = v1[u][0] = v1[u][1] = v1[u][2] = v1[u][3] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!in[u]) continue;
            const bool first = cnt == 0;
            const float a00 = m[u].r00, a01 = TRANSPOSED ? m[u].r10 : m[u].r01, a10 = TRANSPOSED ? m[u].r01 : m[u].r10, a11 = m[u].r11;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (mode == MODE_MAX) {
                    const float k = add_rn(mul_rn(v0[u][c], v0[u][c]), mul_rn(v1[u][c], v1[u][c]));
                    const bool take = first || k > key[c];
                    const float tu = add_rn(mul_rn(a00, v0[u][c]), mul_rn(a01, v1[u][c]));
                    const float tv = add_rn(mul_rn(a10, v0[u][c]), mul_rn(a11, v1[u][c]));
                    key[c] = take ? k : key[c];
                    au[c] = take ? tu : au[c];
                    av[c] = take ? tv : av[c];
                    at[c] = take ? (int)row[u] : at[c];
                } else {
                    au[c] = add_rn(add_rn(au[c], mul_rn(a00, v0[u][c])), mul_rn(a01, v1[u][c]));
                    av[c] = add_rn(add_rn(av[c], mul_rn(a10, v0[u][c])), mul_rn(a11, v1[u][c]));
                }
            }
            ++cnt;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ou[c] = mode == MODE_MEAN && cnt > 0 ? au[c] / (float)cnt : au[c];
        ov[c] = mode == MODE_MEAN && cnt > 0 ? av[c] / (float)cnt : av[c];
        arg[c] = mode == MODE_MAX ? at[c] : NO_ARG;
    }
    return cnt;
}

// Channels c0 .. c0+nc-1 of the two rows of point `row`, cl its cluster id and r its table entry: g [2 M, ldg] the rows of the
// cells.  TRANSPOSED: the pooling's backward (through R^T, with arg [M, ldarg] read by max and cptr [M+1] by mean); else the
// un-pooling (through R; the mode is not looked at).  vec: g + c0 is 16-byte aligned in every row and nc = 4.
template <bool TRANSPOSED>
DC_HD void gather4(const float* g, long long ldg, long long m, long long cl, long long row, R4 r, const int64_t* cptr,
                   const int32_t* arg, long long ldarg, int mode, int c0, int nc, bool vec, float* o0, float* o1) {
    o0[0] = o0[1] = o0[2] = o0[3] = o1[0] = o1[1] = o1[2] = o1[3] = 0.f;
    if (!in_cell(cl, m)) return;
    float g0[4], g1[4];
    load4(g + (2 * cl) * ldg + c0, nc, vec, g0);
    load4(g + (2 * cl + 1) * ldg + c0, nc, vec, g1);
    const float a00 = r.r00, a01 = TRANSPOSED ? r.r10 : r.r01, a10 = TRANSPOSED ? r.r01 : r.r10, a11 = r.r11;
    const bool mean = TRANSPOSED && mode == MODE_MEAN, max = TRANSPOSED && mode == MODE_MAX;
    const float div = mean ? (float)(cptr[cl + 1] - cptr[cl]) : 1.f;
    for (int c = 0; c < nc; ++c) {
        const float t0 = mean ? g0[c] / div : g0[c], t1 = mean ? g1[c] / div : g1[c];
        const bool hit = !max || (long long)arg[cl * ldarg + c0 + c] == row;
        o0[c] = hit ? add_rn(mul_rn(a00, t0), mul_rn(a01, t1)) : 0.f;
        o1[c] = hit ? add_rn(mul_rn(a10, t0), mul_rn(a11, t1)) : 0.f;
    }
}

}  // namespace dcclv
