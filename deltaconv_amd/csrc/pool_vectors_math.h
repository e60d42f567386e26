// Arithmetic of the cross-cloud pooling of tangent-vector features (pool_vectors.hip), shared with the g++ host-check build
// (tests/hostcheck_pool_vectors) like pool_math.h / interp_transport_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// What is being restated: the set-abstraction step of PointNet++ (pool_math.h) for the VECTOR stream: every point of a sampled
// cloud reduces the tangent vectors of its k nearest points of the full cloud, each first carried into the sampled point's frame
// by parallel transport (deltaconv/geometry/connection.py:6-47, dcconn::transport).  The reference has no such call site.  Unlike
// the transported interpolation (interp_transport_math.h) no distance weight enters: on a sampled SUBSET the weight
// 1 / max(d2, 1e-16) of the coincident point is 1e16, its coefficient exactly 1.0f, and the interpolation is a gather.  Vector
// fields as in ell_math.h: rows 2i, 2i+1 hold the two coefficients at point i.  Only the VALUES are differentiated.
//
// Every rule is fixed so that a numpy restatement (tests/pool_vectors_restate.py) reproduces the bits:
//   table     slot e = q * k + s of query row q (pair b, nr = rptr[b+1] - rptr[b]) holds R = dcconn::transport(target frame of q,
//             source frame of rptr[b] + idx[e], non_oriented): the matrix alone, no coefficient.  A row in no pair and a slot with
//             idx outside [0, nr) hold four +0.0f.  Frames are indexed by the ABSOLUTE rows qptr / rptr name.
//   valid     slot s of query q is valid iff 0 <= idx[q,s] < nr (dcinterp::valid_slot), never from R; an invalid slot is skipped
//   mode      0 max, 2 sum, 3 mean: the codes of dc_seg_reduce (1, min, has no vector analogue and is refused)
//   cnt       the number of valid slots of the query, one uint8 per query row, in every mode
//   sum       au = av = +0; valid slots s = 0 .. k-1 in order: au = (au + R00*v0) + R01*v1, av = (av + R10*v0) + R11*v1 with v0 / v1
//             rows 2j, 2j+1 of the source values, j = rptr[b] + idx: the order of dcvinterp::fwd4
//   mean      the sum, then ONE division per component by (float)cnt
//   max       per channel.  The key of a slot is n = v0*v0 + v1*v1, two products and one sum, in the SOURCE frame (R is orthogonal
//             up to rounding, so the choice depends on no frame).  The first valid slot is taken; a later one replaces it iff
//             n > n_acc: strict, so ties keep the earlier (nearer) slot; a NaN key in a later slot compares false and is never taken,
//             a NaN key in the first valid slot stays (the rule of pool_math.h).  The output is the winner's transported vector
//             (R00*v0 + R01*v1, R10*v0 + R11*v1): two products and one sum each, no zero start.  arg = the winning slot
//   no slot   a query without a valid slot gets zeros, arg = 255, cnt = 0
//
// The backward w.r.t. the values on the lists of dc_knn_cross_transpose (tptr / tedge; tcoef is not read):
//   in-edges  of source row r: every valid (q, s) of its pair with idx[q,s] == r - rptr[b], named e = q * k + s, in ASCENDING e
//   sum       du = dw = +0; per in-edge, R = table[e], g0 / g1 rows 2q, 2q+1 of g:
//             du = (du + R00*g0) + R10*g1, dw = (dw + R01*g0) + R11*g1  (dcvinterp::bwd4 on the rotation table)
//   mean      the same with g0, g1 each first divided by (float)cnt[q], every quotient rounded on its own
//   max       the same, iff arg[q,ch] == s; an edge that lost adds NOTHING (no + 0)
//   skipped   an edge whose query row falls outside [0, rows of g); a row without in-edges gets zeros.  No atomics.
// Every product, sum and quotient is one fp32 rounding (dcinterp::mul_rn / add_rn), no contraction.
//
// Bounds against the same formulas in fp64 on the fp32 table (tests/test_pool_vectors_host.py asserts them), u = 2^-24:
//   sum       every valid slot adds two products (one rounding each, relative u) and two additions; with S = sum_s (|R00 v0| +
//             |R01 v1|) per component no partial sum exceeds S (1 + O(cnt u)), so each of the 2 cnt additions errs by at most u S and
//             the product roundings by u S in all: |out - out64| <= (2 cnt + 1) u S to first order.  The first addition of a slot
//             list is exact (+0 + p), which pays for the products' share: |out - out64| <= 2 cnt u S.
//   mean      the sum's error divided by cnt, plus one rounding of the quotient (u S / cnt): (2 cnt + 1) u S / cnt
//   backward  the same form over the L in-edges of a row with T = sum_e (|R00 g0| + |R10 g1|): 2 L u T for sum and max (L the edges
//             that add), (2 L + 1) u T for mean, whose terms carry one more rounding (the quotient) each
//   max       three roundings on non-negative terms put the fp32 key within (1 + u)^2 of the exact squared norm, so the chosen
//             slot's exact squared norm is at least (1 - u)^2 / (1 + u)^2 >= 1 - 2^-22 of the largest; the value is within
//             3 u (|R00 v0| + |R01 v1|) of the fp64 transport of that slot (two products, one sum)
#pragma once
#include <stdint.h>

#include "connection_math.h"
#include "interp_math.h"
#include "pool_math.h"

namespace dcvpool {
using dcconn::R4;
using dcinterp::add_rn;
using dcinterp::load4;
using dcinterp::mul_rn;
using dcpool::load_arg4;
using dcpool::MODE_MAX;
using dcpool::MODE_MEAN;
using dcpool::MODE_SUM;
using dcpool::NO_ARG;
using dcpool::store_arg4;

DC_HD bool mode_ok(int mode) { return mode == MODE_MAX || mode == MODE_SUM || mode == MODE_MEAN; }

// Slot s of query row q (absolute) whose pair starts at reference row rbase and holds nr reference rows.
DC_HD R4 rotation_in_pair(long long q, int s, long long rbase, long long nr, int k, const int* idx, const float* tn, const float* tx,
                          const float* ty, const float* sn, const float* sx, int non_oriented) {
    const long long j = idx[q * k + s];
    if (!dcinterp::valid_slot(j, nr)) return R4{0.f, 0.f, 0.f, 0.f};
    const long long r = rbase + j;
    return dcconn::transport(dcconn::ld3(tn + 3 * q), dcconn::ld3(tx + 3 * q), dcconn::ld3(ty + 3 * q), dcconn::ld3(sn + 3 * r),
                             dcconn::ld3(sx + 3 * r), non_oriented);
}

// The table entry of slot e = q * k + s of the call.  HOST-SIDE wrapper (tests/hostcheck_pool_vectors): it finds the pair by
// bisection; the kernel takes its pair from the grid and never visits a row outside every pair.
DC_HD R4 rotation(const int64_t* qptr, const int64_t* rptr, int B, int k, const int* idx, const float* tn, const float* tx,
                  const float* ty, const float* sn, const float* sx, int non_oriented, long long e) {
    const long long q = e / k;
    const int b = dcinterp::pair_of(qptr, B, q);
    if (b < 0) return R4{0.f, 0.f, 0.f, 0.f};
    return rotation_in_pair(q, (int)(e - q * k), rptr[b], rptr[b + 1] - rptr[b], k, idx, tn, tx, ty, sn, sx, non_oriented);
}

// Channels c0 .. c0+nc-1 (nc in 1 .. 4) of one query: v [2 Nr, ldv] the rows of ITS reference cloud, idx [k] / R [k] its slots.
// vec: v + c0 is 16-byte aligned in every row and nc = 4.  ou / ov [4] receive nc values each (rows 2q, 2q+1 of the output), arg [4]
// the slot each channel came from (max; 255 without a valid slot and in the other modes).  -> cnt, the number of valid slots.
DC_HD int fwd4(const float* v, long long ldv, long long nr, int k, const int* idx, const R4* R, int mode, int c0, int nc, bool vec,
               float* ou, float* ov, unsigned char* arg) {
    float au[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f}, key[4] = {0.f, 0.f, 0.f, 0.f};
    int at[4] = {NO_ARG, NO_ARG, NO_ARG, NO_ARG};
    int cnt = 0;
    for (int s = 0; s < k; ++s) {
        const long long j = idx[s];
        if (!dcinterp::valid_slot(j, nr)) continue;
        const R4 m = R[s];                    // one 16-byte load, the same address on every channel group of the query
        float v0[4], v1[4];
        load4(v + (2 * j) * ldv + c0, nc, vec, v0);
        load4(v + (2 * j + 1) * ldv + c0, nc, vec, v1);
        const bool first = cnt == 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (mode == MODE_MAX) {
                const float n = add_rn(mul_rn(v0[c], v0[c]), mul_rn(v1[c], v1[c]));
                const bool take = first || n > key[c];
                const float tu = add_rn(mul_rn(m.r00, v0[c]), mul_rn(m.r01, v1[c]));
                const float tv = add_rn(mul_rn(m.r10, v0[c]), mul_rn(m.r11, v1[c]));
                key[c] = take ? n : key[c];
                au[c] = take ? tu : au[c];
                av[c] = take ? tv : av[c];
                at[c] = take ? s : at[c];
            } else {
                au[c] = add_rn(add_rn(au[c], mul_rn(m.r00, v0[c])), mul_rn(m.r01, v1[c]));
                av[c] = add_rn(add_rn(av[c], mul_rn(m.r10, v0[c])), mul_rn(m.r11, v1[c]));
            }
        }
        ++cnt;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ou[c] = mode == MODE_MEAN && cnt > 0 ? au[c] / (float)cnt : au[c];
        ov[c] = mode == MODE_MEAN && cnt > 0 ? av[c] / (float)cnt : av[c];
        arg[c] = (unsigned char)at[c];
    }
    return cnt;
}

// Channels c0 .. c0+nc-1 of one source row's gradient: its in-edges tedge [n] in ascending order, g [2 rows, ldg] the gradient of
// the call's query rows, R [rows * k] the rotation table, arg [rows, ldarg] / cnt [rows] what the forward wrote (arg is read by max
// only, cnt by mean only).  Query row of edge e = e / k, slot e - row * k, table entry e; an edge whose row falls outside [0, rows)
// is skipped (its table entry would fall outside the table too).  vec: g + c0 is 16-byte aligned in every row and nc = 4; word:
// arg + c0 is 4-byte aligned in every row and nc = 4.  du / dw [4] receive nc values each.  MODE at compile time, for the register
// reason recorded at dcpool::bwd4.
template <int MODE>
DC_HD void bwd4(const float* g, long long ldg, long long rows, int k, const int64_t* tedge, const R4* R, long long n,
                const unsigned char* arg, long long ldarg, const unsigned char* cnt, int c0, int nc, bool vec, bool word, float* du,
                float* dw) {
    constexpr int mode = MODE;
    float au[4] = {0.f, 0.f, 0.f, 0.f}, aw[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;                      // in-edges whose loads fly together; the sum itself stays in list order
    for (long long t0 = 0; rows > 0 && t0 < n; t0 += U) {
        R4 m[U];
        float g0[U][4], g1[U][4], div[U];
        uint32_t a[U], slot[U];              // four slot numbers a word: the forward's, and the edge's own in every byte
        bool in[U];
        long long row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long t = t0 + u < n ? t0 + u : n - 1;             // (clamped: an unconditional load, masked below)
            const long long e = tedge[t];
            const long long q = e >> 32 ? e / k : (long long)((unsigned)e / (unsigned)k);
            in[u] = t0 + u < n && e >= 0 && q < rows;
            slot[u] = (uint32_t)(e - q * k) * 0x01010101u;
            row[u] = in[u] ? q : 0;
            m[u] = R[in[u] ? e : 0];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load4(g + (2 * row[u]) * ldg + c0, nc, vec, g0[u]);
            load4(g + (2 * row[u] + 1) * ldg + c0, nc, vec, g1[u]);
            a[u] = mode == MODE_MAX ? load_arg4(arg + row[u] * ldarg + c0, nc, word) : slot[u];     // sum / mean: every in-edge counts
            div[u] = mode == MODE_MEAN ? (float)cnt[row[u]] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const bool hit = in[u] && (((a[u] ^ slot[u]) >> 8 * ch) & 255u) == 0;
                const float t0g = mode == MODE_MEAN ? g0[u][ch] / div[u] : g0[u][ch];
                const float t1g = mode == MODE_MEAN ? g1[u][ch] / div[u] : g1[u][ch];
                au[ch] = hit ? add_rn(add_rn(au[ch], mul_rn(m[u].r00, t0g)), mul_rn(m[u].r10, t1g)) : au[ch];
                aw[ch] = hit ? add_rn(add_rn(aw[ch], mul_rn(m[u].r01, t0g)), mul_rn(m[u].r11, t1g)) : aw[ch];
            }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        du[ch] = au[ch];
        dw[ch] = aw[ch];
    }
}

}  // namespace dcvpool
