// Arithmetic of the two-set nearest-neighbour search and the inverse-squared-distance interpolation (interp.hip), shared with the
// g++ host-check build (tests/hostcheck_interp) like mesh_math.h / fps_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// What is being restated: torch_cluster.knn(x, y, k, batch_x, batch_y) and torch_geometric.nn.knn_interpolate (unpool/
// knn_interpolate.py: squared distances, weights = 1 / clamp(d2, min=1e-16), y = sum(w * x) / sum(w)) -- PointNet++ feature
// propagation.  The gradient w.r.t. the FEATURES x is restated below (coef / pick / bwd4); there is NO gradient for positions or
// distances: PyG's op is differentiable through the weights, this one is not.
//
// Every rule is fixed so that a numpy restatement (tests/interp_restate.py) reproduces the bits:
//   distance  fp32, dx = q - r per axis, ((dx*dx + dy*dy) + dz*dz), every operation rounded on its own (no contraction): the
//             order contract of dc_knn (knn.hip:5-6)
//   order     ascending distance, ties by the lower reference index: candidates are fed by ASCENDING index and a candidate is
//             placed behind every kept entry with distance <= its own
//   taken     only a candidate whose distance is BELOW +inf: a NaN distance (a NaN coordinate in the query or the candidate)
//             and a distance that overflowed to +inf compare false and are never picked
//   empty     a slot that found no candidate holds idx = -1, d2 = +inf
//   weight    w_s = 1.0f / fmaxf(d2_s, 1e-16f)  (PyG's clamp; fmaxf: a NaN d2 counts as the clamp)
//   sum       slots s = 0 .. k-1 in order, a slot with idx outside [0, Nr) skipped (nothing is indexed): num = num + w_s * x_s,
//             den = den + w_s from num = den = 0, every operation rounded on its own; then out = num / den, one division a channel
//   one slot  a query with exactly ONE valid slot gets that row copied bit for bit (k = 1 is an exact gather)
//   no slot   a query with no valid slot gets a row of zeros
//
// The backward w.r.t. x (tests/interp_grad_restate.py restates it; dc_knn_cross_transpose / dc_knn_interpolate_backward run it):
//   coef      of slot s of query q: walk the slots s = 0 .. k-1 as interp4 does (valid iff 0 <= idx < Nr), w_s = weight(d2_s) and
//             den = den + w_s in that order -- the forward's den bits; then c_s = 1.0f when the query has exactly ONE valid slot
//             (the forward copied the row), otherwise c_s = w_s / den, one division.  An invalid slot has no coefficient.
//   in-edges  of reference row j: every valid (q, s) of its cloud pair with idx[q, s] == j, named e = row(q) * k + s (row(q): the
//             query's row in the call), in ASCENDING e
//   sum       dx[j, ch] = 0, then for every in-edge in that order dx = dx + c_e * g[row(q_e), ch], the product and the sum each
//             rounded on their own (__fmul_rn / __fadd_rn on the device, as dist2); a row without in-edges gets zeros
#pragma once
#include <stdint.h>

#include "point_math.h"

namespace dcinterp {

constexpr int MAX_K = 16;                     // neighbours per query
constexpr float D2_CLAMP = 1e-16f;            // knn_interpolate's clamp(min=1e-16)

DC_HD float inf() { return __builtin_huge_valf(); }

DC_HD float dist2(float qx, float qy, float qz, float rx, float ry, float rz) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float dx = __fsub_rn(qx, rx), dy = __fsub_rn(qy, ry), dz = __fsub_rn(qz, rz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
#else
    const float dx = qx - rx, dy = qy - ry, dz = qz - rz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
#endif
}

// The K smallest (d2, index) seen so far, ascending (the sorted-insertion list of knn.hip).  Feed the candidates by ASCENDING
// index: a candidate goes behind every entry with distance <= its own, so equal distances stay ordered by index.  Every
// comparison is a strict `<` against a list that starts at +inf: NaN and +inf never enter.
template <int K>
struct TopK {
    float d[K];
    int id[K];
    DC_HD void init() {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            d[s] = inf();
            id[s] = -1;
        }
    }
    DC_HD void push(float nd, int nid) {
        if (nd < d[K - 1]) {
#pragma unroll
            for (int s = K - 1; s > 0; --s) {
                const bool shift = nd < d[s - 1];
                const bool place = nd < d[s];
                const float vd = shift ? d[s - 1] : nd;
                const int vi = shift ? id[s - 1] : nid;
                d[s] = place ? vd : d[s];
                id[s] = place ? vi : id[s];
            }
            if (nd < d[0]) {
                d[0] = nd;
                id[0] = nid;
            }
        }
    }
};

DC_HD float weight(float d2) { return 1.0f / fmaxf(d2, D2_CLAMP); }

struct alignas(16) F4 {
    float v[4];
};

// The guarded load of a channel group: r [4] = nc values at row (one 16-byte load when vec), zeros behind them.
DC_HD void load4(const float* row, int nc, bool vec, float* r) {
    r[0] = r[1] = r[2] = r[3] = 0.f;
    if (vec) {
        const F4 t = *reinterpret_cast<const F4*>(row);
        r[0] = t.v[0]; r[1] = t.v[1]; r[2] = t.v[2]; r[3] = t.v[3];
    } else {
        for (int c = 0; c < nc; ++c) r[c] = row[c];
    }
}

// Channels c0 .. c0+nc-1 (nc in 1 .. 4) of one query: x [Nr, ldx] the rows of ITS reference cloud, idx / d2 [k] its slots.
// vec: x + c0 is 16-byte aligned in every row and nc = 4 (one 16-byte load per slot).  out [4] receives nc values.
DC_HD void interp4(const float* x, long long ldx, long long nr, int k, const int* idx, const float* d2, int c0, int nc, bool vec,
                   float* out) {
    float num[4] = {0.f, 0.f, 0.f, 0.f}, only[4] = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    int valid = 0;
    for (int s = 0; s < k; ++s) {
        const long long j = idx[s];
        if (j < 0 || j >= nr) continue;
        const float w = weight(d2[s]);
        float r[4];
        load4(x + j * ldx + c0, nc, vec, r);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float p = w * r[c];
            num[c] = num[c] + p;
            only[c] = r[c];
        }
        den = den + w;
        ++valid;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = valid == 0 ? 0.f : (valid == 1 ? only[c] : num[c] / den);
}

// ---- backward w.r.t. x ------------------------------------------------------------------------------------------------------------
DC_HD float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    const float p = a * b;
    return p;
#endif
}
DC_HD float add_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    const float s = a + b;
    return s;
#endif
}

DC_HD bool valid_slot(long long j, long long nr) { return j >= 0 && j < nr; }

// The coefficient of slot s of one query (idx / d2 [k] its slots, nr the size of ITS reference cloud); 0 for an invalid slot.
DC_HD float coef(long long nr, int k, const int* idx, const float* d2, int s) {
    float den = 0.f, ws = 0.f;
    int valid = 0;
    for (int t = 0; t < k; ++t) {
        if (!valid_slot(idx[t], nr)) continue;
        const float w = weight(d2[t]);
        den = den + w;
        ws = t == s ? w : ws;
        ++valid;
    }
    if (!valid_slot(idx[s], nr)) return 0.f;
    return valid == 1 ? 1.0f : ws / den;
}

// The cloud pair of query row q: the b in [0, B) with qptr[b] <= q < qptr[b+1], or -1 (a row outside every pair).
DC_HD int pair_of(const int64_t* qptr, int B, long long q) {
    int lo = 0, hi = B + 1;                   // the number of offsets <= q, by bisection
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qptr[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    const int b = lo - 1;
    return b >= 0 && b < B ? b : -1;
}

// The reference row (absolute) that edge e = q * k + s feeds, or -1: no pair, or an invalid slot.
DC_HD long long pick(const int64_t* qptr, const int64_t* rptr, int B, int k, const int* idx, long long e) {
    const int b = pair_of(qptr, B, e / k);
    if (b < 0) return -1;
    const long long rbase = rptr[b], nr = rptr[b + 1] - rbase, j = idx[e];
    return valid_slot(j, nr) ? rbase + j : -1;
}

// Channels c0 .. c0+nc-1 of one reference row's gradient: its in-edges tedge / tcoef [n] in ascending order, g [rows, ldg] the
// gradient of the call's query rows, row of edge e = e / k - edge_base (an edge whose row falls outside [0, rows) is skipped:
// lists that do not belong to g).  vec: g + c0 is 16-byte aligned in every row and nc = 4.  out [4] receives nc values.
DC_HD void bwd4(const float* g, long long ldg, long long rows, int k, long long edge_base, const int64_t* tedge,
                const float* tcoef, long long n, int c0, int nc, bool vec, float* out) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;                      // in-edges whose loads fly together; the sum itself stays in list order
    for (long long t0 = 0; rows > 0 && t0 < n; t0 += U) {
        float c[U], r[U][4];
        bool in[U];
        const float* gr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long t = t0 + u < n ? t0 + u : n - 1;             // (clamped: an unconditional load, masked below)
            const long long e = tedge[t];
            const long long row = (e >> 32 ? e / k : (long long)((unsigned)e / (unsigned)k)) - edge_base;
            in[u] = t0 + u < n && row >= 0 && row < rows;
            c[u] = tcoef[t];
            gr[u] = g + (in[u] ? row : 0) * ldg + c0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) load4(gr[u], nc, vec, r[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) acc[ch] = in[u] ? add_rn(acc[ch], mul_rn(c[u], r[u][ch])) : acc[ch];
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) out[ch] = acc[ch];
}

}  // namespace dcinterp
