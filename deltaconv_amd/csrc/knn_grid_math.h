// Arithmetic of the exact k-nearest-neighbour search over a uniform cell grid (knn_grid.hip), shared with the g++ host-check build
// (tests/hostcheck_knn_grid) like interp_math.h / fps_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// EXACT: the same neighbours in the same order as the brute-force kernels (knn.hip, interp.hip: knn_cross_kernel), bit for bit.
// The grid only decides WHICH candidates are looked at and when the search may stop; a candidate's distance is the contract's own
// expression (dist2 below = dcinterp::dist2), and the kept list is sorted by the explicit key (d2, index), so neither the order in
// which cells are walked nor the order of the points inside a cell can reach the result.
//
// Every rule is fixed so that a numpy restatement (tests/knn_grid_restate.py) reproduces the bits:
//   box       lo, hi: fp32 minimum / maximum per axis over the reference points whose three coordinates are all finite (m of them);
//             a point with a non-finite coordinate belongs to no cell and is never picked (the contract of dc_knn_cross)
//   cells     make_grid(m, lo, hi, target), a function of those four alone, in fp64 operations that IEEE rounds the same everywhere
//             (+ - * / floor ceil, no pow / cbrt):
//               want   = clamp(floor(m / target), 1, max(1, 2 m))                  cells wanted; `target` = mean points per cell
//               ext[a] = hi[a] - lo[a] in fp32; the axis is ACTIVE when ext is finite and > 0
//               g_s[a] = ceil(ext[a] / ext_max * s) for active axes, 1 otherwise   (s cells along the longest axis: cubic cells)
//               s      = the largest of 1 .. MAX_AXIS with g_s[0] g_s[1] g_s[2] <= want   (s = 1 gives one cell: always allowed)
//               inv_h[a] = (float)(g[a] / ext[a]) where g[a] > 1 and that quotient lies in [1e-30, 3e38]; otherwise the axis gets
//               exactly ONE cell and inv_h = 0 (zero or non-finite extent, inverse cell size not finite, or nothing to divide)
//             so every axis has at most MAX_AXIS = 1024 cells and the product is at most max(1, 2 m): the workspace is linear in the
//             number of points and computable on the host from sizes alone
//   cell      per axis clamp((int)floorf((p - lo) * inv_h), 0, g - 1), the subtraction and the product each rounded to fp32; the
//             clamp is applied to the float (a query outside the box -- the cross form -- lands in the border cell; no overflow
//             of the conversion); the cell id is (cz * g[1] + cy) * g[0] + cx: runs along x are contiguous
//   distance  dx = q.x - c.x, ...; d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded to fp32, no contraction
//   kept      the K smallest keys (d2, index), lexicographic; only a candidate with d2 BELOW +inf (NaN and overflow never enter)
//   rings     r = 0, 1, 2, ...: the cells at Chebyshev distance exactly r from the query's cell, clipped to the grid
//   stop      after ring r when k candidates are held and the k-th d2 is STRICTLY below bound2(r); or when the rings covered the grid
//
// The stopping bound.  Claim: a reference point p in a cell at Chebyshev distance > r from the query's cell has COMPUTED
// d2 >= bound2(r) for r >= 1 (bound2(0) = 0: ring 1 is always visited).  Take an axis a on which the cells differ by >= r + 1
// (so g = g[a] > 1), write h = 1 / inv_h[a] (real), eps = 2^-24, and u(x) = fl(fl(x - lo) * inv_h), the float whose floor is the
// cell before the clamp.
//   1. Monotonicity.  Subtracting a constant, multiplying by a positive constant, rounding, floor and clamp are all non-decreasing,
//      so the cell is a non-decreasing function of the coordinate.  Say p lies above (cp >= cq + r + 1; the other side mirrors).
//      cp >= 1 was not clamped from below, so u(p) >= cp; cq <= g - 2 was not clamped from above, so u(q) < cq + 1.  Hence
//      u(p) - u(q) > cp - cq - 1 >= r.  A query outside the box: below lo it has cq = 0, u(p) >= r + 1 and q < lo, which gives
//      p - q > p - lo >= (r + 1) h / (1 + eps)^2, more than what follows; above hi it cannot lie below p's cell, and when p lies
//      below it, hi itself has the last cell (u(hi) >= g (1 - 3 eps) >= g - 1), so hi replaces q with |q - p| > hi - p.
//   2. Rounding of (p - lo) * inv_h.  With both coordinates in [lo, hi]: x - lo in [0, ext], each of the two operations errs by a
//      factor (1 +- eps) (an underflowing product by 2^-150 absolute), so
//        r < u(p) - u(q) <= inv_h (p - q) + 2 ext inv_h (2 eps + eps^2) + 2^-149,
//      and ext inv_h <= g (1 + eps)^2 <= MAX_AXIS (1 + eps)^2 (inv_h is a quotient rounded to fp64, then to fp32, and at least 1e-30:
//      normal).  With MAX_AXIS = 2^10 the middle term is at most 2^-12 (1 + 2^-20): |p - q| > (r - 2^-12 (1 + 2^-20)) h
//      >= r h (1 - 2^-12 (1 + 2^-20)).  THIS is the term that grows with the per-axis cap.
//   3. Rounding of d2.  dx = fl(q - p) has |dx| >= |p - q| (1 - eps); fl(dx dx) >= dx^2 (1 - eps) - 2^-150; adding non-negative
//      terms and rounding never goes below the representable first operand: d2 >= fl(dx dx).  Together
//        d2 >= r^2 h^2 (1 - 2^-12 (1 + 2^-20))^2 (1 - eps)^3 - 2^-150 >= r^2 h^2 (1 - 2^-11 - 2^-21) - 2^-150.
//   4. The bound as computed.  min_h = min over the axes with more than one cell of fl(1 / inv_h) <= h (1 + eps);
//      B = fl(fl(r min_h) (1 - 2^-10)) and bound2 = fl(B B) <= r^2 h^2 (1 - 2^-10)^2 (1 + eps)^7 <= r^2 h^2 (1 - 2^-9 + 2^-19).
//      bound2 is used only where it is at least 1e-30 (else 0: no early stop), which makes the 2^-150 of step 3 a relative 2^-50,
//      and is cut to 1e37 (a smaller bound is still a bound; no overflow to +inf).  So bound2(r) < d2 of every unvisited point, with
//      a margin of about 2^-10: a point not yet seen can neither beat nor TIE the k-th kept key once that key is below bound2(r).
#pragma once
#include <math.h>
#include <stdint.h>

#include "point_math.h"

namespace dcgrid {

constexpr int MAX_AXIS = 1024;                // cells per axis (the derivation above holds up to this cap)
constexpr float DEFAULT_TARGET = 1.0f;        // mean points per cell where the caller passes no target (README: measured)
constexpr float SLACK = 0.9990234375f;        // 1 - 2^-10
constexpr float B2_MIN = 1e-30f, B2_MAX = 1e37f;

DC_HD float inf() { return __builtin_huge_valf(); }
DC_HD bool finite1(float x) { return fabsf(x) <= 3.4028234663852886e38f; }      // false for NaN and +-inf
DC_HD bool finite3(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z); }

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

// The grid of one reference cloud: 12 words, the record the kernels keep per cloud.
struct Grid {
    float lo[3];
    float inv_h[3];
    int g[3];
    float min_h;                              // min over the axes with g > 1 of fl(1 / inv_h); 0 when the grid is one cell
    int m;                                    // reference points with three finite coordinates
    int cells;                                // g[0] * g[1] * g[2]
};

DC_HD long long cells_at(const double* ratio, const bool* act, int s, int* g) {
    long long prod = 1;
    for (int a = 0; a < 3; ++a) {
        int c = 1;
        if (act[a]) {
            const double v = ceil(ratio[a] * (double)s);
            c = v < 1.0 ? 1 : (v > (double)MAX_AXIS ? MAX_AXIS : (int)v);
        }
        g[a] = c;
        prod *= c;
    }
    return prod;
}

DC_HD void make_grid(long long m, const float* lo, const float* hi, float target, Grid& G) {
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = m > 0 ? lo[a] : 0.f;
        G.inv_h[a] = 0.f;
        G.g[a] = 1;
    }
    G.min_h = 0.f;
    G.m = (int)(m > 0 ? m : 0);
    G.cells = 1;
    if (m <= 0) return;
    const double cap = 2.0 * (double)m;
    double want = floor((double)m / (double)target);
    want = want < 1.0 ? 1.0 : (want > cap ? cap : want);     // (a NaN quotient cannot occur: target is positive and finite)
    double ext[3], ratio[3], ext_max = 0.0;
    bool act[3];
    for (int a = 0; a < 3; ++a) {
        const float e = hi[a] - lo[a];
        act[a] = finite1(e) && e > 0.f;
        ext[a] = (double)e;
        if (act[a] && ext[a] > ext_max) ext_max = ext[a];
    }
    if (!(ext_max > 0.0)) return;
    for (int a = 0; a < 3; ++a) ratio[a] = act[a] ? ext[a] / ext_max : 0.0;
    int g[3];
    int s_ok = 1, s_hi = MAX_AXIS;            // s_ok is allowed; find the largest allowed s
    while (s_ok < s_hi) {
        const int mid = (s_ok + s_hi + 1) >> 1;
        if ((double)cells_at(ratio, act, mid, g) <= want) s_ok = mid;
        else s_hi = mid - 1;
    }
    cells_at(ratio, act, s_ok, g);
    float min_h = 0.f;
    for (int a = 0; a < 3; ++a) {
        if (g[a] <= 1) continue;
        const double ih = (double)g[a] / ext[a];
        if (!(ih >= 1e-30 && ih <= 3e38)) continue;          // the axis keeps one cell
        G.g[a] = g[a];
        G.inv_h[a] = (float)ih;
        const float h = 1.0f / G.inv_h[a];
        min_h = (min_h == 0.f || h < min_h) ? h : min_h;
    }
    G.min_h = min_h;
    G.cells = G.g[0] * G.g[1] * G.g[2];
}

DC_HD int cell_axis(float p, float lo, float inv_h, int g) {
    if (g <= 1) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = floorf(__fmul_rn(__fsub_rn(p, lo), inv_h));
#else
    const float a = p - lo;
    const float u = a * inv_h;
    const float t = floorf(u);
#endif
    return t >= (float)(g - 1) ? g - 1 : (t > 0.f ? (int)t : 0);
}

DC_HD int cell_of(const Grid& G, int cx, int cy, int cz) { return (cz * G.g[1] + cy) * G.g[0] + cx; }

// bound(r)^2: below the computed d2 of every reference point in a cell at Chebyshev distance > r (the derivation above)
DC_HD float bound2(int r, float min_h) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float b = __fmul_rn(__fmul_rn((float)r, min_h), SLACK);
    const float b2 = __fmul_rn(b, b);
#else
    const float rh = (float)r * min_h;
    const float b = rh * SLACK;
    const float b2 = b * b;
#endif
    return b2 >= B2_MIN ? (b2 <= B2_MAX ? b2 : B2_MAX) : 0.f;
}

// The K smallest keys (d2, index) seen so far, ascending.  Unlike the lists of knn.hip / interp_math.h the candidates arrive in no
// particular index order, so the insertion compares the whole key.  An empty slot holds (+inf, INT_MAX); a candidate enters only
// with d2 below +inf.
template <int K>
struct TopKLex {
    float d[K];
    int id[K];
    DC_HD void init() {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            d[s] = inf();
            id[s] = 0x7fffffff;
        }
    }
    static DC_HD bool less(float ad, int ai, float bd, int bi) { return ad < bd || (ad == bd && ai < bi); }
    DC_HD void push(float nd, int nid) {
        if (nd < inf() && less(nd, nid, d[K - 1], id[K - 1])) {
#pragma unroll
            for (int s = K - 1; s > 0; --s) {
                const bool shift = less(nd, nid, d[s - 1], id[s - 1]);
                const bool place = less(nd, nid, d[s], id[s]);
                const float vd = shift ? d[s - 1] : nd;
                const int vi = shift ? id[s - 1] : nid;
                d[s] = place ? vd : d[s];
                id[s] = place ? vi : id[s];
            }
            if (less(nd, nid, d[0], id[0])) {
                d[0] = nd;
                id[0] = nid;
            }
        }
    }
    DC_HD float kth(int k) const {            // d[k - 1] without a dynamic register index
        float v = d[K - 1];
#pragma unroll
        for (int s = 0; s < K - 1; ++s) v = (s == k - 1) ? d[s] : v;
        return v;
    }
};

// A reference point in cell order: position and its id local to the cloud, 16 bytes (one load a candidate).
struct alignas(16) Pt {
    float x, y, z;
    int id;
};

// cells [c0, c1) of the cloud: a contiguous run of the cell-ordered points.  cstart: the cloud's slice of the exclusive scan of
// the per-cell counts (entry c1 exists: the scan has one entry more than cells); the run is cut to [0, cap).
template <int K>
DC_HD void visit_run(const Pt* pts, const int64_t* cstart, long long cap, int c0, int c1, float qx, float qy, float qz,
                     TopKLex<K>& best) {
    long long s = cstart[c0], e = cstart[c1];
    s = s < 0 ? 0 : s;
    e = e > cap ? cap : e;
    for (long long j = s; j < e; ++j) {
        const Pt p = pts[j];
        best.push(dist2(qx, qy, qz, p.x, p.y, p.z), p.id);
    }
}

// The search of one query with three finite coordinates: rings around its cell until the stopping rule holds.
template <int K>
DC_HD void search(const Grid& G, const Pt* pts, const int64_t* cstart, long long cap, float qx, float qy, float qz, int k,
                  TopKLex<K>& best) {
    const int gx = G.g[0], gy = G.g[1], gz = G.g[2];
    const int cx = cell_axis(qx, G.lo[0], G.inv_h[0], gx);
    const int cy = cell_axis(qy, G.lo[1], G.inv_h[1], gy);
    const int cz = cell_axis(qz, G.lo[2], G.inv_h[2], gz);
    int rmax = cx > gx - 1 - cx ? cx : gx - 1 - cx;
    rmax = cy > rmax ? cy : rmax;
    rmax = gy - 1 - cy > rmax ? gy - 1 - cy : rmax;
    rmax = cz > rmax ? cz : rmax;
    rmax = gz - 1 - cz > rmax ? gz - 1 - cz : rmax;
    for (int r = 0;; ++r) {
        const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < gz - 1 ? cz + r : gz - 1;
        const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < gy - 1 ? cy + r : gy - 1;
        const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < gx - 1 ? cx + r : gx - 1;
        const bool xl = cx - r >= 0, xh = cx + r < gx && r > 0;        // the two end cells of an inner row, where they exist
        for (int z = z0; z <= z1; ++z) {
            const bool zface = z == cz - r || z == cz + r;
            for (int y = y0; y <= y1; ++y) {
                const int row = cell_of(G, 0, y, z);
                if (zface || y == cy - r || y == cy + r) {
                    visit_run(pts, cstart, cap, row + x0, row + x1 + 1, qx, qy, qz, best);
                } else if (xl || xh) {
                    if (xl) visit_run(pts, cstart, cap, row + cx - r, row + cx - r + 1, qx, qy, qz, best);
                    if (xh) visit_run(pts, cstart, cap, row + cx + r, row + cx + r + 1, qx, qy, qz, best);
                } else {
                    y = cy + r - 1 < y1 ? cy + r - 1 : y1;             // nothing of this ring in the inner rows: on to the far face
                }
            }
        }
        if (r >= rmax) break;                                          // the rings have covered the grid
        if (best.kth(k) < bound2(r, G.min_h)) break;
    }
}

}  // namespace dcgrid
