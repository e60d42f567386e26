// Parallel transport between tangent frames: the per-edge 2x2 connection and the sums over it.  Written once and shared by
//   * the HIP kernels (connection.hip) -- the product, and
//   * tests/hostcheck_connection -- a g++ build of the SAME functions looped over edges / points on the CPU.
// Both sides are compiled with -ffp-contract=off: every product, sum, quotient and square root below is one fp32 rounding, in
// the order written, which is what tests/connection_restate.py restates operation by operation in numpy.
//
// Reference being restated: deltaconv/geometry/connection.py (build_transport :6-47, angle_in_plane :50-59, rotate_around
// :62-76).  transport() takes the reference's cos / sin of atan2(y, x) as x / r and y / r (r = sqrt(x*x + y*y)): the same two
// numbers without libm, so the function has ONE fp32 value on every side.  angle_in_plane() / rotate_around() keep atan2f /
// sincosf and are held to a tolerance only.
#pragma once
#include "ell_math.h"

namespace dcconn {
using dcell::Vec;
using dcell::vload;
using dcell::vout;
using dcell::vstore;
using dcell::vzero;

constexpr float AXIS_EPS = 1e-6f;   // connection.py:21,34: below it the axis / the projected x-axis has no direction
constexpr float NORM_CLAMP = 1e-8f; // connection.py:52,54,69: clamp of the normalisations

struct F3 {
    float x, y, z;
};
struct alignas(16) R4 {             // one connection, row-major: [r00 r01; r10 r11]
    float r00, r01, r10, r11;
};

DC_HD F3 ld3(const float* p) { return F3{p[0], p[1], p[2]}; }
DC_HD float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
DC_HD F3 cross3(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
DC_HD float norm3(F3 a) { return sqrtf(dot3(a, a)); }
DC_HD F3 neg3(F3 a) { return F3{-a.x, -a.y, -a.z}; }
DC_HD F3 scale3(F3 a, float s) { return F3{a.x * s, a.y * s, a.z * s}; }
DC_HD F3 div3(F3 a, float s) { return F3{a.x / s, a.y / s, a.z / s}; }
DC_HD F3 sub3(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
DC_HD F3 add3(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
DC_HD F3 normalize_clamped(F3 a, float eps) { return div3(a, fmaxf(norm3(a), eps)); }

// coordinates of v in the plane orthogonal to `normal`, x-axis along the projection of u   (connection.py:51-57)
DC_HD void plane_coords(F3 u, F3 v, F3 normal, float* xc, float* yc) {
    const F3 up = normalize_clamped(sub3(u, scale3(normal, dot3(u, normal))), NORM_CLAMP);
    const F3 by = normalize_clamped(cross3(normal, up), NORM_CLAMP);
    *xc = dot3(v, up);
    *yc = dot3(v, by);
}

// v turned about `axis` by the angle whose cosine / sine are c / s   (connection.py:66-76)
DC_HD F3 rotate_cs(F3 v, F3 axis, float c, float s) {
    const F3 par = scale3(axis, dot3(v, axis));
    const F3 tc = sub3(v, par);
    const float tl = fmaxf(norm3(tc), NORM_CLAMP);
    const F3 bx = div3(tc, tl);
    const F3 by = cross3(axis, bx);
    const F3 rot = add3(scale3(add3(scale3(bx, c), scale3(by, s)), tl), par);
    return tl > 0.f ? rot : par;
}

// One edge: the matrix that takes a vector's coordinates in the source frame (sn, sx, sn x sx) to the target frame
// (tn, tx, ty).  Normals pointing apart (sn . tn < 0) flip the target's normal and y-axis first; with non_oriented the
// result then carries the reflection (determinant -1).
//
// A frame seen from itself (sn == tn and sx == tx, component by component) is the identity by definition and returned as
// such: the steps below give b = tx . ty there, which is 0 only for a frame that is orthogonal exactly (the self edges of a
// kNN graph on build_tangent_basis frames carry up to 3e-8, in the reference's fp32 output too).  The value is the one the
// steps give for b = +0: (1, -0, 0, 1).
DC_HD R4 transport(F3 tn, F3 tx, F3 ty, F3 sn, F3 sx, int non_oriented) {
    if (sn.x == tn.x && sn.y == tn.y && sn.z == tn.z && sx.x == tx.x && sx.y == tx.y && sx.z == tx.z)
        return R4{1.f, -0.f, 0.f, 1.f};
    const bool inverted = dot3(sn, tn) < 0.f;
    if (inverted) {
        tn = neg3(tn);
        ty = neg3(ty);
    }
    F3 axis = cross3(tn, sn);
    const float an = norm3(axis);
    axis = an > AXIS_EPS ? div3(axis, an) : sx;
    float xc, yc;
    plane_coords(sn, tn, axis, &xc, &yc);
    const float r = sqrtf(xc * xc + yc * yc);
    const float c = r > 0.f ? xc / r : 1.f, s = r > 0.f ? yc / r : 0.f;
    const F3 rot = rotate_cs(sx, axis, c, s);
    float a = dot3(rot, tx), b = dot3(rot, ty);
    const float l = sqrtf(a * a + b * b);
    const bool ok = l > AXIS_EPS;
    a = ok ? a / l : 1.f;
    b = ok ? b / l : 0.f;
    const float conj = (non_oriented && inverted) ? -1.f : 1.f;
    return R4{a, -b, b * conj, a * conj};
}

DC_HD float angle_in_plane(F3 u, F3 v, F3 normal) {
    float xc, yc;
    plane_coords(u, v, normal, &xc, &yc);
    return atan2f(yc, xc);
}

DC_HD F3 rotate_around(F3 v, F3 axis, float angle) {
    float s, c;
    sincosf(angle, &s, &c);
    return rotate_cs(v, axis, c, s);
}

// ---- sums over the connection ------------------------------------------------------------------------------------------------
// Vector fields as in ell_math.h: rows 2i, 2i+1 hold the two components at point i.  coef[e] = R4 of edge e = i*k + s.
//   out[2i+a, c] = scale * acc_a,  acc_a = (acc_a + coef[i,s,a,0] * v[2j,c]) + coef[i,s,a,1] * v[2j+1,c],  j = nbr[i,s], s ascending
template <int V>
DC_HD void transport_sum_fwd(long i, int c0, const int* ids, const R4* cf, int k, const float* v, long ldv, float scale,
                             float* out, long ldo) {
    Vec<V> au = vzero<V>(), av = vzero<V>();
#pragma unroll 4
    for (int s = 0; s < k; ++s) {
        const R4 r = cf[s];
        const long j = ids[s];
        const Vec<V> v0 = vload<V>(v + (2 * j) * ldv + c0), v1 = vload<V>(v + (2 * j + 1) * ldv + c0);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            au.v[q] = (au.v[q] + r.r00 * v0.v[q]) + r.r01 * v1.v[q];
            av.v[q] = (av.v[q] + r.r10 * v0.v[q]) + r.r11 * v1.v[q];
        }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) {
        au.v[q] = scale * au.v[q];
        av.v[q] = scale * av.v[q];
    }
    vstore<V>(out + (2 * i) * ldo + c0, au);
    vstore<V>(out + (2 * i + 1) * ldo + c0, av);
}

// the transpose, an accumulator of the transposed skeleton (ell_math.h): in-edges e = i*k + s of point j, ascending,
//   dv_b = (dv_b + coef[e,0,b] * g[2i,c]) + coef[e,1,b] * g[2i+1,c],  dv[2j+b, c] (+)= scale * dv_b
template <int V>
struct TransportSumT {
    const R4* coef; int k; const float* g; long ldg; float scale; float* dv; long ldv; int accumulate; int C;
    Vec<V> au, av;
    DC_HD void init() { au = vzero<V>(); av = vzero<V>(); }
    DC_HD void step(long i, int s, dcell::G2, int c0) {
        const R4 r = coef[i * k + s];
        const Vec<V> g0 = vload<V>(g + (2 * i) * ldg + c0), g1 = vload<V>(g + (2 * i + 1) * ldg + c0);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            au.v[q] = (au.v[q] + r.r00 * g0.v[q]) + r.r10 * g1.v[q];
            av.v[q] = (av.v[q] + r.r01 * g0.v[q]) + r.r11 * g1.v[q];
        }
    }
    DC_HD void finish(long j, int c0) {
#pragma unroll
        for (int q = 0; q < V; ++q) {
            au.v[q] = scale * au.v[q];
            av.v[q] = scale * av.v[q];
        }
        vout<V>(dv + (2 * j) * ldv + c0, au, accumulate);
        vout<V>(dv + (2 * j + 1) * ldv + c0, av, accumulate);
    }
};

}  // namespace dcconn
