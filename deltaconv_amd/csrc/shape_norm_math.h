// Arithmetic of the per-shape normalisation of a device-resident store (shape_norm.hip), shared with the g++ host-check build
// (tests/hostcheck_shapenorm) like mesh_math.h / batch_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// Reference being restated (here the host classes of deltaconv_amd/transforms/__init__.py):
//   SCALE  deltaconv/transforms/normalize_scale.py:12-21   centre on the bounding-box middle, multiply by (1 / ref) * 0.999999
//   AREA   deltaconv/transforms/normalize_area.py:12-20    centre, multiply by 1 / sqrt(A), A the surface area
//   AXES   deltaconv/transforms/normalize_axes.py:17-26    columns in the order of ascending unbiased standard deviation, multiply
//                                                          by 1 / (2 * max of the last column)
// normalize_area.py indexes data.face[:, 1]: with the [3, F] faces its dataset stores, that reads the three vertex ids of face 1,
// not corner 1 of every face.  transforms.NormalizeArea is pinned to the reference when fed [F, 3], the layout in which the
// formula IS the surface area; this op is the surface area over face ROWS, i.e. T.NormalizeArea on Data(pos, face=[F,3]).  In the
// ShapeSeg recipe the difference vanishes: NormalizeAxes follows and rescales uniformly, so only the centring of NormalizeArea
// survives.  Neither side is to be "fixed".
//
// Every op maps fp32 rows to fp32 rows, out[j] = fl32(fl32(in[perm[j]] - c[perm[j]]) * s), and the next op sees the rounded
// result, as the host Compose does; the kernel recomputes earlier ops per element and rounds at these same places.
//   centre   c = fl32(fl32(max + min) / 2) per axis (SCALE, AREA; AXES has c = 0, and x - 0 is x).  The maximum and minimum have
//            no order: a NaN gives the canonical NaN, of two zeros the maximum is +0 and the minimum -0.
//   SCALE    per row of q = fl32(p - c): d = (x*x + y*y) + z*z in fp64 from the widened q (ord 2), or max(|x|, |y|, |z|) in fp32
//            (ord inf); the maximum over rows; ref = fl32(sqrt(d)) (ord inf: the maximum itself); with a scaling_factor, ref is
//            that constant.  s = fl32(fl32(1 / ref) * 0.999999f).
//   AREA     S = the ordered fp64 sum over the shape's face rows of dcmesh::face_area on q (twice the area; a face with an id
//            outside [0, V) or a non-finite area counts 0, as in the sampler); s = fl32(1 / sqrt(S / 2)), rounded once.
//   AXES     per axis the ordered fp64 sums of x and x*x (the square of an fp32 value is exact in fp64); var = (Sxx - Sx*Sx / n) /
//            (n - 1); perm = the stable order of the three variances: axis j moves in front of a lower axis only where its
//            variance is strictly below, so a tie or a NaN keeps the lower axis first and n = 1 (0 / 0) keeps the identity;
//            s = fl32(1 / fl32(2 * max of the column that ends up last)).
//   ordered sum  of v[0 .. n) with T = NORM_T "threads": partial[t] = ((0 + v[t]) + v[t + T]) + ... in index order, then within
//            every group of 64 partials the halving tree a[i] += a[i + o] for o = 32, 16, .., 1, then over the T / 64 group sums
//            the halving tree for o = T / 128, .., 1.  A function of the shape alone: not of B, of the shape's position in the
//            store or of the grouping into calls.  (x + y is y + x bit for bit, so the xor butterfly of a wave is this tree.)
// Non-finite arithmetic follows IEEE as the host transforms do; a zero-area shape gets an infinite scale; nothing is clamped.
#pragma once
#include "mesh_math.h"

namespace dcnorm {

constexpr int NORM_T = 1024;                  // threads of a parameter workgroup: the order of the sums depends on it
constexpr int NORM_WAVES = NORM_T / 64;
constexpr int MAX_OPS = 4;
constexpr int STAT_WORDS = 8;                 // stats [B, n_ops, 8]: centre 3, scale 1, permutation 3, spare 1
enum { OP_SCALE = 1, OP_AREA = 2, OP_AXES = 3 };

// one op of one shape, as the stats row holds it
struct Op {
    float c[3];
    float s;
    int perm[3];
};

DC_HD Op identity_op() { return Op{{0.f, 0.f, 0.f}, 1.f, {0, 1, 2}}; }

// v[a] for a in 0 .. 2 without a dynamically indexed register array
DC_HD float pick3(const float* v, int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }

DC_HD void apply_op(const Op& op, const float* in, float* out) {
    float t[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int a = op.perm[j];
        const float q = pick3(in, a) - pick3(op.c, a);
        t[j] = q * op.s;
    }
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
}

// the row after the first k ops of a chain (in and out may be the same array)
DC_HD void apply_chain(const Op* ops, int k, const float* in, float* out) {
    float r[3] = {in[0], in[1], in[2]};
    for (int i = 0; i < k; ++i) apply_op(ops[i], r, r);
    out[0] = r[0]; out[1] = r[1]; out[2] = r[2];
}

// order-free maximum / minimum (carried in fp64: an fp32 value widens exactly)
DC_HD double nan_free() { return __builtin_nan(""); }
DC_HD bool sign_of(double a) { return __builtin_signbit(a); }
DC_HD double omax(double a, double b) {
    if (a != a || b != b) return nan_free();
    if (a > b) return a;
    if (b > a) return b;
    return sign_of(a) ? b : a;                // equal: of -0 and +0 the maximum is +0
}
DC_HD double omin(double a, double b) {
    if (a != a || b != b) return nan_free();
    if (a < b) return a;
    if (b < a) return b;
    return sign_of(a) ? a : b;                // equal: of -0 and +0 the minimum is -0
}

DC_HD float centre_of(float mx, float mn) {
    const float t = mx + mn;
    return t / 2.0f;
}

DC_HD double row_norm2(const float* q) {
    const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
    return (x * x + y * y) + z * z;
}
DC_HD double row_norm_inf(const float* q) {
    return omax(omax((double)__builtin_fabsf(q[0]), (double)__builtin_fabsf(q[1])), (double)__builtin_fabsf(q[2]));
}
// ref of SCALE from the maximum over rows
DC_HD float scale_ref(double dmax, bool ord_inf) { return ord_inf ? (float)dmax : (float)sqrt(dmax); }
DC_HD float scale_of_ref(float ref) {
    const float r = 1.0f / ref;
    return r * 0.999999f;
}

// twice the area of the face whose three corner rows are q0, q1, q2 (already centred): the sampler's face area
DC_HD double face_area_rows(const float* q0, const float* q1, const float* q2) {
    const float tri[9] = {q0[0], q0[1], q0[2], q1[0], q1[1], q1[2], q2[0], q2[1], q2[2]};
    return dcmesh::face_area(tri, 3, 0, 1, 2);
}
DC_HD float area_scale(double S) { return (float)(1.0 / sqrt(S / 2.0)); }

DC_HD double axes_var(double sx, double sxx, long long n) {
    const double dn = (double)n;
    const double m2 = sx * sx;
    const double corr = m2 / dn;
    const double num = sxx - corr;
    return num / (dn - 1.0);
}
DC_HD void axes_perm(const double* var, int* perm) {
    perm[0] = 0; perm[1] = 1; perm[2] = 2;
    for (int i = 1; i < 3; ++i)               // insertion sort, strict comparison: stable, a NaN never moves anything
        for (int j = i; j > 0 && var[perm[j]] < var[perm[j - 1]]; --j) {
            const int t = perm[j];
            perm[j] = perm[j - 1];
            perm[j - 1] = t;
        }
}
DC_HD float axes_scale(float mx) {
    const float d = 2.0f * mx;
    return 1.0f / d;
}

// the tree over the NORM_T partial sums (the host-check build runs it; the kernel's shuffles and LDS form the same tree)
DC_HD double tree_sum(double* part) {
    for (int w = 0; w < NORM_WAVES; ++w)
        for (int o = 32; o > 0; o >>= 1)
            for (int i = 0; i < o; ++i) part[64 * w + i] = part[64 * w + i] + part[64 * w + i + o];
    for (int o = NORM_WAVES / 2; o > 0; o >>= 1)
        for (int i = 0; i < o; ++i) part[64 * i] = part[64 * i] + part[64 * (i + o)];
    return part[0];
}

DC_HD void write_stats(float* st, const Op& op) {
    st[0] = op.c[0]; st[1] = op.c[1]; st[2] = op.c[2];
    st[3] = op.s;
    st[4] = (float)op.perm[0]; st[5] = (float)op.perm[1]; st[6] = (float)op.perm[2];
    st[7] = 0.f;
}
DC_HD Op read_stats(const float* st) {
    Op op;
    op.c[0] = st[0]; op.c[1] = st[1]; op.c[2] = st[2];
    op.s = st[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int a = (int)st[4 + j];
        op.perm[j] = a < 0 ? 0 : (a > 2 ? 2 : a);    // a table from elsewhere indexes nothing outside the row
    }
    return op;
}

}  // namespace dcnorm
