// Arithmetic of the device surface sampler of triangle meshes (mesh.hip), shared with the g++ host-check build
// (tests/hostcheck_mesh) like batch_math.h / fps_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// Reference being restated: deltaconv/transforms/sample_points.py:22-59 (here transforms.SamplePoints) -- faces drawn with a
// probability proportional to their area, uniform barycentric coordinates with the fold of :36-38, the point in the order of
// :46-48, the normal by F.normalize of the edge cross product (:41-44), the label of corner 0 (:53-54).
//
// Everything that decides WHICH face a sample lands on is integer arithmetic or order-free, so the result is a function of
// the inputs only and a numpy restatement (tests/mesh_restate.py) reproduces it bit for bit:
//   area     fp64 from the widened fp32 vertices: e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2, a = sqrt((cx*cx + cy*cy) + cz*cz)
//            (twice the triangle's area: only ratios matter).  A face with a vertex id outside [0, V) or a non-finite a has a = 0.
//   weight   w = amax > 0 ? (uint64) ((a / amax) * 2^32) : 0 with amax the largest a of the mesh (a maximum has no order),
//            truncating cast, w in [0, 2^32].  A face below 2^-32 of the largest has weight 0.
//   cdf      inclusive sums of w in face order, uint64 (integer addition is associative: any scan shape gives these bits);
//            total = cdf[F-1] < 2^57 for the at most 2^24 faces of a mesh.
//   draw     Philox-4x32-10 (nn_math.h), key (seed, "mesh"), counter (sample j, DATASET index of the mesh, round lo, round hi).
//   pick     u = x << 32 | y; t = high 64 bits of u * total; the FIRST face with cdf[f] > t (zero-weight faces are never
//            picked).  total = 0 (every face degenerate): f = high 64 bits of u * F, uniform by index.
//   fold     f1 = (z >> 8) * 2^-24, f2 = (w >> 8) * 2^-24 in fp32; f1 + f2 > 1 (fp32 sum): f1 = 1 - f1, f2 = 1 - f2 (both exact).
//   point    fp32, every operation rounded on its own: p = (p0 + f1 * e1) + f2 * e2 per axis.  The reference's division by
//            pos.max() and the multiplication back only condition its fp32 area sum and are not restated.
//   normal   fp32: c = e1 x e2, n = c / max(sqrtf((cx*cx + cy*cy) + cz*cz), 1e-12f); a degenerate face gives a zero normal.
#pragma once
#include "nn_math.h"

namespace dcmesh {

typedef unsigned long long u64;

constexpr unsigned MESH_KEY = 0x6D657368u;    // "mesh"; the batch assembly uses 0x6261746B, the dropout 0x64726F70
constexpr float NORMAL_EPS = 1e-12f;          // F.normalize's eps

// twice the area of face (i0, i1, i2) of a mesh of V vertices, fp64; 0 where an id is out of range (nothing is indexed then) or the
// value is not finite
DC_HD double face_area(const float* vert, long long V, long long i0, long long i1, long long i2) {
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return 0.0;
    const float *p0 = vert + 3 * i0, *p1 = vert + 3 * i1, *p2 = vert + 3 * i2;
    const double ax = (double)p0[0], ay = (double)p0[1], az = (double)p0[2];
    const double e1x = (double)p1[0] - ax, e1y = (double)p1[1] - ay, e1z = (double)p1[2] - az;
    const double e2x = (double)p2[0] - ax, e2y = (double)p2[1] - ay, e2z = (double)p2[2] - az;
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const double a = sqrt((cx * cx + cy * cy) + cz * cz);
    return (a == a && a < __builtin_huge_val()) ? a : 0.0;
}

DC_HD u64 face_weight(double a, double amax) { return amax > 0.0 ? (u64)((a / amax) * 4294967296.0) : 0ull; }

DC_HD u64 mulhi64(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

DC_HD dcnn::U4 draw(unsigned seed, long long round, unsigned mesh, unsigned j) {
    const u64 r = (u64)round;
    return dcnn::philox4x32_10(dcnn::U4{j, mesh, (unsigned)r, (unsigned)(r >> 32)}, seed, MESH_KEY);
}

// the face of one draw: cdf [F] of the mesh, F >= 1
DC_HD long long pick_face(const u64* cdf, long long F, unsigned x, unsigned y) {
    const u64 u = (u64)x << 32 | (u64)y;
    const u64 total = cdf[F - 1];
    if (total == 0) return (long long)mulhi64(u, (u64)F);
    const u64 t = mulhi64(u, total);               // < total: the search ends inside the mesh
    long long lo = 0, hi = F - 1;                  // cdf[F-1] = total > t
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

DC_HD void fold(unsigned z, unsigned w, float& f1, float& f2) {
    f1 = (float)(z >> 8) * (1.0f / 16777216.0f);
    f2 = (float)(w >> 8) * (1.0f / 16777216.0f);
    const float s = f1 + f2;
    if (s > 1.0f) {
        f1 = 1.0f - f1;
        f2 = 1.0f - f2;
    }
}

// point and normal of barycentric (f1, f2) on the triangle (p0, p1, p2): fp32, every operation rounded on its own
DC_HD void point_normal(const float* p0, const float* p1, const float* p2, float f1, float f2, float* pos, float* nrm) {
    float e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = p1[a] - p0[a];
        e2[a] = p2[a] - p0[a];
        const float t1 = f1 * e1[a], t2 = f2 * e2[a];
        const float s = p0[a] + t1;
        pos[a] = s + t2;
    }
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = fmaxf(sqrtf((cx * cx + cy * cy) + cz * cz), NORMAL_EPS);
    nrm[0] = cx / len;
    nrm[1] = cy / len;
    nrm[2] = cz / len;
}

// Sample j of the mesh with dataset index `mesh`: vert [V,3], face [F,3] (ids local to the mesh), cdf [F], y_vert [V] or null.
// Every output is written: pos [3], nrm [3], *y (the label of corner 0; -1 without y_vert), *face_id, f12 [2] (the folded
// coordinates).  A picked face with an id outside [0, V) -- possible only where total = 0 picks by index -- is not indexed: zero
// point, zero normal, label -1.
DC_HD void sample_one(const float* vert, long long V, const int* face, long long F, const u64* cdf, const long long* y_vert,
                      unsigned seed, long long round, unsigned mesh, unsigned j, float* pos, float* nrm, long long* y,
                      int* face_id, float* f12) {
    const dcnn::U4 r = draw(seed, round, mesh, j);
    const long long f = pick_face(cdf, F, r.x, r.y);
    float f1, f2;
    fold(r.z, r.w, f1, f2);
    f12[0] = f1;
    f12[1] = f2;
    *face_id = (int)f;
    const long long i0 = face[3 * f], i1 = face[3 * f + 1], i2 = face[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
        pos[0] = pos[1] = pos[2] = 0.f;
        nrm[0] = nrm[1] = nrm[2] = 0.f;
        *y = -1;
        return;
    }
    point_normal(vert + 3 * i0, vert + 3 * i1, vert + 3 * i2, f1, f2, pos, nrm);
    *y = y_vert ? y_vert[i0] : -1;
}

DC_HD unsigned long long workspace_bytes(long long F_total) { return F_total > 0 ? (unsigned long long)F_total * 8ull : 0ull; }

}  // namespace dcmesh
