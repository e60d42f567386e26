// Arithmetic of the per-vertex normals of a device-resident mesh store (mesh_normal.hip), shared with the g++ host-check build
// (tests/hostcheck_mesh_normal) like mesh_math.h / interp_math.h / shape_norm_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// Reference being restated: torch_geometric.transforms.GenerateMeshNormals as experiments/train_shapeseg.py:31 calls it (here the
// host class transforms.GenerateMeshNormals).  Per face a = p1 - p0, b = p2 - p0, c = a x b:
//   uniform (0)  the face gives c / max(|c|, 1e-12) to each of its three corners (PyG's, the default)
//   area    (1)  the face gives c itself
//   vertex       n = s / max(|s|, 1e-12), s the sum over the vertex's incident face corners; no incident corner or s = 0: the
//                zero vector.  A zero-area face gives zero, a face that names a vertex twice gives to it twice.  The face winding
//                decides the sign; inconsistent winding is not repaired.
// Everything is fp32, every operation rounded on its own (the build passes -ffp-contract=off), |v| = sqrt((x*x + y*y) + z*z), and
// the sum of a vertex is SEQUENTIAL over its list in ascending 3 * store_face_row + corner, starting from +0.  Within a mesh that
// order is the order of (its face rows, corner) whatever the mesh's place in the store, so a vertex's normal is a function of its
// mesh alone; permuting the faces of a mesh may change the last bits.  A numpy restatement (tests/mesh_normal_restate.py)
// reproduces it bit for bit.  A face row with an id outside [0, V) has no corner in any list and gives nothing; nothing is indexed
// outside the ranges the offsets give.
//
// Distance to the fp64 evaluation of the same formula on the same fp32 vertices, u = 2^-24, first order in u, per vertex with a
// list of L corners and the fp64 contributions t_f and sum s (the bound tests/test_mesh_normal_host.py holds the restatement to):
//   |n32 - n64|_inf <= ((8 * sum_f w_f + (L + 4) * sum_f |t_f|) * u) / |s| + 4 * u
//   edges        a, b: one subtraction per component, relative error u each.
//   cross        a component x*y - z*w carries u from each of its four edge components, u from each product and u from the
//                subtraction: |dc_j| <= 4u (|x y| + |z w|) <= 4u |a||b| by Cauchy-Schwarz, so |dc|_2 <= sqrt(3) * 4u |a||b| < 8u |a||b|.
//                area: this IS the error of the contribution, w_f = |a||b|.  uniform: a perturbation dc turns the unit vector by at
//                most |dc|_2 / |c|, w_f = |a||b| / |c| (0 for a zero-area face: c = 0 exactly in both precisions).
//   unit (uniform)  the norm: two squares and two sums under a square root, (3u / 2 + u); the division: u.  Below 4u |t_f|.
//   sum          L - 1 additions after the first, each u of a partial sum that is at most sum_f |t_f|: (L - 1) u sum_f |t_f|.
//                With the 4u of the line above: (L + 4) u sum_f |t_f|, loose by 1 (uniform) or 5 (area).
//   vertex       an error ds of the sum turns n by |ds| / |s|; the norm and the division of the last step add 3.5u |n| <= 4u.
#pragma once
#include <stdint.h>

#include "interp_math.h"

namespace dcvnorm {

constexpr float NORMAL_EPS = 1e-12f;          // F.normalize's eps
enum { W_UNIFORM = 0, W_AREA = 1 };

DC_HD float norm3(const float* v) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// what face (p0, p1, p2) gives to each of its corners
DC_HD void face_contribution(const float* p0, const float* p1, const float* p2, int weighting, float* t) {
    const float a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const float b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    t[0] = a[1] * b[2] - a[2] * b[1];
    t[1] = a[2] * b[0] - a[0] * b[2];
    t[2] = a[0] * b[1] - a[1] * b[0];
    if (weighting == W_AREA) return;
    const float len = fmaxf(norm3(t), NORMAL_EPS);
    t[0] = t[0] / len;
    t[1] = t[1] / len;
    t[2] = t[2] / len;
}

// one step of the ordered sum
DC_HD void accumulate(float* s, const float* t) {
    s[0] = s[0] + t[0];
    s[1] = s[1] + t[1];
    s[2] = s[2] + t[2];
}

// n = s / max(|s|, eps); -> true where n is the zero vector
DC_HD bool finish(const float* s, float* n) {
    const float len = fmaxf(norm3(s), NORMAL_EPS);
    n[0] = s[0] / len;
    n[1] = s[1] / len;
    n[2] = s[2] / len;
    return n[0] == 0.f && n[1] == 0.f && n[2] == 0.f;
}

// The vertex row (absolute) that corner slot e = 3 * face_row + corner names, or -1: a face row outside every mesh of the call, a
// vertex id outside [0, V) anywhere in that face row (the whole row is dropped, as the sampler drops it), or a vertex past num_verts.
DC_HD long long corner_vertex(const int* face, const int64_t* vptr, const int64_t* fptr, int B, long long num_verts, long long e) {
    const long long f = e / 3;
    const int b = dcinterp::pair_of(fptr, B, f);
    if (b < 0) return -1;
    const long long vbase = vptr[b], nv = vptr[b + 1] - vbase;
    const long long i0 = face[3 * f], i1 = face[3 * f + 1], i2 = face[3 * f + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return -1;
    const long long v = vbase + face[e];
    return v >= 0 && v < num_verts ? v : -1;
}

// The normal of one vertex of the mesh with vertex rows [vbase, vbase + nv) and face rows [fbase, fbase + nf): list [n] its corner
// slots in ascending order.  An entry that names a face row outside the mesh or a row with an id outside [0, V) is skipped (lists
// that do not belong to this store).  -> true where the normal is the zero vector.
DC_HD bool vertex_normal(const float* vert, const int* face, long long vbase, long long nv, long long fbase, long long nf,
                         const int64_t* list, long long n, int weighting, float* out) {
    float s[3] = {0.f, 0.f, 0.f};
    for (long long k = 0; k < n; ++k) {
        const long long f = list[k] / 3;
        if (f < fbase || f >= fbase + nf) continue;
        const long long i0 = face[3 * f], i1 = face[3 * f + 1], i2 = face[3 * f + 2];
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) continue;
        float t[3];
        face_contribution(vert + 3 * (vbase + i0), vert + 3 * (vbase + i1), vert + 3 * (vbase + i2), weighting, t);
        accumulate(s, t);
    }
    return finish(s, out);
}

}  // namespace dcvnorm
