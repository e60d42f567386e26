// g++ build of deltaconv_amd/csrc/mesh_normal_math.h -- the corner-to-vertex map, the face contributions, the ordered sum and the
// final normalisation of the per-vertex normals (mesh_normal.hip), looped over corners / vertices on the CPU
// (tests/test_mesh_normal_host.py).
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/mesh_normal_math.h"

extern "C" {

// vf_ptr [num_verts+1], vf_edge [3*num_faces] of a store: count, scan and a fill in ascending corner slot, serially (the order
// the device's ranking pass restores).  -> the number of entries written.
int64_t hn_lists(const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B, int64_t num_verts, int64_t num_faces,
                 int64_t* vf_ptr, int64_t* vf_edge) {
    const long long ne = 3 * (long long)num_faces;
    std::vector<int64_t> cursor(num_verts + 1, 0);
    for (long long e = 0; e < ne; ++e) {
        const long long v = dcvnorm::corner_vertex(face, vptr, fptr, B, num_verts, e);
        if (v >= 0) ++cursor[v];
    }
    int64_t run = 0;
    for (int64_t v = 0; v < num_verts; ++v) {
        vf_ptr[v] = run;
        run += cursor[v];
        cursor[v] = vf_ptr[v];
    }
    vf_ptr[num_verts] = run;
    for (long long e = 0; e < ne; ++e) {
        const long long v = dcvnorm::corner_vertex(face, vptr, fptr, B, num_verts, e);
        if (v >= 0) vf_edge[cursor[v]++] = e;
    }
    return run;
}

// normals [num_verts,3] and zero_count [B] (or null) on finished lists: the body of vertex_normals_kernel, one vertex at a time
void hn_normals(const float* vert, const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B, int64_t num_verts,
                int64_t num_faces, const int64_t* vf_ptr, const int64_t* vf_edge, int32_t weighting, float* normals,
                int32_t* zero_count) {
    for (int32_t b = 0; zero_count && b < B; ++b) zero_count[b] = 0;
    for (int64_t v = 0; v < num_verts; ++v) {
        const int b = dcinterp::pair_of(vptr, B, v);
        if (b < 0) continue;
        const bool zero = dcvnorm::vertex_normal(vert, face, vptr[b], vptr[b + 1] - vptr[b], fptr[b], fptr[b + 1] - fptr[b],
                                                 vf_edge + vf_ptr[v], vf_ptr[v + 1] - vf_ptr[v], weighting, normals + 3 * v);
        if (zero && zero_count) ++zero_count[b];
    }
}

// one face's contribution [3] (both weightings are cases of the tests)
void hn_contribution(const float* p0, const float* p1, const float* p2, int32_t weighting, float* t) {
    dcvnorm::face_contribution(p0, p1, p2, weighting, t);
}

}  // extern "C"
