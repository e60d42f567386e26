// g++ build of deltaconv_amd/csrc/mesh_math.h -- the face weights, the cdf and the per-sample code of the surface sampler
// (mesh.hip), looped over faces / samples on the CPU (tests/test_mesh_host.py).
#include <stdint.h>

#include "../../deltaconv_amd/csrc/mesh_math.h"

extern "C" {

// area [F] fp64, w [F], cdf [F] of one mesh (face [F,3], ids local to the mesh); -> total.  The two passes of mesh_cdf_kernel,
// serially.
uint64_t hm_cdf(const float* vert, int64_t V, const int32_t* face, int64_t F, double* area, uint64_t* w, uint64_t* cdf) {
    double amax = 0.0;
    for (int64_t f = 0; f < F; ++f) {
        area[f] = dcmesh::face_area(vert, V, face[3 * f], face[3 * f + 1], face[3 * f + 2]);
        amax = area[f] > amax ? area[f] : amax;
    }
    dcmesh::u64 run = 0;
    for (int64_t f = 0; f < F; ++f) {
        w[f] = dcmesh::face_weight(area[f], amax);
        run += w[f];
        cdf[f] = run;
    }
    return run;
}

// samples 0 .. num-1 of the mesh drawn as dataset index `mesh`: pos [num,3], norm [num,3], y [num] (or null with y_vert),
// face_id [num], f12 [num,2]
void hm_sample(const float* vert, int64_t V, const int32_t* face, int64_t F, const uint64_t* cdf, const int64_t* y_vert,
               uint32_t seed, int64_t round, int64_t mesh, int32_t num, float* pos, float* norm, int64_t* y, int32_t* face_id,
               float* f12) {
    for (int32_t j = 0; j < num; ++j) {
        long long lab = -1;
        dcmesh::sample_one(vert, V, face, F, reinterpret_cast<const dcmesh::u64*>(cdf), reinterpret_cast<const long long*>(y_vert),
                           seed, round, (unsigned)mesh, (unsigned)j, pos + 3L * j, norm + 3L * j, &lab, face_id + j, f12 + 2L * j);
        if (y) y[j] = lab;
    }
}

uint64_t hm_mulhi64(uint64_t a, uint64_t b) { return dcmesh::mulhi64(a, b); }

}  // extern "C"
