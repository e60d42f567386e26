// Arithmetic of the two-set nearest-neighbour search and the inverse-squared-distance interpolation (interp.hip), shared with the
// g++ host-check build (tests/hostcheck_interp) like mesh_math.h / fps_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// What is being restated: torch_cluster.knn(x, y, k, batch_x, batch_y) and torch_geometric.nn.knn_interpolate (unpool/
// knn_interpolate.py: squared distances, weights = 1 / clamp(d2, min=1e-16), y = sum(w * x) / sum(w)) -- PointNet++ feature
// propagation.  Inference only: nothing here has a backward.
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
#pragma once
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
        const float* row = x + j * ldx + c0;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            const F4 t = *reinterpret_cast<const F4*>(row);
            r[0] = t.v[0]; r[1] = t.v[1]; r[2] = t.v[2]; r[3] = t.v[3];
        } else {
            for (int c = 0; c < nc; ++c) r[c] = row[c];
        }
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

}  // namespace dcinterp
