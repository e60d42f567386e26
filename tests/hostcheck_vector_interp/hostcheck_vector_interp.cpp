// g++ build of deltaconv_amd/csrc/interp_transport_math.h (entry / fwd4 / bwd4) -- the per-thread code of dc_knn_cross_transport,
// dc_knn_interpolate_vectors and dc_knn_interpolate_vectors_backward (interp_transport.hip), looped over slots / queries / source
// rows / channel groups on the CPU (tests/test_vector_interp_host.py).  Built without contraction, as the library is.
#include <stdint.h>

#include "../../deltaconv_amd/csrc/interp_transport_math.h"

extern "C" {

// every slot of the call's num_query rows -> tmat [num_query*k, 4]; rows outside every pair get zeros
void hv_table(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int32_t k, const int32_t* idx, const float* d2,
              const float* tn, const float* tx, const float* ty, const float* sn, const float* sx, int32_t non_oriented,
              float* tmat) {
    for (int64_t e = 0; e < num_query * k; ++e) {
        const dcconn::R4 m = dcvinterp::entry(qptr, rptr, B, k, idx, d2, tn, tx, ty, sn, sx, non_oriented, e);
        tmat[4 * e] = m.r00;
        tmat[4 * e + 1] = m.r01;
        tmat[4 * e + 2] = m.r10;
        tmat[4 * e + 3] = m.r11;
    }
}

// v [2 Nr, ldv] -> out rows 2q, 2q+1 of every query of every pair, C channels in groups of 4 as the kernel's threads take them;
// vec: 16-byte loads for whole groups (v 16-byte aligned, ldv a multiple of 4)
void hv_forward(const float* v, int64_t ldv, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B, int32_t k,
                const int32_t* idx, const float* tmat, int32_t vec, float* out, int64_t ldo) {
    const dcconn::R4* M = reinterpret_cast<const dcconn::R4*>(tmat);
    for (int b = 0; b < B; ++b)
        for (int64_t q = qptr[b]; q < qptr[b + 1]; ++q)
            for (int c0 = 0; c0 < C; c0 += 4) {
                const int nc = C - c0 < 4 ? C - c0 : 4;
                float ou[4], ov[4];
                dcvinterp::fwd4(v + 2 * rptr[b] * ldv, ldv, rptr[b + 1] - rptr[b], k, idx + q * k, M + q * k, c0, nc, vec && nc == 4,
                                ou, ov);
                for (int c = 0; c < nc; ++c) {
                    out[(2 * q) * ldo + c0 + c] = ou[c];
                    out[(2 * q + 1) * ldo + c0 + c] = ov[c];
                }
            }
}

// g [2 g_rows, ldg] -> dv rows 2r, 2r+1 of every source row of every pair
void hv_backward(const float* g, int64_t ldg, int64_t g_rows, int32_t C, const int64_t* rptr, int32_t B, int32_t k,
                 const int64_t* tptr, const int64_t* tedge, int64_t edge_base, const float* tmat, int64_t tmat_rows, int32_t vec,
                 float* dv, int64_t ldv) {
    const dcconn::R4* M = reinterpret_cast<const dcconn::R4*>(tmat);
    for (int b = 0; b < B; ++b)
        for (int64_t r = rptr[b]; r < rptr[b + 1]; ++r)
            for (int c0 = 0; c0 < C; c0 += 4) {
                const int nc = C - c0 < 4 ? C - c0 : 4;
                float du[4], dw[4];
                dcvinterp::bwd4(g, ldg, g_rows, k, edge_base, tedge + tptr[r], M, tmat_rows, tptr[r + 1] - tptr[r], c0, nc,
                                vec && nc == 4, du, dw);
                for (int c = 0; c < nc; ++c) {
                    dv[(2 * r) * ldv + c0 + c] = du[c];
                    dv[(2 * r + 1) * ldv + c0 + c] = dw[c];
                }
            }
}

}  // extern "C"
