// g++ build of deltaconv_amd/csrc/pool_vectors_math.h (rotation / fwd4 / bwd4) -- the per-thread code of dc_knn_cross_rotation,
// dc_knn_pool_vectors and dc_knn_pool_vectors_backward (pool_vectors.hip), looped over slots / cloud pairs / rows / channel groups
// on the CPU as the frame of cross_stage.h loops them (tests/test_pool_vectors_host.py).  Built without contraction, as the
// library is.
#include <stdint.h>

#include "../../deltaconv_amd/csrc/pool_vectors_math.h"

extern "C" {

// rmat [num_query * k, 4]: every entry written (zeros for a row outside every pair and for an invalid slot)
int hpv_rotation(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int32_t k, const int32_t* idx,
                 const float* tn, const float* tx, const float* ty, const float* sn, const float* sx, int32_t non_oriented,
                 float* rmat) {
    if (k < 1 || k > dcinterp::MAX_K) return -1;
    for (int64_t e = 0; e < num_query * k; ++e) {
        const dcconn::R4 m = dcvpool::rotation(qptr, rptr, B, k, idx, tn, tx, ty, sn, sx, non_oriented, e);
        rmat[4 * e + 0] = m.r00;
        rmat[4 * e + 1] = m.r01;
        rmat[4 * e + 2] = m.r10;
        rmat[4 * e + 3] = m.r11;
    }
    return 0;
}

// v [*,ldv] (two rows a point) -> out [*,ldo] (two rows a query), arg [*,ldarg] (max only), cnt [*] over the query rows of every
// pair.  vec / word as in hostcheck_pool.  -> 0, or -1 for a k outside 1 .. 16 or a mode outside {0, 2, 3}
int hpv_forward(const float* v, int64_t ldv, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B, int32_t k,
                const int32_t* idx, const float* rmat, int32_t mode, int32_t vec, float* out, int64_t ldo, uint8_t* arg,
                int64_t ldarg, int32_t word, uint8_t* cnt) {
    if (k < 1 || k > dcinterp::MAX_K || !dcvpool::mode_ok(mode)) return -1;
    const dcconn::R4* R = reinterpret_cast<const dcconn::R4*>(rmat);
    for (int b = 0; b < B; ++b) {
        const long long nr = rptr[b + 1] - rptr[b];
        for (int64_t row = qptr[b]; row < qptr[b + 1]; ++row)
            for (int c0 = 0; c0 < C; c0 += 4) {
                const int nc = C - c0 < 4 ? C - c0 : 4;
                float u[4], w[4];
                unsigned char a[4];
                const int n = dcvpool::fwd4(v + 2 * rptr[b] * ldv, ldv, nr < 0 ? 0 : nr, k, idx + row * k, R + row * k, mode, c0, nc,
                                            vec && nc == 4, u, w, a);
                for (int c = 0; c < nc; ++c) {
                    out[(2 * row) * ldo + c0 + c] = u[c];
                    out[(2 * row + 1) * ldo + c0 + c] = w[c];
                }
                if (arg && mode == dcvpool::MODE_MAX) dcvpool::store_arg4(arg + row * ldarg + c0, a, nc, word && nc == 4);
                if (c0 == 0) cnt[row] = (unsigned char)n;
            }
    }
    return 0;
}

// g [2 g_rows,ldg] -> dv rows 2 rptr[b] .. 2 rptr[b+1] of every pair over the lists tptr / tedge; arg / cnt as hpv_forward wrote them
int hpv_backward(const float* g, int64_t ldg, int64_t g_rows, int32_t C, const int64_t* rptr, int32_t B, int32_t k,
                 const int64_t* tptr, const int64_t* tedge, const float* rmat, int32_t mode, const uint8_t* arg, int64_t ldarg,
                 int32_t word, const uint8_t* cnt, int32_t vec, float* dv, int64_t ldv) {
    if (k < 1 || k > dcinterp::MAX_K || !dcvpool::mode_ok(mode)) return -1;
    const dcconn::R4* R = reinterpret_cast<const dcconn::R4*>(rmat);
    for (int b = 0; b < B; ++b)
        for (int64_t r = rptr[b]; r < rptr[b + 1]; ++r)
            for (int c0 = 0; c0 < C; c0 += 4) {
                const int nc = C - c0 < 4 ? C - c0 : 4;
                const int64_t* list = tedge + tptr[r];
                const long long n = tptr[r + 1] - tptr[r];
                const bool v16 = vec && nc == 4, w4 = word && nc == 4;
                float u[4], w[4];
                if (mode == dcvpool::MODE_MAX)
                    dcvpool::bwd4<dcvpool::MODE_MAX>(g, ldg, g_rows, k, list, R, n, arg, ldarg, cnt, c0, nc, v16, w4, u, w);
                else if (mode == dcvpool::MODE_SUM)
                    dcvpool::bwd4<dcvpool::MODE_SUM>(g, ldg, g_rows, k, list, R, n, arg, ldarg, cnt, c0, nc, v16, w4, u, w);
                else
                    dcvpool::bwd4<dcvpool::MODE_MEAN>(g, ldg, g_rows, k, list, R, n, arg, ldarg, cnt, c0, nc, v16, w4, u, w);
                for (int c = 0; c < nc; ++c) {
                    dv[(2 * r) * ldv + c0 + c] = u[c];
                    dv[(2 * r + 1) * ldv + c0 + c] = w[c];
                }
            }
    return 0;
}

}  // extern "C"
