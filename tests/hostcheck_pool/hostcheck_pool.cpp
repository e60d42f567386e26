// g++ build of deltaconv_amd/csrc/pool_math.h (fwd4 / store_arg4 / load_arg4 / bwd4) -- the per-thread code of dc_knn_pool and
// dc_knn_pool_backward (pool.hip), looped over cloud pairs / rows / channel groups on the CPU as the frame of cross_stage.h loops
// them (tests/test_pool_host.py).  Built without contraction, as the library is.
#include <stdint.h>

#include "../../deltaconv_amd/csrc/pool_math.h"

extern "C" {

// x [*,ldx] -> out [*,ldo], arg [*,ldarg] (max / min only), cnt [*] over the query rows of every pair.  vec: 16-byte loads for whole
// groups (x 16-byte aligned, ldx a multiple of 4); word: one 32-bit store of the slot numbers for whole groups (arg 4-byte aligned,
// ldarg a multiple of 4).  -> 0, or -1 for a k outside 1 .. 16 or a mode outside 0 .. 3
int hp_forward(const float* x, int64_t ldx, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B, int32_t k,
               const int32_t* idx, int32_t mode, int32_t vec, float* out, int64_t ldo, uint8_t* arg, int64_t ldarg, int32_t word,
               uint8_t* cnt) {
    if (k < 1 || k > dcinterp::MAX_K || mode < 0 || mode > 3) return -1;
    for (int b = 0; b < B; ++b) {
        const long long nr = rptr[b + 1] - rptr[b];
        for (int64_t row = qptr[b]; row < qptr[b + 1]; ++row)
            for (int c0 = 0; c0 < C; c0 += 4) {
                const int nc = C - c0 < 4 ? C - c0 : 4;
                float v[4];
                unsigned char a[4];
                const int n = dcpool::fwd4(x + rptr[b] * ldx, ldx, nr < 0 ? 0 : nr, k, idx + row * k, mode, c0, nc, vec && nc == 4, v, a);
                for (int c = 0; c < nc; ++c) out[row * ldo + c0 + c] = v[c];
                if (arg && mode <= dcpool::MODE_MIN) dcpool::store_arg4(arg + row * ldarg + c0, a, nc, word && nc == 4);
                if (c0 == 0) cnt[row] = (unsigned char)n;
            }
    }
    return 0;
}

// g [g_rows,ldg] -> dx rows rptr[b] .. rptr[b+1] of every pair over the lists tptr / tedge; arg / cnt as hp_forward wrote them
int hp_backward(const float* g, int64_t ldg, int64_t g_rows, int32_t C, const int64_t* rptr, int32_t B, int32_t k,
                const int64_t* tptr, const int64_t* tedge, int32_t mode, const uint8_t* arg, int64_t ldarg, int32_t word,
                const uint8_t* cnt, int32_t vec, float* dx, int64_t ldx) {
    if (k < 1 || k > dcinterp::MAX_K || mode < 0 || mode > 3) return -1;
    for (int b = 0; b < B; ++b)
        for (int64_t r = rptr[b]; r < rptr[b + 1]; ++r)
            for (int c0 = 0; c0 < C; c0 += 4) {
                const int nc = C - c0 < 4 ? C - c0 : 4;
                const int64_t* list = tedge + tptr[r];
                const long long n = tptr[r + 1] - tptr[r];
                const bool v16 = vec && nc == 4, w4 = word && nc == 4;
                float v[4];
                if (mode <= dcpool::MODE_MIN) dcpool::bwd4<dcpool::MODE_MAX>(g, ldg, g_rows, k, list, n, arg, ldarg, cnt, c0, nc, v16, w4, v);
                else if (mode == dcpool::MODE_SUM) dcpool::bwd4<dcpool::MODE_SUM>(g, ldg, g_rows, k, list, n, arg, ldarg, cnt, c0, nc, v16, w4, v);
                else dcpool::bwd4<dcpool::MODE_MEAN>(g, ldg, g_rows, k, list, n, arg, ldarg, cnt, c0, nc, v16, w4, v);
                for (int c = 0; c < nc; ++c) dx[r * ldx + c0 + c] = v[c];
            }
    return 0;
}

}  // extern "C"
