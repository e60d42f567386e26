// g++ build of the backward functions of deltaconv_amd/csrc/interp_math.h (coef / pair_of / pick / bwd4) -- the per-thread code
// of dc_knn_cross_transpose and dc_knn_interpolate_backward (interp.hip), looped over slots / reference rows / channel groups on
// the CPU (tests/test_interp_grad_host.py).  Built without contraction, as the library is.
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/interp_math.h"

extern "C" {

// one cloud pair: idx / d2 [nq,k] -> coef [nq,k] (0 for an invalid slot)
void hg_coef(int64_t nq, int64_t nr, int32_t k, const int32_t* idx, const float* d2, float* coef) {
    for (int64_t q = 0; q < nq; ++q)
        for (int s = 0; s < k; ++s) coef[q * k + s] = dcinterp::coef(nr, k, idx + q * k, d2 + q * k, s);
}

// the lists of a call: the slots are visited by ascending edge id, so every list comes out ascending.  -> the number of in-edges, or
// -1 for a k outside 1 .. 16
int64_t hg_transpose(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t num_ref, int32_t k,
                     const int32_t* idx, const float* d2, int64_t* tptr, int64_t* tedge, float* tcoef) {
    if (k < 1 || k > dcinterp::MAX_K) return -1;
    const int64_t ne = num_query * k;
    std::vector<int64_t> cursor(num_ref + 1, 0);
    for (int64_t e = 0; e < ne; ++e) {
        const long long r = dcinterp::pick(qptr, rptr, B, k, idx, e);
        if (r >= 0 && r < num_ref) ++cursor[r];
    }
    int64_t run = 0;
    for (int64_t r = 0; r < num_ref; ++r) {
        const int64_t c = cursor[r];
        tptr[r] = cursor[r] = run;
        run += c;
    }
    tptr[num_ref] = run;
    for (int64_t e = 0; e < ne; ++e) {
        const long long r = dcinterp::pick(qptr, rptr, B, k, idx, e);
        if (r < 0 || r >= num_ref) continue;
        const int64_t q = e / k;
        const int b = dcinterp::pair_of(qptr, B, q);
        tedge[cursor[r]] = e;
        tcoef[cursor[r]++] = dcinterp::coef(rptr[b + 1] - rptr[b], k, idx + q * k, d2 + q * k, (int)(e - q * k));
    }
    return run;
}

// g [g_rows,ldg] -> dx rows rptr[b] .. rptr[b+1] of every pair, C channels in groups of 4 as the kernel's threads take them; vec:
// 16-byte loads for whole groups (g 16-byte aligned, ldg a multiple of 4)
void hg_backward(const float* g, int64_t ldg, int64_t g_rows, int32_t C, const int64_t* rptr, int32_t B, int32_t k,
                 const int64_t* tptr, const int64_t* tedge, const float* tcoef, int64_t edge_base, int32_t vec, float* dx,
                 int64_t ldx) {
    for (int b = 0; b < B; ++b)
        for (int64_t r = rptr[b]; r < rptr[b + 1]; ++r)
            for (int c0 = 0; c0 < C; c0 += 4) {
                const int nc = C - c0 < 4 ? C - c0 : 4;
                float v[4];
                dcinterp::bwd4(g, ldg, g_rows, k, edge_base, tedge + tptr[r], tcoef + tptr[r], tptr[r + 1] - tptr[r], c0, nc,
                               vec && nc == 4, v);
                for (int c = 0; c < nc; ++c) dx[r * ldx + c0 + c] = v[c];
            }
}

}  // extern "C"
