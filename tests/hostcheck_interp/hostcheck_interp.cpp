// g++ build of deltaconv_amd/csrc/interp_math.h -- the per-thread code of the two-set nearest-neighbour search and of the
// inverse-squared-distance interpolation (interp.hip), looped over queries / channel groups on the CPU
// (tests/test_interp_host.py).
#include <stdint.h>

#include "../../deltaconv_amd/csrc/interp_math.h"

namespace {

template <int K>
void search(const float* query, int64_t nq, const float* ref, int64_t nr, int32_t k, int32_t* idx, float* d2) {
    for (int64_t q = 0; q < nq; ++q) {
        dcinterp::TopK<K> best;
        best.init();
        for (int64_t c = 0; c < nr; ++c)
            best.push(dcinterp::dist2(query[3 * q], query[3 * q + 1], query[3 * q + 2], ref[3 * c], ref[3 * c + 1], ref[3 * c + 2]),
                      (int)c);
        for (int s = 0; s < k; ++s) {
            idx[q * k + s] = best.id[s];
            d2[q * k + s] = best.d[s];
        }
    }
}

}  // namespace

extern "C" {

// one cloud pair: query [nq,3], ref [nr,3] -> idx [nq,k], d2 [nq,k]; K by the dispatch of dc_knn_cross.  -> 0, or -1 for a k outside
// 1 .. 16
int hi_knn_cross(const float* query, int64_t nq, const float* ref, int64_t nr, int32_t k, int32_t* idx, float* d2) {
    if (k < 1 || k > dcinterp::MAX_K) return -1;
    if (k == 1) search<1>(query, nq, ref, nr, k, idx, d2);
    else if (k <= 4) search<4>(query, nq, ref, nr, k, idx, d2);
    else if (k <= 8) search<8>(query, nq, ref, nr, k, idx, d2);
    else search<16>(query, nq, ref, nr, k, idx, d2);
    return 0;
}

// one cloud pair: x [nr,ldx] -> out [nq,ldo], C channels in groups of 4 as the kernel's threads take them; vec: 16-byte loads for
// whole groups (x 16-byte aligned, ldx a multiple of 4)
void hi_interpolate(const float* x, int64_t ldx, int32_t C, int64_t nr, int64_t nq, int32_t k, const int32_t* idx, const float* d2,
                    int32_t vec, float* out, int64_t ldo) {
    for (int64_t q = 0; q < nq; ++q)
        for (int c0 = 0; c0 < C; c0 += 4) {
            const int nc = C - c0 < 4 ? C - c0 : 4;
            float v[4];
            dcinterp::interp4(x, ldx, nr, k, idx + q * k, d2 + q * k, c0, nc, vec && nc == 4, v);
            for (int c = 0; c < nc; ++c) out[q * ldo + c0 + c] = v[c];
        }
}

}  // extern "C"
