// g++ build of deltaconv_amd/csrc/eval_math.h -- the row arg-max and the per-cloud IoU fold of the evaluation-metric kernel
// (eval.hip), looped over rows / clouds on the CPU the way the kernel's workgroups do (tests/test_eval_host.py).
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/eval_math.h"

extern "C" {

int he_max_p() { return dceval::MAX_P; }

// out [R]: the arg-max of every row of rows [R, P] (row stride ld)
void he_argmax(const float* rows, int64_t R, int P, int64_t ld, int64_t* out) {
    for (int64_t r = 0; r < R; ++r) out[r] = dceval::argmax_row(rows + r * ld, P);
}

// One cloud from its predictions and labels: the three integer counters, then the fold over parts start .. start + count - 1.
// hit / cnt [P] and ignored [1] are written as the kernel writes them.
double he_cloud_iou(const int64_t* pred, const int64_t* y, int64_t n, int P, int start, int count, int32_t* hit, int32_t* cnt,
                    int32_t* ignored) {
    std::vector<int> h(P, 0), c(P, 0), np(P, 0);
    int ign = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int idx = (int)pred[r];
        ++np[idx];
        if (y[r] >= 0 && y[r] < P) {
            ++c[y[r]];
            if (y[r] == idx) ++h[y[r]];
        } else {
            ++ign;
        }
    }
    for (int k = 0; k < P; ++k) { hit[k] = h[k]; cnt[k] = c[k]; }
    *ignored = ign;
    return dceval::iou_fold(h.data(), c.data(), np.data(), P, start, count);
}

}  // extern "C"
