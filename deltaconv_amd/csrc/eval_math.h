// Per-row and per-cloud arithmetic of the evaluation-metric kernel (eval.hip), shared with the g++ host-check build
// (tests/hostcheck_eval) like batch_math.h / nn_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// Reference being restated: /root/reference/experiments/utils.py:27-51 (calc_shape_IoU) and test_shapenet.py:84-103
// (np.argmax over the summed logits, per-shape part IoU) --
//   arg-max   numpy's rule: the FIRST index of the row maximum; a NaN counts as the maximum and the first NaN wins
//   IoU       per part: I = #(pred == part and y == part), U = #(pred == part or y == part), U == 0 ? 1 : I / U in fp64;
//             per shape: the mean over the shape's parts, summed in part order in fp64
// The counts are integers: with cnt[c] = #(y == c), npred[c] = #(pred == c) and hit[c] = #(pred == c and y == c),
// I = hit[c] and U = cnt[c] + npred[c] - hit[c].
#pragma once
#include "point_math.h"

namespace dceval {

constexpr int MAX_P = 256;                    // classes per row the kernel takes (LDS counters, rows of a slab)

// One step of a row scan, columns in ascending order.  State: (best, idx); start with best = row[0], idx = 0 and feed
// columns 1 .. P-1.  A NaN once taken is never replaced (v > NaN and NaN > v are both false, the explicit test keeps the first).
DC_HD void argmax_step(float& best, int& idx, float v, int c) {
    const bool best_nan = best != best;
    if (!best_nan && (v != v || v > best)) {
        best = v;
        idx = c;
    }
}

DC_HD int argmax_row(const float* row, int P, long stride = 1) {
    float best = row[0];
    int idx = 0;
    for (int c = 1; c < P; ++c) argmax_step(best, idx, row[(long)c * stride], c);
    return idx;
}

// mean over the parts start .. start + count - 1 of (U == 0 ? 1 : I / U).  A part outside [0, P) is in no row (predictions lie
// in [0, P), labels outside it are ignored): its union is empty, it counts as 1 and indexes nothing -- the parts below 0 and the
// parts from P on enter as one term each, so the loop is at most P long whatever the tables hold.  count <= 0: the mean of
// nothing, NaN, as numpy has it.
DC_HD double iou_fold(const int* hit, const int* cnt, const int* npred, int P, int start, int count) {
    if (count <= 0) return __builtin_nan("");
    const long lo = start, hi = (long)start + count;                 // parts [lo, hi)
    const long a = lo < 0 ? 0 : (lo > P ? (long)P : lo), b = hi < 0 ? 0 : (hi > P ? (long)P : hi);    // those inside [0, P)
    const long before = lo < 0 ? (hi < 0 ? hi : 0) - lo : 0, after = count - (b - a) - before;
    double sum = (double)before;
    for (long part = a; part < b; ++part) {
        const int i = hit[part], u = cnt[part] + npred[part] - hit[part];
        sum += u == 0 ? 1.0 : (double)i / (double)u;
    }
    sum += (double)after;
    return sum / (double)count;
}

}  // namespace dceval
