// The rules of Euclidean farthest-point sampling (fps_euclid.hip: dc_fps_batch), shared with the g++ host-check build
// (tests/hostcheck_fps_euclid) like knn_grid_math.h / fps_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// One cloud of n points samples m <= n picks from start row s (an id local to the cloud).  Every rule is fixed so that a numpy
// restatement (tests/fps_euclid_restate.py) reproduces the picks exactly:
//   distance   d2(p, c) = dcinterp::dist2: fp32, dx = p - c per axis, (dx*dx + dy*dy) + dz*dz, every operation rounded on its own
//              (no contraction: -ffp-contract=off, and __fmul_rn / __fadd_rn on the device)
//   state      one fp32 key md per point.  A point with a non-finite coordinate starts at NONFINITE = -0.5, every other point at
//              +inf.  A picked point is set to PICKED = -1.  (The kernel's padding slots past the cloud hold PAD = -2.)
//   update     after a pick c every point with md >= 0 takes md = d2 if d2 < md.  A NaN d2 compares false and lowers nothing; a
//              marked (-1) or non-finite (-0.5) point is never touched.
//   selection  the next pick is the FIRST index (lowest local id) of max(md).  As one unsigned maximum: key = (image(md) << 32) |
//              (0xFFFFFFFF - id), image() the usual order-preserving map of fp32 bit patterns onto unsigned integers (md is never
//              NaN and never -0: it is +inf, a negative constant, or a rounded sum of squares).
// Consequences:
//   * The picks are pairwise distinct for m <= n: a picked point holds -1, below every unpicked point (>= -0.5), and while fewer
//     than n points are picked an unpicked one exists.
//   * Non-finite points are picked only after every finite one, in ascending id: a finite unpicked point holds md >= 0 > -0.5,
//     and the non-finite ones all hold the same -0.5, so the lowest id wins.
//   * A non-finite start is allowed: its distances are NaN or +inf and lower nothing; the next pick is the first finite point.
//   * Greedy: the first m' picks of an m-pick sample are the m'-pick sample from the same start.
//   * If a cloud is re-ordered so that its first m rows are the picks in pick order, sampling it from row 0 returns 0, 1, .., m-1:
//     md after r picks is the same function of the same points, max(md) is the same number, and among the points that attain it
//     the original pick is now row r -- every row below r is marked, so it is the first index.  (A tie that the original order
//     broke towards another point cannot occur: that point WAS the original pick.)  This is what geometry.prefix_levels rests on.
//
// fp64 bound.  Take the fp32 inputs as exact reals and u = 2^-24.  dx = fl(p - c) = (p - c)(1 + e1), |e1| <= u; fl(dx dx) =
// (p - c)^2 (1 + e1)^2 (1 + e2): at most 3u + O(u^2) per square; the two additions of non-negative terms add u each.  Hence
// |fl(d2) - d2| <= 5u d2 + O(u^2) (no underflow: a term below 2^-126 is absolute, not relative; no overflow).  A minimum and a
// maximum of numbers each within a relative 5u of their exact values are within 5u of the exact minimum / maximum, so with
// md64(i) = the exact minimum over the picks so far of d2(i, pick):
//   md64(pick_j) >= (1 - 5u) / (1 + 5u) * max_i md64(i) >= (1 - 12u) * max_i md64(i)      over the finite, unpicked points i
// (10u + O(u^2), and 2u of room for the fp64 evaluation of the right-hand side).  tests/test_fps_euclid_host.py asserts it.
#pragma once
#include <stdint.h>

#include "interp_math.h"

namespace dcfpse {

constexpr int MAX_POINTS = 16384;             // DC_FPS_EUCLID_MAX_POINTS: 16 points per thread x 1024 threads, all in registers
constexpr float PICKED = -1.0f, NONFINITE = -0.5f, PAD = -2.0f;

DC_HD float inf() { return __builtin_huge_valf(); }
DC_HD bool finite1(float x) { return fabsf(x) <= 3.4028234663852886e38f; }      // false for NaN and +-inf
DC_HD float init_md(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z) ? inf() : NONFINITE; }

// md after the pick at (cx, cy, cz); `picked`: this point IS the pick
DC_HD float update(float md, bool picked, float x, float y, float z, float cx, float cy, float cz) {
    const float d2 = dcinterp::dist2(x, y, z, cx, cy, cz);
    const float lowered = (md >= 0.f && d2 < md) ? d2 : md;
    return picked ? PICKED : lowered;
}

DC_HD uint32_t float_bits(float v) {
    union { float f; uint32_t u; } c;
    c.f = v;
    return c.u;
}
// order-preserving image of a non-NaN fp32 on the unsigned integers
DC_HD uint32_t image(float v) {
    const uint32_t b = float_bits(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// "largest md, then lowest id" as one unsigned maximum
DC_HD unsigned long long key(float md, int id) { return ((unsigned long long)image(md) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)id); }
DC_HD int key_id(unsigned long long k) { return (int)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull)); }

// a start outside its cloud is read as row 0 (the Python layer cannot check a device tensor without a synchronise)
DC_HD int clamp_start(int s, int n) { return (s < 0 || s >= n) ? 0 : s; }

// The whole sample of one cloud as plain loops: pos [n,3], md [n] scratch -> picks [m] local ids in pick order; a pick index
// r >= n gets -1.  The kernel runs the same update / key per point and the same maximum, spread over a workgroup.
inline void sample(const float* pos, int n, int m, int start, float* md, int32_t* picks) {
    for (int i = 0; i < n; ++i) md[i] = init_md(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
    int cur = n > 0 ? clamp_start(start, n) : 0;
    for (int r = 0; r < m; ++r) {
        if (r >= n) {
            picks[r] = -1;
            continue;
        }
        picks[r] = cur;
        const float cx = pos[3 * cur], cy = pos[3 * cur + 1], cz = pos[3 * cur + 2];
        unsigned long long best = 0ull;
        for (int i = 0; i < n; ++i) {
            md[i] = update(md[i], i == cur, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], cx, cy, cz);
            const unsigned long long k = key(md[i], i);
            best = k > best ? k : best;
        }
        cur = key_id(best);
    }
}

}  // namespace dcfpse
