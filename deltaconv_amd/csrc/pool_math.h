// Arithmetic of the cross-cloud pooling of scalar features (pool.hip), shared with the g++ host-check build
// (tests/hostcheck_pool) like interp_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// What is being restated: a torch_cluster.knn(x_fine, x_coarse, k) search followed by torch_scatter.scatter(x[col], row,
// reduce="max" | "min" | "sum" | "mean") -- the set-abstraction step of PointNet++: every point of a sampled cloud takes the
// maximum, minimum, sum or mean over its k nearest points of the full cloud.  The reference has no such call site; its
// multi-resolution use (GeodesicFPS, train_shapenet.py:32) is what the op is for.  The gradient is w.r.t. the FEATURES x only.
//
// Every rule is fixed so that a numpy restatement (tests/pool_restate.py) reproduces the bits:
//   valid     slot s of query q is valid iff 0 <= idx[q,s] < nr (dcinterp::valid_slot); an invalid slot is skipped, nothing is indexed
//   mode      0 max, 1 min, 2 sum, 3 mean: the codes of dc_seg_reduce
//   start     acc = the value of the FIRST valid slot, copied bit for bit, arg = that slot (k = 1 is an exact gather in every mode)
//   max/min   a later valid slot replaces acc iff v > acc (max) / v < acc (min), and arg with it: strict, so ties keep the earlier
//             (nearer) slot; a NaN in a later slot compares false and is never taken, a NaN in the first valid slot stays -- the rule
//             of seg_reduce_kernel (edge.hip).  arg is the slot number 0 .. k-1, per channel
//   sum       the later valid slots in order, acc = acc + v, every addition rounded on its own (dcinterp::add_rn)
//   mean      the sum, then ONE division acc / (float)cnt
//   cnt       the number of valid slots of the query, one uint8 per query row, in every mode
//   no slot   a query without a valid slot gets a row of zeros, arg = 255, cnt = 0
//
// The backward w.r.t. x (tests/pool_restate.py restates it; dc_knn_pool_backward runs it) on the lists of dc_knn_cross_transpose:
//   in-edges  of reference row j: every valid (q, s) of its cloud pair with idx[q, s] == j, named e = q * k + s, in ASCENDING e
//   term      of edge e for channel ch: max / min: g[q, ch] if arg[q, ch] == s, otherwise the edge adds NOTHING (no + 0);
//             sum: g[q, ch]; mean: g[q, ch] / (float)cnt[q], the division rounded on its own
//   sum       dx[j, ch] = 0, then for every in-edge in that order dx = dx + term (add_rn); an edge whose query row falls outside
//             [0, rows of g) is skipped; a row without in-edges gets zeros.  No atomics: a function of the inputs only
#pragma once
#include <stdint.h>

#include "interp_math.h"

namespace dcpool {

constexpr int MODE_MAX = 0, MODE_MIN = 1, MODE_SUM = 2, MODE_MEAN = 3;
constexpr unsigned char NO_ARG = 255;         // arg of a query without a valid slot

using dcinterp::add_rn;
using dcinterp::load4;
using dcinterp::valid_slot;

// Channels c0 .. c0+nc-1 (nc in 1 .. 4) of one query: x [Nr, ldx] the rows of ITS reference cloud, idx [k] its slots.  vec: x + c0
// is 16-byte aligned in every row and nc = 4.  out [4] receives nc values, arg [4] the slot each came from (max / min; 255 without a
// valid slot, and in the other modes, which have no arg to store).  -> cnt, the number of valid slots.
DC_HD int fwd4(const float* x, long long ldx, long long nr, int k, const int* idx, int mode, int c0, int nc, bool vec, float* out,
               unsigned char* arg) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int at[4] = {NO_ARG, NO_ARG, NO_ARG, NO_ARG};
    int cnt = 0;
    for (int s = 0; s < k; ++s) {
        const long long j = idx[s];
        if (!valid_slot(j, nr)) continue;
        float r[4];
        load4(x + j * ldx + c0, nc, vec, r);
        const bool first = cnt == 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (mode <= MODE_MIN) {
                const bool take = first || (mode == MODE_MAX ? r[c] > acc[c] : r[c] < acc[c]);
                acc[c] = take ? r[c] : acc[c];
                at[c] = take ? s : at[c];
            } else {
                acc[c] = first ? r[c] : add_rn(acc[c], r[c]);
            }
        }
        ++cnt;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        out[c] = mode == MODE_MEAN && cnt > 0 ? acc[c] / (float)cnt : acc[c];
        arg[c] = (unsigned char)at[c];
    }
    return cnt;
}

// The four slot numbers of a channel group, one 32-bit access when word: p is 4-byte aligned and all four are there.
DC_HD void store_arg4(unsigned char* p, const unsigned char* a, int nc, bool word) {
    if (word) {
        const uint32_t w = (uint32_t)a[0] | (uint32_t)a[1] << 8 | (uint32_t)a[2] << 16 | (uint32_t)a[3] << 24;
        __builtin_memcpy(__builtin_assume_aligned(p, 4), &w, 4);
    } else {
        for (int c = 0; c < nc; ++c) p[c] = a[c];
    }
}
// -> the four slot numbers packed as store_arg4 packs them, 255 where a channel is not there.
DC_HD uint32_t load_arg4(const unsigned char* p, int nc, bool word) {
    uint32_t w = 0xffffffffu;
    if (word) {
        __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
    } else {
        for (int c = 0; c < nc; ++c) w = (w & ~(255u << 8 * c)) | (uint32_t)p[c] << 8 * c;
    }
    return w;
}

// Channels c0 .. c0+nc-1 of one reference row's gradient: its in-edges tedge [n] in ascending order, g [rows, ldg] the gradient of
// the call's query rows, arg [rows, ldarg] / cnt [rows] what the forward wrote for them (arg is read by max / min only, cnt by
// mean only).  Query row of edge e = e / k, slot e - row * k; an edge whose row falls outside [0, rows) is skipped (lists that do
// not belong to g).  vec: g + c0 is 16-byte aligned in every row and nc = 4; word: arg + c0 is 4-byte aligned in every row and
// nc = 4.  out [4] receives nc values.  MODE at compile time (max and min are the same walk: instantiate MODE_MAX for both): with a
// run-time mode the unrolled body holds all three forms at once, 111 VGPRs against the 65 of dcinterp::bwd4's kernel.
template <int MODE>
DC_HD void bwd4(const float* g, long long ldg, long long rows, int k, const int64_t* tedge, long long n, const unsigned char* arg,
                long long ldarg, const unsigned char* cnt, int c0, int nc, bool vec, bool word, float* out) {
    constexpr int mode = MODE;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;                      // in-edges whose loads fly together; the sum itself stays in list order
    for (long long t0 = 0; rows > 0 && t0 < n; t0 += U) {
        float r[U][4], div[U];
        uint32_t a[U], slot[U];              // four slot numbers a word: the forward's, and the edge's own in every byte
        bool in[U];
        long long row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long t = t0 + u < n ? t0 + u : n - 1;             // (clamped: an unconditional load, masked below)
            const long long e = tedge[t];
            const long long q = e >> 32 ? e / k : (long long)((unsigned)e / (unsigned)k);
            in[u] = t0 + u < n && q >= 0 && q < rows;
            slot[u] = (uint32_t)(e - q * k) * 0x01010101u;
            row[u] = in[u] ? q : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load4(g + row[u] * ldg + c0, nc, vec, r[u]);
            a[u] = mode <= MODE_MIN ? load_arg4(arg + row[u] * ldarg + c0, nc, word) : slot[u];   // sum / mean: every in-edge counts
            div[u] = mode == MODE_MEAN ? (float)cnt[row[u]] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const bool hit = in[u] && (((a[u] ^ slot[u]) >> 8 * ch) & 255u) == 0;
                const float term = mode == MODE_MEAN ? r[u][ch] / div[u] : r[u][ch];
                acc[ch] = hit ? add_rn(acc[ch], term) : acc[ch];
            }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) out[ch] = acc[ch];
}

}  // namespace dcpool
