// Arithmetic of the pooling over the cells of a cluster vector (cluster.hip), shared with the g++ host-check build
// (tests/hostcheck_cluster) like pool_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// What is being restated: torch_geometric's voxel_grid followed by max_pool / avg_pool_x / pool_pos, that is
// torch_scatter.scatter(x, cluster, reduce="max" | "min" | "sum" | "mean") over ANY cluster vector (dc_voxel_subsample's, or the
// caller's), with the barycentres and the majority labels of the cells.  The gradient is w.r.t. the FEATURES only.
//
// Every rule is fixed so that a numpy restatement (tests/cluster_restate.py) reproduces the bits:
//   cell      row i belongs to cell cluster[i] iff 0 <= cluster[i] < M (in_cell); any other value, -1 included, names no cell
//   lists     the members of cell j are its rows in ASCENDING order: members[cptr[j] .. cptr[j+1]); rank_of gives a row's place
//             (the number of smaller rows in its list, in whatever order the fill left them)
//   mode      0 max, 1 min, 2 sum, 3 mean: the codes of dc_seg_reduce
//   start     acc = the value of the FIRST member, copied bit for bit, arg = that row (a cell of one row is an exact gather)
//   max/min   a later member replaces acc iff v > acc (max) / v < acc (min), and arg with it: strict, so ties keep the LOWER row
//             (+0.0 against -0.0 is a tie); a later NaN compares false and is never taken, a first NaN stays -- the rule of
//             pool_math.h.  arg is the ROW of x, int32, per channel
//   sum       the later members in order, acc = acc + v, every addition rounded on its own (dcinterp::add_rn)
//   mean      the sum, then ONE division acc / (float)cnt
//   empty     a cell without a member gets zeros, arg = -1
//   foreign   a member outside [0, rows of x) is skipped and not counted (lists that do not belong to x; dc_cluster_lists makes none)
// The backward w.r.t. x is a gather, every point belongs to one cell: max / min: dx[i,c] = arg[cl,c] == i ? g[cl,c] : 0; sum:
// g[cl,c]; mean: g[cl,c] / (float)(cptr[cl+1] - cptr[cl]), the quotient rounded on its own (the term of dcpool::bwd4); a point
// without a cell gets zeros.  The un-pooling out[i] = x[cluster[i]] IS the sum-mode backward, and its own backward the sum-mode
// forward over the lists: an ordered, atomics-free index_add_.
//   mean3     [N,3] rows (positions, normals): per cell an fp64 sum in member order, ONE fp64 division by the count, ONE rounding
//             to fp32.  normalize: the fp64 sum divided by its fp64 norm sqrt((sx*sx + sy*sy) + sz*sz) instead; zeros where that
//             norm is zero or not finite.  (An fp32 chain loses the low bits of a cloud shifted by 4 096.)
//   majority  per cell the label in [0, num_classes) with the most members, ties to the LOWEST label; labels outside the range
//             are ignored; -1 for a cell without a valid label.  Integer counting only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pool_math.h"

namespace dccl {

using dcpool::MODE_MAX;
using dcpool::MODE_MEAN;
using dcpool::MODE_MIN;
using dcpool::MODE_SUM;
using dcinterp::add_rn;
using dcinterp::load4;

constexpr long long MAX_ROWS = 0x7fffffffll;  // arg holds rows of x as int32
constexpr int MAX_CLASSES = 1024;
constexpr int NO_ARG = -1;

DC_HD bool in_cell(long long c, long long m) { return c >= 0 && c < m; }

// The place of row e in its list: how many of the list's entries unordered[lo .. hi) are smaller (they are pairwise distinct).
DC_HD long long rank_of(const int64_t* unordered, long long lo, long long hi, long long e) {
    long long rank = 0;
#pragma unroll 8
    for (long long p = lo; p < hi; ++p) rank += unordered[p] < e;
    return rank;
}

// Channels c0 .. c0+nc-1 (nc in 1 .. 4) of one cell: x [rows, ldx], mem [n] its members in ascending order.  vec: x + c0 is
// 16-byte aligned in every row and nc = 4.  out [4] receives nc values, arg [4] the row each came from (max / min; -1 for an
// empty cell and in the other modes).  -> the number of members taken.
DC_HD long long fwd4(const float* x, long long ldx, long long rows, const int64_t* mem, long long n, int mode, int c0, int nc,
                     bool vec, float* out, int* arg) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int at[4] = {NO_ARG, NO_ARG, NO_ARG, NO_ARG};
    long long cnt = 0;
    constexpr int U = 4;                      // members whose loads fly together; the walk itself stays in list order
    for (long long t0 = 0; t0 < n; t0 += U) {
        float r[U][4];
        long long row[U];
        bool in[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long j = mem[t0 + u < n ? t0 + u : n - 1];            // (clamped: an unconditional load, masked below)
            in[u] = t0 + u < n && j >= 0 && j < rows;
            row[u] = in[u] ? j : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (rows > 0) load4(x + row[u] * ldx + c0, nc, vec, r[u]);
            else r[u][0] = r[u][1] = r[u][2] = r[u][3] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!in[u]) continue;
            const bool first = cnt == 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (mode <= MODE_MIN) {
                    const bool take = first || (mode == MODE_MAX ? r[u][c] > acc[c] : r[u][c] < acc[c]);
                    acc[c] = take ? r[u][c] : acc[c];
                    at[c] = take ? (int)row[u] : at[c];
                } else {
                    acc[c] = first ? r[u][c] : add_rn(acc[c], r[u][c]);
                }
            }
            ++cnt;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        out[c] = mode == MODE_MEAN && cnt > 0 ? acc[c] / (float)cnt : acc[c];
        arg[c] = mode <= MODE_MIN ? at[c] : NO_ARG;
    }
    return cnt;
}

// Channels c0 .. c0+nc-1 of the gradient of point `row`, cl its cluster id: g [M, ldg] the gradient of the pooled rows, arg
// [M, ldarg] what the forward wrote (max / min only), cptr [M+1] (mean only).  vec: g + c0 is 16-byte aligned in every row and
// nc = 4.  Mode MODE_SUM is also the un-pooling out[row] = x[cl].
DC_HD void bwd4(const float* g, long long ldg, long long m, long long cl, long long row, const int64_t* cptr, const int32_t* arg,
                long long ldarg, int mode, int c0, int nc, bool vec, float* out) {
    out[0] = out[1] = out[2] = out[3] = 0.f;
    if (!in_cell(cl, m)) return;
    float r[4];
    load4(g + cl * ldg + c0, nc, vec, r);
    if (mode <= MODE_MIN) {
        for (int c = 0; c < nc; ++c) out[c] = (long long)arg[cl * ldarg + c0 + c] == row ? r[c] : 0.f;
    } else if (mode == MODE_SUM) {
        for (int c = 0; c < nc; ++c) out[c] = r[c];
    } else {
        const float div = (float)(cptr[cl + 1] - cptr[cl]);
        for (int c = 0; c < nc; ++c) out[c] = r[c] / div;
    }
}

// One cell of dc_cluster_mean3: p [rows,3], mem [n] -> out [3].
DC_HD void mean3(const float* p, long long rows, const int64_t* mem, long long n, int normalize, float* out) {
    double s[3] = {0.0, 0.0, 0.0};
    long long cnt = 0;
    for (long long t = 0; t < n; ++t) {
        const long long j = mem[t];
        if (j < 0 || j >= rows) continue;
        s[0] = s[0] + (double)p[3 * j];
        s[1] = s[1] + (double)p[3 * j + 1];
        s[2] = s[2] + (double)p[3 * j + 2];
        ++cnt;
    }
    out[0] = out[1] = out[2] = 0.f;
    if (cnt == 0) return;
    double div = (double)cnt;
    if (normalize) {
        const double xx = s[0] * s[0], yy = s[1] * s[1], zz = s[2] * s[2];
        const double q = xx + yy;
        div = sqrt(q + zz);
        if (!(div > 0.0) || !(div < (double)__builtin_huge_val())) return;     // zero, NaN or infinite: zeros
    }
    for (int a = 0; a < 3; ++a) out[a] = (float)(s[a] / div);
}

// One cell of dc_cluster_majority: labels [rows], mem [n] -> the label, or -1.  The classes between the smallest and the largest
// valid label of the cell are counted one by one: classes x members integer compares, no table.
DC_HD long long majority(const int64_t* labels, long long rows, const int64_t* mem, long long n, int num_classes) {
    long long lo = num_classes, hi = -1;
    for (long long t = 0; t < n; ++t) {
        const long long j = mem[t];
        if (j < 0 || j >= rows) continue;
        const long long l = labels[j];
        if (l < 0 || l >= num_classes) continue;
        lo = l < lo ? l : lo;
        hi = l > hi ? l : hi;
    }
    long long best = -1, most = 0;
    for (long long c = lo; c <= hi; ++c) {
        long long cnt = 0;
        for (long long t = 0; t < n; ++t) {
            const long long j = mem[t];
            cnt += (j >= 0 && j < rows && labels[j] == c) ? 1 : 0;
        }
        if (cnt > most) {                     // strict: a tie keeps the lower label
            most = cnt;
            best = c;
        }
    }
    return best;
}

}  // namespace dccl
