// Pooling of per-point data over the cells of a cluster vector (dc_voxel_subsample's, or any int64 [N] with values in [0, M)):
// torch_geometric's voxel_grid + max_pool / avg_pool_x / pool_pos, torch_scatter.scatter(x, cluster, reduce=...) -- the linear-time
// way DOWN between resolutions, next to dc_knn_pool.  The arithmetic is csrc/cluster_math.h (shared with tests/hostcheck_cluster).
//
// dc_cluster_lists: the member lists, the project's usual build -- launch sizes from the HOST numbers (N rows, M cells) alone:
//   dc_zero_words        the counters [M]
//   cl_count_kernel      one thread per row: an integer atomicAdd on its cell's counter
//   list_sum / list_scan (list_scan.h)  exclusive scan over the cells: cptr [M+1], the counters become fill cursors
//   cl_fill_kernel       one thread per row: its place by an integer atomicAdd on the cursor -> the unordered lists
//   cl_rank_kernel       one thread per FILL POSITION (so a long list spreads over the grid, as transpose_rank_kernel in
//                        interp.hip): the row there counts the smaller rows of its list and writes itself at that rank; positions
//                        past cptr[M] get -1.  Quadratic in a list's length: a single cell holding all 262 144 rows of a call costs
//                        262 144 compares per thread -- long, not a hang.
// Only WHERE a row lands in the unordered list depends on the race, and the ranks do not depend on that: a function of the inputs.
//
// dc_cluster_pool           thread = (cell, group of 4 channels): the cell's members in list order, four rows in flight, 16-byte
//                           loads where x, ldx and C allow, scalar otherwise (any C >= 1)
// dc_cluster_pool_backward  thread = (point, group of 4 channels): a gather from the point's cell
// dc_cluster_gather         the un-pooling out[i] = x[cluster[i]]: the sum-mode backward kernel
// dc_cluster_mean3          thread = cell: fp64 barycentre / normalised mean of [N,3] rows
// dc_cluster_majority       thread = cell: the most frequent label
// Plain loads and stores, no floating-point atomics, no LDS: the outputs are a function of the inputs only.
#include "common.h"
#include "list_scan.h"
#include "cluster_math.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr long long CL_MAX_ITEMS = (long long)CL_THREADS * 0x7fffffffll;      // threads of one launch

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
size_t lists_bytes(long long n, long long m) {
    return up16(8 * ((size_t)m + (size_t)dc_cdiv(m, SC_THREADS) + (size_t)n)) + 16;
}

template <bool FILL>
__global__ __launch_bounds__(CL_THREADS) void cl_count_kernel(const int64_t* __restrict__ cluster, long long n, long long m,
                                                              u64* __restrict__ cnt, int64_t* __restrict__ unordered) {
    const long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long c = cluster[i];
    if (!dccl::in_cell(c, m)) return;
    const u64 at = atomicAdd(cnt + c, 1ull);
    if (FILL && at < (u64)n) unordered[at] = i;           // (always: the counts came from the same inputs)
}

__global__ __launch_bounds__(CL_THREADS) void cl_rank_kernel(const int64_t* __restrict__ cluster, long long n, long long m,
                                                             const int64_t* __restrict__ cptr,
                                                             const int64_t* __restrict__ unordered,
                                                             int64_t* __restrict__ members) {
    const long long t = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (t >= n) return;
    if (t >= cptr[m]) {
        members[t] = -1;
        return;
    }
    const long long e = unordered[t];
    if (e < 0 || e >= n) return;
    const long long c = cluster[e];
    if (!dccl::in_cell(c, m)) return;
    long long lo = cptr[c], hi = cptr[c + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const long long rank = dccl::rank_of(unordered, lo, hi, e);
    if (lo + rank >= hi) return;              // (never: e is one of the list's distinct entries)
    members[lo + rank] = e;
}

// [lo, hi) of cell j inside the n entries of members
__device__ __forceinline__ void cell_span(const int64_t* __restrict__ cptr, long long j, long long n, long long& lo, long long& len) {
    lo = cptr[j];
    long long hi = cptr[j + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    len = hi > lo ? hi - lo : 0;
}

__global__ __launch_bounds__(CL_THREADS) void cl_pool_kernel(const float* __restrict__ x, long long ldx, long long n, int C,
                                                             const int64_t* __restrict__ cptr,
                                                             const int64_t* __restrict__ members, long long m, int mode,
                                                             int vec_in, float* __restrict__ out, long long ldo, int vec_out,
                                                             int32_t* __restrict__ arg, long long ldarg, int vec_arg) {
    const int groups = (C + 3) >> 2;
    const long long t = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    const long long j = t / groups;
    if (j >= m) return;
    const int c0 = 4 * (int)(t - j * groups), nc = C - c0 < 4 ? C - c0 : 4;
    long long lo, len;
    cell_span(cptr, j, n, lo, len);
    float v[4];
    int a[4];
    dccl::fwd4(x, ldx, n, members + lo, len, mode, c0, nc, vec_in && nc == 4, v, a);
    float* o = out + j * ldo + c0;
    if (vec_out && nc == 4) {
        *reinterpret_cast<dc_f32x4*>(o) = dc_f32x4{v[0], v[1], v[2], v[3]};
    } else {
        for (int c = 0; c < nc; ++c) o[c] = v[c];
    }
    if (arg) {
        int32_t* p = arg + j * ldarg + c0;
        if (vec_arg && nc == 4) {
            *reinterpret_cast<int4*>(p) = make_int4(a[0], a[1], a[2], a[3]);
        } else {
            for (int c = 0; c < nc; ++c) p[c] = a[c];
        }
    }
}

__global__ __launch_bounds__(CL_THREADS) void cl_gather_kernel(const float* __restrict__ g, long long ldg, long long m, int C,
                                                               const int64_t* __restrict__ cluster, long long n,
                                                               const int64_t* __restrict__ cptr,
                                                               const int32_t* __restrict__ arg, long long ldarg, int mode,
                                                               int vec_in, float* __restrict__ dx, long long ldx, int vec_out) {
    const int groups = (C + 3) >> 2;
    const long long t = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    const long long i = t / groups;
    if (i >= n) return;
    const int c0 = 4 * (int)(t - i * groups), nc = C - c0 < 4 ? C - c0 : 4;
    float v[4];
    dccl::bwd4(g, ldg, m, cluster[i], i, cptr, arg, ldarg, mode, c0, nc, vec_in && nc == 4, v);
    float* o = dx + i * ldx + c0;
    if (vec_out && nc == 4) {
        *reinterpret_cast<dc_f32x4*>(o) = dc_f32x4{v[0], v[1], v[2], v[3]};
    } else {
        for (int c = 0; c < nc; ++c) o[c] = v[c];
    }
}

__global__ __launch_bounds__(CL_THREADS) void cl_mean3_kernel(const float* __restrict__ p, long long n,
                                                              const int64_t* __restrict__ cptr,
                                                              const int64_t* __restrict__ members, long long m, int normalize,
                                                              float* __restrict__ out) {
    const long long j = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (j >= m) return;
    long long lo, len;
    cell_span(cptr, j, n, lo, len);
    float v[3];
    dccl::mean3(p, n, members + lo, len, normalize, v);
    out[3 * j] = v[0];
    out[3 * j + 1] = v[1];
    out[3 * j + 2] = v[2];
}

__global__ __launch_bounds__(CL_THREADS) void cl_majority_kernel(const int64_t* __restrict__ labels, long long n,
                                                                 const int64_t* __restrict__ cptr,
                                                                 const int64_t* __restrict__ members, long long m,
                                                                 int num_classes, int64_t* __restrict__ out) {
    const long long j = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (j >= m) return;
    long long lo, len;
    cell_span(cptr, j, n, lo, len);
    out[j] = dccl::majority(labels, n, members + lo, len, num_classes);
}

inline int vec16(const void* p, long long ld) { return p && aligned_to(p, 16) && (ld & 3) == 0; }

// the checks the feature entry points share: sizes, and a [rows, C] fp32 operand with its leading dimension
bool sizes_ok(const char* fn, int64_t n, int64_t m, int32_t C) {
    if (n < 0 || n > dccl::MAX_ROWS) return dc_set_error("%s: num_points = %lld outside [0, 2^31)", fn, (long long)n), false;
    if (m < 0 || m > dccl::MAX_ROWS) return dc_set_error("%s: num_cells = %lld outside [0, 2^31)", fn, (long long)m), false;
    if (C < 1) return dc_set_error("%s: C = %d, at least one channel", fn, C), false;
    const long long groups = (C + 3) / 4;
    if ((n > m ? n : m) * groups > CL_MAX_ITEMS)
        return dc_set_error("%s: %lld rows of %d channels are more than one launch takes", fn, (long long)(n > m ? n : m), C), false;
    return true;
}

int launch_gather(const char* fn, const float* g, int64_t ldg, int64_t m, int32_t C, const int64_t* cluster, int64_t n,
                  const int64_t* cptr, const int32_t* arg, int64_t ldarg, int32_t mode, float* dx, int64_t ldx, void* stream) {
    if (!sizes_ok(fn, n, m, C)) return DC_ERR_ARG;
    DC_REQUIRE(ldg >= C && ldx >= C, "%s: leading dimensions (%lld, %lld) below C = %d", fn, (long long)ldg, (long long)ldx, C);
    if (n == 0) return DC_OK;
    DC_REQUIRE(cluster && dx && (m == 0 || g), "%s: null pointer (g, cluster, dx)", fn);
    const long long groups = (C + 3) / 4;
    hipLaunchKernelGGL(cl_gather_kernel, dim3(dc_cdiv(n * groups, CL_THREADS)), dim3(CL_THREADS), 0, static_cast<hipStream_t>(stream),
                       g, (long long)ldg, (long long)m, (int)C, cluster, (long long)n, cptr, arg, (long long)ldarg, (int)mode,
                       vec16(g, ldg), dx, (long long)ldx, vec16(dx, ldx));
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}

}  // namespace

DC_EXPORT size_t dc_cluster_lists_workspace_bytes(int64_t num_points, int64_t num_cells) {
    if (num_points < 0 || num_points > dccl::MAX_ROWS || num_cells < 0 || num_cells > dccl::MAX_ROWS) return 0;
    return lists_bytes(num_points, num_cells);
}

DC_EXPORT int dc_cluster_lists(const int64_t* cluster, int64_t num_points, int64_t num_cells, int64_t* cptr, int64_t* members,
                               void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "dc_cluster_lists";
    DC_REQUIRE(num_points >= 0 && num_points <= dccl::MAX_ROWS, "%s: num_points = %lld outside [0, 2^31)", fn, (long long)num_points);
    DC_REQUIRE(num_cells >= 0 && num_cells <= dccl::MAX_ROWS, "%s: num_cells = %lld outside [0, 2^31)", fn, (long long)num_cells);
    DC_REQUIRE(cptr, "%s: null pointer (cptr)", fn);
    DC_REQUIRE(num_points == 0 || (cluster && members), "%s: null pointer (cluster, members)", fn);
    const long long n = num_points, m = num_cells;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0 || m == 0) {                   // no member at all: every list is empty
        dc_zero_words(cptr, 2 * ((long)m + 1), s);
        DC_CHECK_LAUNCH(fn);
        if (n > 0) {
            hipLaunchKernelGGL(cl_rank_kernel, dim3(dc_cdiv(n, CL_THREADS)), dim3(CL_THREADS), 0, s, cluster, n, 0ll, cptr,
                               static_cast<const int64_t*>(nullptr), members);      // cptr[0] = 0: every position gets -1
            DC_CHECK_LAUNCH(fn);
        }
        return DC_OK;
    }
    DC_REQUIRE(workspace && aligned_to(workspace, 8) && workspace_bytes >= lists_bytes(n, m),
               "%s: workspace null, not 8-byte aligned or too small (%zu bytes, dc_cluster_lists_workspace_bytes: %zu)", fn,
               workspace_bytes, lists_bytes(n, m));
    const int sblocks = dc_cdiv(m, SC_THREADS), blocks = dc_cdiv(n, CL_THREADS);
    u64* cnt = static_cast<u64*>(workspace);
    u64* part = cnt + m;
    int64_t* unordered = reinterpret_cast<int64_t*>(part + sblocks);
    dc_zero_words(cnt, 2 * (long)m, s);
    hipLaunchKernelGGL((cl_count_kernel<false>), dim3(blocks), dim3(CL_THREADS), 0, s, cluster, n, m, cnt, unordered);
    hipLaunchKernelGGL(list_sum_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, m, part);
    hipLaunchKernelGGL(list_scan_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, m, part, cptr);
    hipLaunchKernelGGL((cl_count_kernel<true>), dim3(blocks), dim3(CL_THREADS), 0, s, cluster, n, m, cnt, unordered);
    hipLaunchKernelGGL(cl_rank_kernel, dim3(blocks), dim3(CL_THREADS), 0, s, cluster, n, m, cptr, unordered, members);
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}

DC_EXPORT int dc_cluster_pool(const float* x, int64_t ldx, int64_t num_points, int32_t C, const int64_t* cptr, const int64_t* members,
                              int64_t num_cells, int32_t mode, float* out, int64_t ldo, int32_t* arg, int64_t ldarg, void* stream) {
    const char* fn = "dc_cluster_pool";
    DC_REQUIRE(mode >= 0 && mode <= 3, "%s: mode = %d outside 0 .. 3 (max, min, sum, mean)", fn, mode);
    if (!sizes_ok(fn, num_points, num_cells, C)) return DC_ERR_ARG;
    DC_REQUIRE(ldx >= C && ldo >= C, "%s: leading dimensions (ldx %lld, ldo %lld) below C = %d", fn, (long long)ldx, (long long)ldo, C);
    if (num_cells == 0) return DC_OK;
    DC_REQUIRE(arg || mode >= dccl::MODE_SUM, "%s: null pointer (arg, unless mode is sum or mean)", fn);
    DC_REQUIRE(!arg || ldarg >= C, "%s: leading dimension ldarg = %lld below C = %d", fn, (long long)ldarg, C);
    DC_REQUIRE(cptr && out && (num_points == 0 || (x && members)), "%s: null pointer (x, cptr, members, out)", fn);
    const long long groups = (C + 3) / 4;
    hipLaunchKernelGGL(cl_pool_kernel, dim3(dc_cdiv(num_cells * groups, CL_THREADS)), dim3(CL_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, (long long)ldx, (long long)num_points, (int)C, cptr, members,
                       (long long)num_cells, (int)mode, vec16(x, ldx), out, (long long)ldo, vec16(out, ldo),
                       mode <= dccl::MODE_MIN ? arg : nullptr, (long long)ldarg, vec16(arg, ldarg));
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}

DC_EXPORT int dc_cluster_pool_backward(const float* g, int64_t ldg, int64_t num_cells, int32_t C, const int64_t* cluster,
                                       int64_t num_points, const int64_t* cptr, const int32_t* arg, int64_t ldarg, int32_t mode,
                                       float* dx, int64_t ldx, void* stream) {
    const char* fn = "dc_cluster_pool_backward";
    DC_REQUIRE(mode >= 0 && mode <= 3, "%s: mode = %d outside 0 .. 3 (max, min, sum, mean)", fn, mode);
    DC_REQUIRE(num_cells == 0 || num_points == 0 || arg || mode >= dccl::MODE_SUM, "%s: null pointer (arg, unless mode is sum or mean)",
               fn);
    DC_REQUIRE(!arg || ldarg >= C, "%s: leading dimension ldarg = %lld below C = %d", fn, (long long)ldarg, C);
    DC_REQUIRE(num_cells == 0 || num_points == 0 || cptr || mode != dccl::MODE_MEAN, "%s: null pointer (cptr, for the mean)", fn);
    return launch_gather(fn, g, ldg, num_cells, C, cluster, num_points, cptr, arg, ldarg, mode, dx, ldx, stream);
}

DC_EXPORT int dc_cluster_gather(const float* x, int64_t ldx, int64_t num_cells, int32_t C, const int64_t* cluster, int64_t num_points,
                                float* out, int64_t ldo, void* stream) {
    return launch_gather("dc_cluster_gather", x, ldx, num_cells, C, cluster, num_points, nullptr, nullptr, 0, dccl::MODE_SUM, out, ldo,
                         stream);
}

DC_EXPORT int dc_cluster_mean3(const float* p, int64_t num_points, const int64_t* cptr, const int64_t* members, int64_t num_cells,
                               int32_t normalize, float* out, void* stream) {
    const char* fn = "dc_cluster_mean3";
    if (!sizes_ok(fn, num_points, num_cells, 3)) return DC_ERR_ARG;
    DC_REQUIRE(normalize == 0 || normalize == 1, "%s: normalize = %d (0 or 1)", fn, normalize);
    if (num_cells == 0) return DC_OK;
    DC_REQUIRE(cptr && out && (num_points == 0 || (p && members)), "%s: null pointer (p, cptr, members, out)", fn);
    hipLaunchKernelGGL(cl_mean3_kernel, dim3(dc_cdiv(num_cells, CL_THREADS)), dim3(CL_THREADS), 0, static_cast<hipStream_t>(stream), p,
                       (long long)num_points, cptr, members, (long long)num_cells, (int)normalize, out);
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}

DC_EXPORT int dc_cluster_majority(const int64_t* labels, int64_t num_points, const int64_t* cptr, const int64_t* members,
                                  int64_t num_cells, int32_t num_classes, int64_t* out, void* stream) {
    const char* fn = "dc_cluster_majority";
    if (!sizes_ok(fn, num_points, num_cells, 1)) return DC_ERR_ARG;
    DC_REQUIRE(num_classes >= 1 && num_classes <= dccl::MAX_CLASSES, "%s: num_classes = %d outside [1, %d]", fn, num_classes,
               dccl::MAX_CLASSES);
    if (num_cells == 0) return DC_OK;
    DC_REQUIRE(cptr && out && (num_points == 0 || (labels && members)), "%s: null pointer (labels, cptr, members, out)", fn);
    hipLaunchKernelGGL(cl_majority_kernel, dim3(dc_cdiv(num_cells, CL_THREADS)), dim3(CL_THREADS), 0, static_cast<hipStream_t>(stream),
                       labels, (long long)num_points, cptr, members, (long long)num_cells, (int)num_classes, out);
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}
