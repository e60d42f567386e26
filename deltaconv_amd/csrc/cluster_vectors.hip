// Pooling of tangent-vector features over the cells of a cluster vector: the VECTOR stream's sibling of cluster.hip, the
// linear-time sibling of pool_vectors.hip.  Every member of a cell is carried into the cell's frame by parallel transport
// (deltaconv/geometry/connection.py:6-47) before it is reduced; on the way up the cell's vector is carried into every member's
// frame.  The arithmetic is csrc/cluster_vectors_math.h (shared with tests/hostcheck_cluster_vectors); the lists are
// dc_cluster_lists'.
//
// Every point belongs to ONE cell, so the rotations are stored per POINT (dc_cluster_rotation, once per clustering and direction:
// 16 N bytes) and the apply kernels are pure walks / gathers over them:
//   clv_rotation_kernel   one thread per point: one 16-byte entry
//   clv_walk_kernel<T>    thread = (cell, group of 4 channels): the cell's members in list order, four in flight; per member one
//                         16-byte load of R (the same address for every channel group of the cell) and two rows, 16 bytes at a
//                         time where base, stride and C allow, scalar otherwise (any C >= 1).  T = false: the pooling over rdown,
//                         with arg; T = true: the un-pooling's backward, the sum through the transposed rup
//   clv_gather_kernel<T>  thread = (point, group of 4 channels): the two rows of the point's cell through its own R.  T = true:
//                         the pooling's backward (R^T, arg / mean handling); T = false: the un-pooling (R)
// Plain loads and stores, no LDS, no floating-point atomics; launch sizes from the HOST numbers alone: every call is capturable.
#include "common.h"
#include "cluster_vectors_math.h"

namespace {

constexpr int CLV_THREADS = 256;
constexpr long long CLV_MAX_ITEMS = (long long)CLV_THREADS * 0x7fffffffll;    // threads of one launch

__global__ __launch_bounds__(CLV_THREADS) void clv_rotation_kernel(const int64_t* __restrict__ cluster, long long n, long long m,
                                                                   const float* __restrict__ fn, const float* __restrict__ fx,
                                                                   const float* __restrict__ fy, const float* __restrict__ cn,
                                                                   const float* __restrict__ cx, const float* __restrict__ cy,
                                                                   int to_cell, int non_oriented, float* __restrict__ rmat) {
    const long long i = (long long)blockIdx.x * CLV_THREADS + threadIdx.x;
    if (i >= n) return;
    *reinterpret_cast<dcconn::R4*>(rmat + 4 * i) = dcclv::rotation(i, cluster[i], m, fn, fx, fy, cn, cx, cy, to_cell, non_oriented);
}

__device__ __forceinline__ void store2(float* __restrict__ out, long long ldo, long long row, int c0, int nc, int vec, const float* a,
                                       const float* b) {
    float* o0 = out + (2 * row) * ldo + c0;
    float* o1 = o0 + ldo;
    if (vec && nc == 4) {
        *reinterpret_cast<dc_f32x4*>(o0) = dc_f32x4{a[0], a[1], a[2], a[3]};
        *reinterpret_cast<dc_f32x4*>(o1) = dc_f32x4{b[0], b[1], b[2], b[3]};
    } else {
        for (int c = 0; c < nc; ++c) {
            o0[c] = a[c];
            o1[c] = b[c];
        }
    }
}

template <bool TRANSPOSED>
__global__ __launch_bounds__(CLV_THREADS) void clv_walk_kernel(const float* __restrict__ v, long long ldv, long long n, int C,
                                                               const int64_t* __restrict__ cptr,
                                                               const int64_t* __restrict__ members, long long m,
                                                               const dcconn::R4* __restrict__ rmat, int mode, int vec_in,
                                                               float* __restrict__ out, long long ldo, int vec_out,
                                                               int32_t* __restrict__ arg, long long ldarg, int vec_arg) {
    const int groups = (C + 3) >> 2;
    const long long t = (long long)blockIdx.x * CLV_THREADS + threadIdx.x;
    const long long j = t / groups;
    if (j >= m) return;
    const int c0 = 4 * (int)(t - j * groups), nc = C - c0 < 4 ? C - c0 : 4;
    long long lo = cptr[j], hi = cptr[j + 1];                  // [lo, hi) of cell j inside the n entries of members
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const long long len = hi > lo ? hi - lo : 0;
    float a[4], b[4];
    int at[4];
    dcclv::walk4<TRANSPOSED>(v, ldv, n, members + lo, len, rmat, mode, c0, nc, vec_in && nc == 4, a, b, at);
    store2(out, ldo, j, c0, nc, vec_out, a, b);
    if (!TRANSPOSED && arg) {
        int32_t* p = arg + j * ldarg + c0;
        if (vec_arg && nc == 4) {
            *reinterpret_cast<int4*>(p) = make_int4(at[0], at[1], at[2], at[3]);
        } else {
            for (int c = 0; c < nc; ++c) p[c] = at[c];
        }
    }
}

template <bool TRANSPOSED>
__global__ __launch_bounds__(CLV_THREADS) void clv_gather_kernel(const float* __restrict__ g, long long ldg, long long m, int C,
                                                                 const int64_t* __restrict__ cluster, long long n,
                                                                 const int64_t* __restrict__ cptr,
                                                                 const dcconn::R4* __restrict__ rmat,
                                                                 const int32_t* __restrict__ arg, long long ldarg, int mode,
                                                                 int vec_in, float* __restrict__ out, long long ldo, int vec_out) {
    const int groups = (C + 3) >> 2;
    const long long t = (long long)blockIdx.x * CLV_THREADS + threadIdx.x;
    const long long i = t / groups;
    if (i >= n) return;
    const int c0 = 4 * (int)(t - i * groups), nc = C - c0 < 4 ? C - c0 : 4;
    float a[4], b[4];
    dcclv::gather4<TRANSPOSED>(g, ldg, m, cluster[i], i, rmat[i], cptr, arg, ldarg, mode, c0, nc, vec_in && nc == 4, a, b);
    store2(out, ldo, i, c0, nc, vec_out, a, b);
}

inline int vec16(const void* p, long long ld) { return p && aligned_to(p, 16) && (ld & 3) == 0; }

// the checks the entry points share (those of cluster.hip): sizes, and one launch's worth of threads
bool sizes_ok(const char* fn, int64_t n, int64_t m, int32_t C) {
    if (n < 0 || n > dcclv::MAX_ROWS) return dc_set_error("%s: num_points = %lld outside [0, 2^31)", fn, (long long)n), false;
    if (m < 0 || m > dcclv::MAX_ROWS) return dc_set_error("%s: num_cells = %lld outside [0, 2^31)", fn, (long long)m), false;
    if (C < 1) return dc_set_error("%s: C = %d, at least one channel", fn, C), false;
    const long long groups = (C + 3) / 4;
    if ((n > m ? n : m) * groups > CLV_MAX_ITEMS)
        return dc_set_error("%s: %lld rows of %d channels are more than one launch takes", fn, (long long)(n > m ? n : m), C), false;
    return true;
}

// the walk over the member lists: v [2 n, C] -> out [2 m, C]
template <bool TRANSPOSED>
int launch_walk(const char* fn, const float* v, int64_t ldv, int64_t n, int32_t C, const int64_t* cptr, const int64_t* members,
                int64_t m, const float* rmat, int32_t mode, float* out, int64_t ldo, int32_t* arg, int64_t ldarg, void* stream) {
    if (!sizes_ok(fn, n, m, C)) return DC_ERR_ARG;
    DC_REQUIRE(ldv >= C && ldo >= C, "%s: leading dimensions (%lld, %lld) below C = %d", fn, (long long)ldv, (long long)ldo, C);
    if (m == 0) return DC_OK;
    DC_REQUIRE(cptr && out && (n == 0 || (v && members && rmat)), "%s: null pointer (values, cptr, members, rmat, out)", fn);
    DC_REQUIRE(!rmat || aligned_to(rmat, 16), "%s: rmat must be 16-byte aligned", fn);
    const long long groups = (C + 3) / 4;
    hipLaunchKernelGGL((clv_walk_kernel<TRANSPOSED>), dim3(dc_cdiv(m * groups, CLV_THREADS)), dim3(CLV_THREADS), 0,
                       static_cast<hipStream_t>(stream), v, (long long)ldv, (long long)n, (int)C, cptr, members, (long long)m,
                       reinterpret_cast<const dcconn::R4*>(rmat), (int)mode, vec16(v, ldv), out, (long long)ldo, vec16(out, ldo), arg,
                       (long long)ldarg, vec16(arg, ldarg));
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}

// the gather from every point's cell: g [2 m, C] -> out [2 n, C]
template <bool TRANSPOSED>
int launch_gather(const char* fn, const float* g, int64_t ldg, int64_t m, int32_t C, const int64_t* cluster, int64_t n,
                  const int64_t* cptr, const float* rmat, const int32_t* arg, int64_t ldarg, int32_t mode, float* out, int64_t ldo,
                  void* stream) {
    if (!sizes_ok(fn, n, m, C)) return DC_ERR_ARG;
    DC_REQUIRE(ldg >= C && ldo >= C, "%s: leading dimensions (%lld, %lld) below C = %d", fn, (long long)ldg, (long long)ldo, C);
    if (n == 0) return DC_OK;
    DC_REQUIRE(cluster && rmat && out && (m == 0 || g), "%s: null pointer (values, cluster, rmat, out)", fn);
    DC_REQUIRE(aligned_to(rmat, 16), "%s: rmat must be 16-byte aligned", fn);
    const long long groups = (C + 3) / 4;
    hipLaunchKernelGGL((clv_gather_kernel<TRANSPOSED>), dim3(dc_cdiv(n * groups, CLV_THREADS)), dim3(CLV_THREADS), 0,
                       static_cast<hipStream_t>(stream), g, (long long)ldg, (long long)m, (int)C, cluster, (long long)n, cptr,
                       reinterpret_cast<const dcconn::R4*>(rmat), arg, (long long)ldarg, (int)mode, vec16(g, ldg), out, (long long)ldo,
                       vec16(out, ldo));
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}

}  // namespace

DC_EXPORT int dc_cluster_rotation(const int64_t* cluster, int64_t num_points, int64_t num_cells, const float* fine_normal,
                                  const float* fine_x, const float* fine_y, const float* coarse_normal, const float* coarse_x,
                                  const float* coarse_y, int32_t to_cell, int32_t non_oriented, float* rmat, void* stream) {
    const char* fn = "dc_cluster_rotation";
    if (!sizes_ok(fn, num_points, num_cells, 1)) return DC_ERR_ARG;
    DC_REQUIRE(to_cell == 0 || to_cell == 1, "%s: to_cell = %d (0: into the points' frames, 1: into the cells')", fn, to_cell);
    if (num_points == 0) return DC_OK;
    DC_REQUIRE(cluster && rmat, "%s: null pointer (cluster, rmat)", fn);
    DC_REQUIRE(aligned_to(rmat, 16), "%s: rmat must be 16-byte aligned", fn);
    DC_REQUIRE(num_cells == 0 || (fine_normal && fine_x && coarse_normal && coarse_x && (to_cell ? coarse_y : fine_y)),
               "%s: null pointer (fine_normal, fine_x, coarse_normal, coarse_x, and the y-axes of the target frames)", fn);
    hipLaunchKernelGGL(clv_rotation_kernel, dim3(dc_cdiv(num_points, CLV_THREADS)), dim3(CLV_THREADS), 0, static_cast<hipStream_t>(stream),
                       cluster, (long long)num_points, (long long)num_cells, fine_normal, fine_x, fine_y, coarse_normal, coarse_x,
                       coarse_y, (int)to_cell, (int)non_oriented, rmat);
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}

DC_EXPORT int dc_cluster_pool_vectors(const float* v, int64_t ldv, int64_t num_points, int32_t C, const int64_t* cptr,
                                      const int64_t* members, int64_t num_cells, const float* rmat, int32_t mode, float* out,
                                      int64_t ldo, int32_t* arg, int64_t ldarg, void* stream) {
    const char* fn = "dc_cluster_pool_vectors";
    DC_REQUIRE(dcclv::mode_ok(mode), "%s: mode = %d, supported: 0 (max), 2 (sum), 3 (mean)", fn, mode);
    DC_REQUIRE(num_cells <= 0 || arg || mode >= dcclv::MODE_SUM, "%s: null pointer (arg, unless mode is sum or mean)", fn);
    DC_REQUIRE(!arg || ldarg >= C, "%s: leading dimension ldarg = %lld below C = %d", fn, (long long)ldarg, C);
    return launch_walk<false>(fn, v, ldv, num_points, C, cptr, members, num_cells, rmat, mode, out, ldo,
                              mode == dcclv::MODE_MAX ? arg : nullptr, ldarg, stream);
}

DC_EXPORT int dc_cluster_pool_vectors_backward(const float* g, int64_t ldg, int64_t num_cells, int32_t C, const int64_t* cluster,
                                               int64_t num_points, const int64_t* cptr, const float* rmat, const int32_t* arg,
                                               int64_t ldarg, int32_t mode, float* dv, int64_t ldv, void* stream) {
    const char* fn = "dc_cluster_pool_vectors_backward";
    DC_REQUIRE(dcclv::mode_ok(mode), "%s: mode = %d, supported: 0 (max), 2 (sum), 3 (mean)", fn, mode);
    const bool work = num_cells > 0 && num_points > 0;
    DC_REQUIRE(!work || arg || mode >= dcclv::MODE_SUM, "%s: null pointer (arg, unless mode is sum or mean)", fn);
    DC_REQUIRE(!arg || ldarg >= C, "%s: leading dimension ldarg = %lld below C = %d", fn, (long long)ldarg, C);
    DC_REQUIRE(!work || cptr || mode != dcclv::MODE_MEAN, "%s: null pointer (cptr, for the mean)", fn);
    return launch_gather<true>(fn, g, ldg, num_cells, C, cluster, num_points, cptr, rmat, mode == dcclv::MODE_MAX ? arg : nullptr, ldarg,
                               mode, dv, ldv, stream);
}

DC_EXPORT int dc_cluster_unpool_vectors(const float* x, int64_t ldx, int64_t num_cells, int32_t C, const int64_t* cluster,
                                        int64_t num_points, const float* rmat, float* out, int64_t ldo, void* stream) {
    return launch_gather<false>("dc_cluster_unpool_vectors", x, ldx, num_cells, C, cluster, num_points, nullptr, rmat, nullptr, 0,
                                dcclv::MODE_SUM, out, ldo, stream);
}

DC_EXPORT int dc_cluster_unpool_vectors_backward(const float* g, int64_t ldg, int64_t num_points, int32_t C, const int64_t* cptr,
                                                 const int64_t* members, int64_t num_cells, const float* rmat, float* dx, int64_t ldx,
                                                 void* stream) {
    return launch_walk<true>("dc_cluster_unpool_vectors_backward", g, ldg, num_points, C, cptr, members, num_cells, rmat,
                             dcclv::MODE_SUM, dx, ldx, nullptr, 0, stream);
}
