// Pooling of tangent-vector features from a cloud down to a sampled one, batched over cloud pairs: the vector stream's
// set-abstraction step, the sibling of dc_knn_pool (pool.hip).  Every sampled point carries the vectors of its k nearest points of
// the full cloud into its own frame (parallel transport, deltaconv/geometry/connection.py:6-47) and takes the one of largest norm
// (max, per channel), their sum or their mean; the search is dc_knn_cross with the sampled cloud as the query.  The reference has
// no such call site.  The arithmetic is csrc/pool_vectors_math.h (shared with tests/hostcheck_pool_vectors).
//
// The per-slot rotations R are STORED (dc_knn_cross_rotation, once per search), as the M = c * R of dc_knn_cross_transport are:
// forward and backward stay pure gather kernels.  16 k bytes per target row.
//
// Mapping, the grid conventions of interp.hip: (chunks up to the largest cloud) x (cloud pairs), at most 65 535 pairs a launch; a
// workgroup past its cloud's end returns, block-uniformly.  The apply kernels are the frame of cross_stage.h:
//   rotation_table_kernel          one thread per slot of a query cloud (256 slots a workgroup), the kernel of
//                                  dc_knn_cross_transport without the coefficient: one 16-byte entry a thread
//   cross_fwd_kernel<PoolVectorsF> thread = (query, group of 4 channels): per slot one 16-byte load of R (the same address for every
//                                  group of the query) and two source rows, 16 bytes at a time where v, ldv and C allow, scalar
//                                  otherwise (any C >= 1).  Beside the frame's store of the two pooled rows the body writes the
//                                  group's four slot numbers (max) and, from the thread of channel group 0, the query's count
//   cross_bwd_kernel<PoolVectorsT<MODE>>   thread = (source row, group of 4 channels): it walks the row's in-edges (the lists of
//                                  dc_knn_cross_transpose) in order, four edges in flight; per edge one table entry, two rows of g
//                                  and the four slot numbers (max) or the count (mean) of the edge's query
// Plain vector loads and stores, no atomics, no LDS: the outputs are a function of the inputs only.
#include "common.h"
#include "cross_stage.h"
#include "pool_vectors_math.h"

namespace {
using dccross::THREADS;

__global__ __launch_bounds__(THREADS) void rotation_table_kernel(const int64_t* __restrict__ qptr, const int64_t* __restrict__ rptr,
                                                                 long long num_query, int k, const int32_t* __restrict__ idx,
                                                                 const float* __restrict__ tn, const float* __restrict__ tx,
                                                                 const float* __restrict__ ty, const float* sn, const float* sx,
                                                                 int non_oriented, float* __restrict__ rmat) {
    const auto [qbase, nq, rbase, nr] = dccross::pair_span(qptr, rptr);
    const long long e0 = (long long)blockIdx.x * THREADS;
    if (nq <= 0 || e0 >= nq * k) return;      // block-uniform
    const long long el = e0 + threadIdx.x;    // the slot within this query cloud
    if (el >= nq * k) return;
    const long long ql = (long long)((unsigned long long)el / (unsigned)k);
    const long long q = qbase + ql;
    if (q < 0 || q >= num_query) return;      // (never with offsets that fit the call's arrays)
    const dcconn::R4 m = dcvpool::rotation_in_pair(q, (int)(el - ql * k), rbase, nr, k, idx, tn, tx, ty, sn, sx, non_oriented);
    *reinterpret_cast<dcconn::R4*>(rmat + 4 * (q * k + (el - ql * k))) = m;
}

// The reduction over a query's k transported reference vectors, with its side outputs (cross_stage.h: cross_fwd_kernel).
struct PoolVectorsF {
    static constexpr int ROWS = 2;
    const float* __restrict__ v;
    long long ldv;
    int k, mode;
    const int32_t* __restrict__ idx;
    const dcconn::R4* __restrict__ rmat;
    unsigned char* __restrict__ arg;          // null: sum / mean without one
    long long ldarg;
    unsigned char* __restrict__ cnt;
    int word;                                 // arg + 4 g is 4-byte aligned in every row
    __device__ __forceinline__ void operator()(const dccross::Span& p, long long row, int c0, int nc, bool vec, float (*o)[4]) const {
        unsigned char a[4];
        const int n = dcvpool::fwd4(v + 2 * p.rbase * ldv, ldv, p.nr, k, idx + row * k, rmat + row * k, mode, c0, nc, vec, o[0], o[1], a);
        if (arg && mode == dcvpool::MODE_MAX) dcvpool::store_arg4(arg + row * ldarg + c0, a, nc, word && nc == 4);
        if (c0 == 0) cnt[row] = (unsigned char)n;
    }
};

// The ordered sum over a source row's in-edges, through the transposed rotations (cross_stage.h: cross_bwd_kernel).
template <int MODE>
struct PoolVectorsT {
    static constexpr int ROWS = 2;
    const float* __restrict__ g;
    long long ldg, g_rows;
    int k;
    const int64_t* __restrict__ tedge;
    const dcconn::R4* __restrict__ rmat;
    const unsigned char* __restrict__ arg;
    long long ldarg;
    const unsigned char* __restrict__ cnt;
    int word;
    __device__ __forceinline__ void operator()(long long lo, long long n, int c0, int nc, bool vec, float (*o)[4]) const {
        dcvpool::bwd4<MODE>(g, ldg, g_rows, k, tedge + lo, rmat, n, arg, ldarg, cnt, c0, nc, vec, word && nc == 4, o[0], o[1]);
    }
};

inline int arg_words(const void* arg, long long ldarg) { return arg && aligned_to(arg, 4) && (ldarg & 3) == 0; }

}  // namespace

DC_EXPORT int dc_knn_cross_rotation(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t max_query_cloud,
                                    int32_t k, const int32_t* idx, const float* tn, const float* tx, const float* ty,
                                    const float* sn, const float* sx, int32_t non_oriented, float* rmat, void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_cross_rotation: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_cross_rotation: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(num_query >= 0 && num_query <= dccross::MAX_ITEMS / dcinterp::MAX_K,
               "dc_knn_cross_rotation: num_query = %lld outside [0, 2^35)", (long long)num_query);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= dccross::MAX_ITEMS / dcinterp::MAX_K,
               "dc_knn_cross_rotation: max_query_cloud = %lld outside [0, 2^35)", (long long)max_query_cloud);
    if (B == 0 || max_query_cloud == 0 || num_query == 0) return DC_OK;
    DC_REQUIRE(qptr && rptr && idx && tn && tx && ty && sn && sx && rmat,
               "dc_knn_cross_rotation: null pointer (qptr, rptr, idx, tn, tx, ty, sn, sx, rmat)");
    DC_REQUIRE(aligned_to(rmat, 16), "dc_knn_cross_rotation: rmat must be 16-byte aligned");
    hipLaunchKernelGGL(rotation_table_kernel, dim3(dc_cdiv((long long)max_query_cloud * k, THREADS), B), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), qptr, rptr, (long long)num_query, (int)k, idx, tn, tx, ty, sn, sx,
                       (int)non_oriented, rmat);
    DC_CHECK_LAUNCH("dc_knn_cross_rotation");
    return DC_OK;
}

DC_EXPORT int dc_knn_pool_vectors(const float* v, int64_t ldv, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                                  int64_t max_query_cloud, int32_t k, const int32_t* idx, const float* rmat, int32_t mode,
                                  float* out, int64_t ldo, uint8_t* arg, int64_t ldarg, uint8_t* cnt, void* stream) {
    DC_REQUIRE(dcvpool::mode_ok(mode), "dc_knn_pool_vectors: mode = %d, supported: 0 (max), 2 (sum), 3 (mean)", mode);
    DC_REQUIRE(!arg || ldarg >= C, "dc_knn_pool_vectors: leading dimension ldarg = %lld below C = %d", (long long)ldarg, C);
    DC_REQUIRE(cnt && (arg || mode >= dcvpool::MODE_SUM), "dc_knn_pool_vectors: null pointer (cnt; arg unless mode is sum or mean)");
    const dccross::Call c{"dc_knn_pool_vectors", "ldv", "out", "ldo", "v, qptr, rptr, idx, rmat, out", idx && rmat, rmat, "rmat"};
    return dccross::launch_fwd(c, v, ldv, C, qptr, rptr, B, max_query_cloud, k, out, ldo,
                               PoolVectorsF{v, ldv, k, mode, idx, reinterpret_cast<const dcconn::R4*>(rmat), arg, ldarg, cnt,
                                            arg_words(arg, ldarg)},
                               stream);
}

DC_EXPORT int dc_knn_pool_vectors_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                                           int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge,
                                           int64_t num_edges, const float* rmat, int32_t mode, const uint8_t* arg, int64_t ldarg,
                                           const uint8_t* cnt, float* dv, int64_t ldv, void* stream) {
    DC_REQUIRE(dcvpool::mode_ok(mode), "dc_knn_pool_vectors_backward: mode = %d, supported: 0 (max), 2 (sum), 3 (mean)", mode);
    DC_REQUIRE(!arg || ldarg >= C, "dc_knn_pool_vectors_backward: leading dimension ldarg = %lld below C = %d", (long long)ldarg, C);
    DC_REQUIRE(cnt && (arg || mode >= dcvpool::MODE_SUM),
               "dc_knn_pool_vectors_backward: null pointer (cnt; arg unless mode is sum or mean)");
    const dccross::Call c{"dc_knn_pool_vectors_backward", "ldg", "dv", "ldv", "g, tedge, rmat", tedge && rmat, rmat, "rmat"};
    const auto R = reinterpret_cast<const dcconn::R4*>(rmat);
    const auto run = [&](auto body) {
        return dccross::launch_bwd(c, g, ldg, num_g_rows, C, rptr, B, max_ref_cloud, k, tptr, num_edges, false, dv, ldv, body, stream);
    };
    const int word = arg_words(arg, ldarg);
    if (mode == dcvpool::MODE_MAX) return run(PoolVectorsT<dcvpool::MODE_MAX>{g, ldg, num_g_rows, k, tedge, R, arg, ldarg, cnt, word});
    if (mode == dcvpool::MODE_SUM) return run(PoolVectorsT<dcvpool::MODE_SUM>{g, ldg, num_g_rows, k, tedge, R, arg, ldarg, cnt, word});
    return run(PoolVectorsT<dcvpool::MODE_MEAN>{g, ldg, num_g_rows, k, tedge, R, arg, ldarg, cnt, word});
}
