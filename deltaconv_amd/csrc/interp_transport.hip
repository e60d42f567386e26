// Interpolation of tangent-vector features between two clouds by parallel transport, batched over cloud pairs -- stands in for
// deltaconv/geometry/connection.py:6-47 (build_transport) composed with torch_geometric.nn.knn_interpolate: every neighbour's
// vector is carried into the target point's frame, then weighted as dc_knn_interpolate weights it.  The vector stream's way across
// resolutions (up from a sampled cloud, or -- with the roles swapped -- a transported, distance-weighted pooling down to one).
// The arithmetic is csrc/interp_transport_math.h (shared with tests/hostcheck_vector_interp).
//
// The per-slot matrices M = c * R are STORED (dc_knn_cross_transport, once per search) rather than recomputed by the apply
// kernels: a Propagator searches once per store and applies once per batch, vote and epoch, and forward and backward stay pure
// gather kernels of the dc_transport_sum form.  16 k bytes per target row next to the 8 k of idx / d2.
//
// Mapping, the grid conventions of interp.hip: (chunks of 256 items up to the largest cloud) x (cloud pairs), at most 65 535 pairs
// a launch; a workgroup past its cloud's end returns, block-uniformly.  The apply kernels are the frame of cross_stage.h:
//   transport_table_kernel      one thread per slot of a query cloud (256 slots a workgroup); the k slots of a query re-read its three
//                               target rows (36 B, cache hits), gather one source frame (24 B) and write one 16-byte entry
//   cross_fwd_kernel<VectorInterpF>   thread = (query, group of 4 channels): per slot one 16-byte load of M (the same address for
//                               every group of the query) and two source rows, 16 bytes at a time where v, ldv and C allow, scalar
//                               otherwise (any C >= 1)
//   cross_bwd_kernel<VectorInterpT>   thread = (source row, group of 4 channels): it walks the row's in-edges (the lists of
//                               dc_knn_cross_transpose) in order, four edges in flight
// Plain vector loads and stores, no atomics, no LDS: the outputs are a function of the inputs only.
#include "common.h"
#include "cross_stage.h"
#include "interp_transport_math.h"

namespace {
using dccross::THREADS;

__global__ __launch_bounds__(THREADS) void transport_table_kernel(const int64_t* __restrict__ qptr, const int64_t* __restrict__ rptr,
                                                                  long long num_query, int k, const int32_t* __restrict__ idx,
                                                                  const float* __restrict__ d2, const float* __restrict__ tn,
                                                                  const float* __restrict__ tx, const float* __restrict__ ty,
                                                                  const float* sn, const float* sx, int non_oriented,
                                                                  float* __restrict__ tmat) {
    const auto [qbase, nq, rbase, nr] = dccross::pair_span(qptr, rptr);
    const long long e0 = (long long)blockIdx.x * THREADS;
    if (nq <= 0 || e0 >= nq * k) return;      // block-uniform
    const long long el = e0 + threadIdx.x;    // the slot within this query cloud
    if (el >= nq * k) return;
    const long long ql = (long long)((unsigned long long)el / (unsigned)k);
    const long long q = qbase + ql;
    if (q < 0 || q >= num_query) return;      // (never with offsets that fit the call's arrays)
    const dcconn::R4 m = dcvinterp::entry_in_pair(q, (int)(el - ql * k), rbase, nr, k, idx, d2, tn, tx, ty, sn, sx, non_oriented);
    *reinterpret_cast<dcconn::R4*>(tmat + 4 * (q * k + (el - ql * k))) = m;
}

// A query's k reference vectors, each carried into its frame by the slot's matrix (cross_stage.h: cross_fwd_kernel).
struct VectorInterpF {
    static constexpr int ROWS = 2;
    const float* __restrict__ v;
    long long ldv;
    int k;
    const int32_t* __restrict__ idx;
    const dcconn::R4* __restrict__ tmat;
    __device__ __forceinline__ void operator()(const dccross::Span& p, long long row, int c0, int nc, bool vec, float (*o)[4]) const {
        dcvinterp::fwd4(v + 2 * p.rbase * ldv, ldv, p.nr, k, idx + row * k, tmat + row * k, c0, nc, vec, o[0], o[1]);
    }
};

// The ordered sum over a source row's in-edges, through the transposed matrices (cross_stage.h: cross_bwd_kernel).
struct VectorInterpT {
    static constexpr int ROWS = 2;
    const float* __restrict__ g;
    long long ldg, g_rows;
    int k;
    long long edge_base;
    const int64_t* __restrict__ tedge;
    const dcconn::R4* __restrict__ tmat;
    long long tmat_rows;
    __device__ __forceinline__ void operator()(long long lo, long long n, int c0, int nc, bool vec, float (*o)[4]) const {
        dcvinterp::bwd4(g, ldg, g_rows, k, edge_base, tedge + lo, tmat, tmat_rows, n, c0, nc, vec, o[0], o[1]);
    }
};

}  // namespace

DC_EXPORT int dc_knn_cross_transport(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t max_query_cloud,
                                     int32_t k, const int32_t* idx, const float* d2, const float* tn, const float* tx,
                                     const float* ty, const float* sn, const float* sx, int32_t non_oriented, float* tmat,
                                     void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_cross_transport: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_cross_transport: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(num_query >= 0 && num_query <= dccross::MAX_ITEMS / dcinterp::MAX_K,
               "dc_knn_cross_transport: num_query = %lld outside [0, 2^35)", (long long)num_query);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= dccross::MAX_ITEMS / dcinterp::MAX_K,
               "dc_knn_cross_transport: max_query_cloud = %lld outside [0, 2^35)", (long long)max_query_cloud);
    if (B == 0 || max_query_cloud == 0 || num_query == 0) return DC_OK;
    DC_REQUIRE(qptr && rptr && idx && d2 && tn && tx && ty && sn && sx && tmat,
               "dc_knn_cross_transport: null pointer (qptr, rptr, idx, d2, tn, tx, ty, sn, sx, tmat)");
    DC_REQUIRE(aligned_to(tmat, 16), "dc_knn_cross_transport: tmat must be 16-byte aligned");
    hipLaunchKernelGGL(transport_table_kernel, dim3(dc_cdiv((long long)max_query_cloud * k, THREADS), B), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), qptr, rptr, (long long)num_query, (int)k, idx, d2, tn, tx, ty, sn, sx,
                       (int)non_oriented, tmat);
    DC_CHECK_LAUNCH("dc_knn_cross_transport");
    return DC_OK;
}

DC_EXPORT int dc_knn_interpolate_vectors(const float* v, int64_t ldv, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                                         int64_t max_query_cloud, int32_t k, const int32_t* idx, const float* tmat, float* out,
                                         int64_t ldo, void* stream) {
    const dccross::Call c{"dc_knn_interpolate_vectors", "ldv", "out", "ldo", "v, qptr, rptr, idx, tmat, out", idx && tmat, tmat};
    return dccross::launch_fwd(c, v, ldv, C, qptr, rptr, B, max_query_cloud, k, out, ldo,
                               VectorInterpF{v, ldv, k, idx, reinterpret_cast<const dcconn::R4*>(tmat)}, stream);
}

DC_EXPORT int dc_knn_interpolate_vectors_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr,
                                                  int32_t B, int64_t max_ref_cloud, int32_t k, const int64_t* tptr,
                                                  const int64_t* tedge, int64_t num_edges, int64_t edge_base, const float* tmat,
                                                  int64_t tmat_rows, float* dv, int64_t ldv, void* stream) {
    DC_REQUIRE(tmat_rows >= 0, "dc_knn_interpolate_vectors_backward: tmat_rows = %lld below 0", (long long)tmat_rows);
    const dccross::Call c{"dc_knn_interpolate_vectors_backward", "ldg", "dv", "ldv", "g, tedge, tmat", tedge && tmat, tmat};
    return dccross::launch_bwd(c, g, ldg, num_g_rows, C, rptr, B, max_ref_cloud, k, tptr, num_edges, tmat_rows == 0, dv, ldv,
                               VectorInterpT{g, ldg, num_g_rows, k, edge_base, tedge, reinterpret_cast<const dcconn::R4*>(tmat),
                                             tmat_rows},
                               stream);
}
