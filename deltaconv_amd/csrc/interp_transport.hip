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
// a launch; a workgroup past its cloud's end returns, block-uniformly:
//   transport_table_kernel      one thread per slot of a query cloud (256 slots a workgroup); the k slots of a query re-read its three
//                               target rows (36 B, cache hits), gather one source frame (24 B) and write one 16-byte entry
//   vector_interpolate_kernel   thread = (query, group of 4 channels), the mapping of interpolate_kernel: per slot one 16-byte load
//                               of M (the same address for every group of the query) and two source rows, 16 bytes at a time where
//                               v, ldv and C allow, scalar otherwise (any C >= 1)
//   vector_interpolate_backward_kernel   thread = (source row, group of 4 channels), the mapping of interpolate_backward_kernel: it
//                               walks the row's in-edges (the lists of dc_knn_cross_transpose) in order, four edges in flight
// Plain vector loads and stores, no atomics, no LDS: the outputs are a function of the inputs only.
#include "common.h"
#include "interp_transport_math.h"

namespace {

constexpr int VT_THREADS = 256;
constexpr long long VT_MAX_REF = 0x7fffffffll;                      // idx is int32, local to the reference cloud
constexpr long long VT_MAX_ITEMS = (1ll << 31) * VT_THREADS - VT_THREADS;   // 256 items a workgroup, at most 2^31 - 1 of them

__global__ __launch_bounds__(VT_THREADS) void transport_table_kernel(const int64_t* __restrict__ qptr, const int64_t* __restrict__ rptr,
                                                                     long long num_query, int k, const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ d2, const float* __restrict__ tn,
                                                                     const float* __restrict__ tx, const float* __restrict__ ty,
                                                                     const float* sn, const float* sx, int non_oriented,
                                                                     float* __restrict__ tmat) {
    const int b = blockIdx.y;
    const long long qbase = qptr[b], nq = qptr[b + 1] - qbase;
    const long long rbase = rptr[b];
    long long nr = rptr[b + 1] - rbase;
    nr = nr < 0 ? 0 : (nr > VT_MAX_REF ? VT_MAX_REF : nr);
    const long long e0 = (long long)blockIdx.x * VT_THREADS;
    if (nq <= 0 || e0 >= nq * k) return;      // block-uniform
    const long long el = e0 + threadIdx.x;    // the slot within this query cloud
    if (el >= nq * k) return;
    const long long ql = (long long)((unsigned long long)el / (unsigned)k);
    const long long q = qbase + ql;
    if (q < 0 || q >= num_query) return;      // (never with offsets that fit the call's arrays)
    const dcconn::R4 m = dcvinterp::entry_in_pair(q, (int)(el - ql * k), rbase, nr, k, idx, d2, tn, tx, ty, sn, sx, non_oriented);
    *reinterpret_cast<dcconn::R4*>(tmat + 4 * (q * k + (el - ql * k))) = m;
}

__device__ __forceinline__ void store_group(float* o, const float* v, int nc, bool vec) {
    if (vec) {
        dc_f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<dc_f32x4*>(o) = t;
    } else {
        for (int c = 0; c < nc; ++c) o[c] = v[c];
    }
}

__global__ __launch_bounds__(VT_THREADS) void vector_interpolate_kernel(const float* __restrict__ v, long long ldv, int C,
                                                                        const int64_t* __restrict__ qptr,
                                                                        const int64_t* __restrict__ rptr, int k,
                                                                        const int32_t* __restrict__ idx,
                                                                        const dcconn::R4* __restrict__ tmat, float* __restrict__ out,
                                                                        long long ldo, int vec_in, int vec_out) {
    const int b = blockIdx.y;
    const long long qbase = qptr[b], nq = qptr[b + 1] - qbase;
    const long long rbase = rptr[b];
    long long nr = rptr[b + 1] - rbase;
    nr = nr < 0 ? 0 : (nr > VT_MAX_REF ? VT_MAX_REF : nr);
    const long long q0 = (long long)blockIdx.x * VT_THREADS;
    if (q0 >= nq) return;                     // block-uniform
    const int rows = (int)(nq - q0 < VT_THREADS ? nq - q0 : VT_THREADS);
    const int groups = (C + 3) >> 2;
    const float* vr = v + 2 * rbase * ldv;    // the rows of this pair's reference cloud
    for (int item = threadIdx.x; item < rows * groups; item += VT_THREADS) {
        const int r = item / groups, g = item - r * groups;
        const long long row = qbase + q0 + r;
        const int c0 = 4 * g, nc = C - c0 < 4 ? C - c0 : 4;
        float ou[4], ov[4];
        dcvinterp::fwd4(vr, ldv, nr, k, idx + row * k, tmat + row * k, c0, nc, vec_in && nc == 4, ou, ov);
        float* o = out + (2 * row) * ldo + c0;
        store_group(o, ou, nc, vec_out && nc == 4);
        store_group(o + ldo, ov, nc, vec_out && nc == 4);
    }
}

__global__ __launch_bounds__(VT_THREADS) void vector_interpolate_backward_kernel(
    const float* __restrict__ g, long long ldg, long long g_rows, int C, const int64_t* __restrict__ rptr, int k,
    const int64_t* __restrict__ tptr, const int64_t* __restrict__ tedge, long long num_edges, long long edge_base,
    const dcconn::R4* __restrict__ tmat, long long tmat_rows, float* __restrict__ dv, long long ldv, int rpb, int vec_in, int vec_out) {
    const int b = blockIdx.y;
    const long long rbase = rptr[b], nr = rptr[b + 1] - rbase;
    const long long r0 = (long long)blockIdx.x * rpb;
    if (r0 >= nr) return;                     // block-uniform (covers nr <= 0)
    const int rows = (int)(nr - r0 < rpb ? nr - r0 : rpb);
    const int groups = (C + 3) >> 2;
    for (int item = threadIdx.x; item < rows * groups; item += VT_THREADS) {
        const int r = item / groups, gi = item - r * groups;
        const long long row = rbase + r0 + r;
        const int c0 = 4 * gi, nc = C - c0 < 4 ? C - c0 : 4;
        long long lo = tptr[row], hi = tptr[row + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > num_edges ? num_edges : hi;
        float du[4], dw[4];
        dcvinterp::bwd4(g, ldg, g_rows, k, edge_base, tedge + lo, tmat, tmat_rows, hi > lo ? hi - lo : 0, c0, nc, vec_in && nc == 4, du,
                        dw);
        float* o = dv + (2 * row) * ldv + c0;
        store_group(o, du, nc, vec_out && nc == 4);
        store_group(o + ldv, dw, nc, vec_out && nc == 4);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

DC_EXPORT int dc_knn_cross_transport(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t max_query_cloud,
                                     int32_t k, const int32_t* idx, const float* d2, const float* tn, const float* tx,
                                     const float* ty, const float* sn, const float* sx, int32_t non_oriented, float* tmat,
                                     void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_cross_transport: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_cross_transport: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(num_query >= 0 && num_query <= VT_MAX_ITEMS / dcinterp::MAX_K,
               "dc_knn_cross_transport: num_query = %lld outside [0, 2^35)", (long long)num_query);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= VT_MAX_ITEMS / dcinterp::MAX_K,
               "dc_knn_cross_transport: max_query_cloud = %lld outside [0, 2^35)", (long long)max_query_cloud);
    if (B == 0 || max_query_cloud == 0 || num_query == 0) return DC_OK;
    DC_REQUIRE(qptr && rptr && idx && d2 && tn && tx && ty && sn && sx && tmat,
               "dc_knn_cross_transport: null pointer (qptr, rptr, idx, d2, tn, tx, ty, sn, sx, tmat)");
    DC_REQUIRE(aligned16(tmat), "dc_knn_cross_transport: tmat must be 16-byte aligned");
    hipLaunchKernelGGL(transport_table_kernel, dim3(dc_cdiv((long long)max_query_cloud * k, VT_THREADS), B), dim3(VT_THREADS), 0,
                       static_cast<hipStream_t>(stream), qptr, rptr, (long long)num_query, (int)k, idx, d2, tn, tx, ty, sn, sx,
                       (int)non_oriented, tmat);
    DC_CHECK_LAUNCH("dc_knn_cross_transport");
    return DC_OK;
}

DC_EXPORT int dc_knn_interpolate_vectors(const float* v, int64_t ldv, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                                         int64_t max_query_cloud, int32_t k, const int32_t* idx, const float* tmat, float* out,
                                         int64_t ldo, void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_interpolate_vectors: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_interpolate_vectors: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(C >= 1 && C <= (1 << 20), "dc_knn_interpolate_vectors: C = %d channels, supported: 1 .. 2^20", C);
    DC_REQUIRE(ldv >= C && ldo >= C, "dc_knn_interpolate_vectors: leading dimensions ldv = %lld, ldo = %lld below C = %d",
               (long long)ldv, (long long)ldo, C);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= VT_MAX_ITEMS,
               "dc_knn_interpolate_vectors: max_query_cloud = %lld outside [0, 2^39)", (long long)max_query_cloud);
    if (B == 0 || max_query_cloud == 0) return DC_OK;
    DC_REQUIRE(v && qptr && rptr && idx && tmat && out, "dc_knn_interpolate_vectors: null pointer (v, qptr, rptr, idx, tmat, out)");
    DC_REQUIRE(aligned16(tmat), "dc_knn_interpolate_vectors: tmat must be 16-byte aligned");
    const int vec_in = aligned16(v) && (ldv & 3) == 0;
    const int vec_out = aligned16(out) && (ldo & 3) == 0;
    hipLaunchKernelGGL(vector_interpolate_kernel, dim3(dc_cdiv(max_query_cloud, VT_THREADS), B), dim3(VT_THREADS), 0,
                       static_cast<hipStream_t>(stream), v, (long long)ldv, (int)C, qptr, rptr, (int)k, idx,
                       reinterpret_cast<const dcconn::R4*>(tmat), out, (long long)ldo, vec_in, vec_out);
    DC_CHECK_LAUNCH("dc_knn_interpolate_vectors");
    return DC_OK;
}

DC_EXPORT int dc_knn_interpolate_vectors_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr,
                                                  int32_t B, int64_t max_ref_cloud, int32_t k, const int64_t* tptr,
                                                  const int64_t* tedge, int64_t num_edges, int64_t edge_base, const float* tmat,
                                                  int64_t tmat_rows, float* dv, int64_t ldv, void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_interpolate_vectors_backward: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_interpolate_vectors_backward: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(C >= 1 && C <= (1 << 20), "dc_knn_interpolate_vectors_backward: C = %d channels, supported: 1 .. 2^20", C);
    DC_REQUIRE(ldg >= C && ldv >= C, "dc_knn_interpolate_vectors_backward: leading dimensions ldg = %lld, ldv = %lld below C = %d",
               (long long)ldg, (long long)ldv, C);
    DC_REQUIRE(max_ref_cloud >= 0 && max_ref_cloud < (1ll << 31),
               "dc_knn_interpolate_vectors_backward: max_ref_cloud = %lld outside [0, 2^31)", (long long)max_ref_cloud);
    DC_REQUIRE(num_g_rows >= 0 && num_edges >= 0 && tmat_rows >= 0,
               "dc_knn_interpolate_vectors_backward: num_g_rows = %lld, num_edges = %lld, tmat_rows = %lld below 0",
               (long long)num_g_rows, (long long)num_edges, (long long)tmat_rows);
    if (B == 0 || max_ref_cloud == 0) return DC_OK;
    DC_REQUIRE(rptr && tptr && dv, "dc_knn_interpolate_vectors_backward: null pointer (rptr, tptr, dv)");
    DC_REQUIRE((num_edges == 0 || num_g_rows == 0 || tmat_rows == 0) || (g && tedge && tmat),
               "dc_knn_interpolate_vectors_backward: null pointer (g, tedge, tmat)");
    DC_REQUIRE(aligned16(tmat), "dc_knn_interpolate_vectors_backward: tmat must be 16-byte aligned");
    if (!g || !tedge || !tmat) num_edges = 0;                    // nothing to read: every list is cut to nothing, dv gets zeros
    const int vec_in = aligned16(g) && (ldg & 3) == 0;
    const int vec_out = aligned16(dv) && (ldv & 3) == 0;
    // a thread's cost is its list length, so a workgroup takes only as many source rows as give each thread about one item
    const int groups = (C + 3) >> 2, rpb = groups >= VT_THREADS ? 1 : VT_THREADS / groups;
    hipLaunchKernelGGL(vector_interpolate_backward_kernel, dim3(dc_cdiv(max_ref_cloud, rpb), B), dim3(VT_THREADS), 0,
                       static_cast<hipStream_t>(stream), g, (long long)ldg, (long long)num_g_rows, (int)C, rptr, (int)k, tptr, tedge,
                       (long long)num_edges, (long long)edge_base, reinterpret_cast<const dcconn::R4*>(tmat), (long long)tmat_rows, dv,
                       (long long)ldv, rpb, vec_in, vec_out);
    DC_CHECK_LAUNCH("dc_knn_interpolate_vectors_backward");
    return DC_OK;
}
