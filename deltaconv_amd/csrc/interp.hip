// Two-set nearest-neighbour search and inverse-squared-distance interpolation, batched over cloud pairs -- replaces
// torch_cluster.knn(x, y, k, batch_x, batch_y) and torch_geometric.nn.knn_interpolate (PointNet++ feature propagation): the way
// back up from a sampled cloud to the points or vertices it was sampled from -- and the gradient of the interpolation w.r.t. the
// interpolated FEATURES (dc_knn_cross_transpose + dc_knn_interpolate_backward).  No gradient for positions or distances.
//
// Order (bit-exact contract shared with dc_knn, knn.hip:5-6): fp32 squared distance ((dx*dx + dy*dy) + dz*dz) evaluated WITHOUT
// fma contraction, ascending, ties by lower reference index.  The arithmetic is csrc/interp_math.h (shared with
// tests/hostcheck_interp).
//
// Mapping, both kernels on the grid (chunks of 256 queries up to max_query_cloud) x (cloud pairs); a workgroup past its cloud's
// end returns, block-uniformly (cross_stage.h: the pair span, the frame of the apply kernels and their argument checks):
//   knn_cross_kernel    one query per thread.  The reference cloud is staged through LDS in SoA tiles of 2048 points (24 KiB)
//                       and read as broadcasts; the sorted top-K list lives in registers (the sorted-insertion kernel of knn.hip,
//                       P = 1), K in {1, 4, 8, 16} by dispatch.  VALU-bound: Nq x Nr distance evaluations per pair.
//   cross_fwd_kernel<InterpF>   thread = (query, group of 4 channels), consecutive threads on consecutive groups of one query: the
//                       k reference rows are read 16 bytes at a time where x, ldx and C allow, scalar otherwise (any C >= 1).
// Plain vector loads and stores, no atomics: the outputs are a function of the inputs only.
//
// The backward (csrc/interp_math.h: coef / pick / bwd4) is a transposed, ordered sum -- no floating-point atomics anywhere:
//   transpose_*_kernel   the in-edge lists of every reference row, the shape of csc.hip: count (integer atomics, one thread per
//                        slot), exclusive scan over ALL reference rows of the call (list_scan.h: per-1024-row sums, then every block adds
//                        the sums before it: the base of a pair is the valid slots of the earlier pairs), unordered fill (integer
//                        cursors), then the ranking: ONE FILL POSITION PER THREAD -- it finds its list through idx[e] and counts
//                        the smaller entries of that list.  A list here can hold thousands of entries (a 200 k-vertex mesh
//                        against 1024 samples: ~600 a row; a one-point cloud: every query), so the L^2 comparisons of a long list
//                        are spread over the grid, L a thread, instead of one list per wave as csc_rank_kernel does.  The lists
//                        come out in ascending edge id whatever order the atomics ran in: a function of the inputs only.
//   cross_bwd_kernel<InterpT>     thread = (reference row, group of 4 channels) on the grid (chunks of 256 / (C/4) reference rows
//                        up to max_ref_cloud: about one item a thread) x (cloud pairs); it walks the row's in-edges in order,
//                        four loads in flight, and reads g 16 bytes at a time where g, ldg and C allow, scalar otherwise.
//                        Gather-bound, the cost of a thread is its list length.
#include "common.h"
#include "cross_stage.h"
#include "interp_math.h"
#include "list_scan.h"

namespace {
using dccross::THREADS;

constexpr int IT_TILE = 2048;                 // reference points staged per LDS tile: 3 x 2048 x 4 B = 24 KiB

template <int K>
__global__ __launch_bounds__(THREADS) void knn_cross_kernel(const float* __restrict__ query, const int64_t* __restrict__ qptr,
                                                            const float* __restrict__ ref, const int64_t* __restrict__ rptr,
                                                            int k, int32_t* __restrict__ idx, float* __restrict__ d2) {
    __shared__ float tx[IT_TILE], ty[IT_TILE], tz[IT_TILE];
    const int tid = threadIdx.x;
    const auto [qbase, nq, rbase, nr] = dccross::pair_span(qptr, rptr);
    const long long q0 = (long long)blockIdx.x * THREADS;
    if (q0 >= nq) return;                     // block-uniform (covers nq <= 0)
    const long long q = q0 + tid;
    const bool active = q < nq;

    float px = 0.f, py = 0.f, pz = 0.f;
    if (active) {
        const float* p = query + 3 * (qbase + q);
        px = p[0];
        py = p[1];
        pz = p[2];
    }
    dcinterp::TopK<K> best;
    best.init();

    for (long long t0 = 0; t0 < nr; t0 += IT_TILE) {
        const int tn = (int)(nr - t0 < IT_TILE ? nr - t0 : IT_TILE);
        __syncthreads();                      // the previous tile's readers are done
#pragma clang loop vectorize(disable)                  // (vectorised, the staging costs 23 VGPRs and a wave of occupancy at K = 16)
        for (int c = tid; c < tn; c += THREADS) {
            const float* p = ref + 3 * (rbase + t0 + c);
            tx[c] = p[0];
            ty[c] = p[1];
            tz[c] = p[2];
        }
        __syncthreads();
        if (active) {
            for (int c = 0; c < tn; ++c) best.push(dcinterp::dist2(px, py, pz, tx[c], ty[c], tz[c]), (int)t0 + c);
        }
    }
    if (active) {
        int32_t* oi = idx + (qbase + q) * k;
        float* od = d2 + (qbase + q) * k;
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s < k) {
                oi[s] = best.id[s];
                od[s] = best.d[s];
            }
    }
}

// The inverse-squared-distance mean of a query's k reference rows (cross_stage.h: cross_fwd_kernel).
struct InterpF {
    static constexpr int ROWS = 1;
    const float* __restrict__ x;
    long long ldx;
    int k;
    const int32_t* __restrict__ idx;
    const float* __restrict__ d2;
    __device__ __forceinline__ void operator()(const dccross::Span& p, long long row, int c0, int nc, bool vec, float (*v)[4]) const {
        dcinterp::interp4(x + p.rbase * ldx, ldx, p.nr, k, idx + row * k, d2 + row * k, c0, nc, vec, v[0]);
    }
};

// ---- backward: transposed lists -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void transpose_count_kernel(const int64_t* __restrict__ qptr,
                                                                  const int64_t* __restrict__ rptr, int B, int k,
                                                                  const int32_t* __restrict__ idx, long long ne,
                                                                  long long num_ref, u64* __restrict__ cnt) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= ne) return;
    const long long r = dcinterp::pick(qptr, rptr, B, k, idx, e);
    if (r >= 0 && r < num_ref) atomicAdd(cnt + r, 1ull);
}

__global__ __launch_bounds__(THREADS) void transpose_fill_kernel(const int64_t* __restrict__ qptr,
                                                                 const int64_t* __restrict__ rptr, int B, int k,
                                                                 const int32_t* __restrict__ idx, long long ne,
                                                                 long long num_ref, u64* __restrict__ cursor,
                                                                 int64_t* __restrict__ unordered) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= ne) return;
    const long long r = dcinterp::pick(qptr, rptr, B, k, idx, e);
    if (r < 0 || r >= num_ref) return;
    const u64 at = atomicAdd(cursor + r, 1ull);
    if (at < (u64)ne) unordered[at] = e;      // (always: the counts came from the same inputs)
}

__global__ __launch_bounds__(THREADS) void transpose_rank_kernel(const int64_t* __restrict__ qptr,
                                                                 const int64_t* __restrict__ rptr, int B, int k,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ d2,
                                                                 long long ne, long long num_ref,
                                                                 const int64_t* __restrict__ tptr,
                                                                 const int64_t* __restrict__ unordered,
                                                                 int64_t* __restrict__ tedge, float* __restrict__ tcoef) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= ne || t >= tptr[num_ref]) return;
    const long long e = unordered[t];
    if (e < 0 || e >= ne) return;
    const long long q = e / k;
    const int s = (int)(e - q * k);
    const int b = dcinterp::pair_of(qptr, B, q);
    if (b < 0) return;
    const long long rbase = rptr[b], nr = rptr[b + 1] - rbase, j = idx[e];
    if (!dcinterp::valid_slot(j, nr) || rbase + j >= num_ref) return;
    long long lo = tptr[rbase + j], hi = tptr[rbase + j + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > ne ? ne : hi;
    long long rank = 0;
#pragma unroll 8
    for (long long p = lo; p < hi; ++p) rank += unordered[p] < e;
    if (lo + rank >= hi) return;              // (never: e is one of the list's distinct entries)
    tedge[lo + rank] = e;
    tcoef[lo + rank] = dcinterp::coef(nr, k, idx + q * k, d2 + q * k, s);
}

// The ordered sum over a reference row's in-edges (cross_stage.h: cross_bwd_kernel).
struct InterpT {
    static constexpr int ROWS = 1;
    const float* __restrict__ g;
    long long ldg, g_rows;
    int k;
    long long edge_base;
    const int64_t* __restrict__ tedge;
    const float* __restrict__ tcoef;
    __device__ __forceinline__ void operator()(long long lo, long long n, int c0, int nc, bool vec, float (*v)[4]) const {
        dcinterp::bwd4(g, ldg, g_rows, k, edge_base, tedge + lo, tcoef + lo, n, c0, nc, vec, v[0]);
    }
};

constexpr long long TR_MAX_EDGES = dccross::MAX_ITEMS;                        // one thread per slot
constexpr long long TR_MAX_REF = (1ll << 31) * SC_THREADS - SC_THREADS;

size_t transpose_bytes(long long num_query, long long num_ref, int k) {
    return 8 * ((size_t)num_ref + (size_t)dc_cdiv(num_ref, SC_THREADS) + (size_t)num_query * (size_t)k);
}

template <int K>
int launch_cross(const float* query, const int64_t* qptr, const float* ref, const int64_t* rptr, int B, long long max_q, int k,
                 int32_t* idx, float* d2, hipStream_t s) {
    hipLaunchKernelGGL((knn_cross_kernel<K>), dim3(dc_cdiv(max_q, THREADS), B), dim3(THREADS), 0, s, query, qptr, ref, rptr, k,
                       idx, d2);
    DC_CHECK_LAUNCH("dc_knn_cross");
    return DC_OK;
}

}  // namespace

DC_EXPORT int dc_knn_cross(const float* query, const int64_t* qptr, const float* ref, const int64_t* rptr, int32_t B,
                           int64_t max_query_cloud, int32_t k, int32_t* idx, float* d2, void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_cross: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_cross: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= dccross::MAX_ITEMS,
               "dc_knn_cross: max_query_cloud = %lld outside [0, 2^39)", (long long)max_query_cloud);
    if (B == 0 || max_query_cloud == 0) return DC_OK;
    DC_REQUIRE(query && qptr && ref && rptr && idx && d2, "dc_knn_cross: null pointer (query, qptr, ref, rptr, idx, d2)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (k == 1) return launch_cross<1>(query, qptr, ref, rptr, B, max_query_cloud, k, idx, d2, s);
    if (k <= 4) return launch_cross<4>(query, qptr, ref, rptr, B, max_query_cloud, k, idx, d2, s);
    if (k <= 8) return launch_cross<8>(query, qptr, ref, rptr, B, max_query_cloud, k, idx, d2, s);
    return launch_cross<16>(query, qptr, ref, rptr, B, max_query_cloud, k, idx, d2, s);
}

DC_EXPORT int dc_knn_interpolate(const float* x, int64_t ldx, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                                 int64_t max_query_cloud, int32_t k, const int32_t* idx, const float* d2, float* out, int64_t ldo,
                                 void* stream) {
    const dccross::Call c{"dc_knn_interpolate", "ldx", "out", "ldo", "x, qptr, rptr, idx, d2, out", idx && d2, nullptr};
    return dccross::launch_fwd(c, x, ldx, C, qptr, rptr, B, max_query_cloud, k, out, ldo, InterpF{x, ldx, k, idx, d2}, stream);
}

// workspace: the counters / fill cursors [num_ref], the scan's block sums and the unordered fill [num_query * k], 8 bytes each
DC_EXPORT size_t dc_knn_cross_transpose_workspace_bytes(int64_t num_query, int64_t num_ref, int32_t k) {
    if (num_query < 0 || num_ref < 0 || k < 1 || k > dcinterp::MAX_K || num_query * k > TR_MAX_EDGES || num_ref > TR_MAX_REF)
        return 0;
    return transpose_bytes(num_query, num_ref, k);
}

DC_EXPORT int dc_knn_cross_transpose(const int64_t* qptr, const int64_t* rptr, int32_t B, int64_t num_query, int64_t num_ref,
                                     int32_t k, const int32_t* idx, const float* d2, int64_t* tptr, int64_t* tedge, float* tcoef,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    DC_REQUIRE(B >= 0, "dc_knn_cross_transpose: B = %d cloud pairs", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_cross_transpose: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(num_query >= 0 && num_query * k <= TR_MAX_EDGES, "dc_knn_cross_transpose: num_query = %lld: num_query * k outside [0, 2^39)",
               (long long)num_query);
    DC_REQUIRE(num_ref >= 0 && num_ref <= TR_MAX_REF, "dc_knn_cross_transpose: num_ref = %lld outside [0, 2^41)", (long long)num_ref);
    DC_REQUIRE(tptr, "dc_knn_cross_transpose: null pointer (tptr)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long ne = (long long)num_query * k;
    if (B == 0 || ne == 0 || num_ref == 0) {  // no in-edge at all: every list is empty
        dc_zero_words(tptr, 2 * ((long)num_ref + 1), s);
        DC_CHECK_LAUNCH("dc_knn_cross_transpose");
        return DC_OK;
    }
    DC_REQUIRE(qptr && rptr && idx && d2 && tedge && tcoef, "dc_knn_cross_transpose: null pointer (qptr, rptr, idx, d2, tedge, tcoef)");
    DC_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= transpose_bytes(num_query, num_ref, k),
               "dc_knn_cross_transpose: workspace null, not 8-byte aligned or too small (%zu bytes, needs %zu)", workspace_bytes,
               transpose_bytes(num_query, num_ref, k));
    const int sblocks = dc_cdiv(num_ref, SC_THREADS), eblocks = dc_cdiv(ne, THREADS);
    u64* cnt = static_cast<u64*>(workspace);
    u64* part = cnt + num_ref;
    int64_t* unordered = reinterpret_cast<int64_t*>(part + sblocks);
    dc_zero_words(cnt, 2 * (long)num_ref, s);
    hipLaunchKernelGGL(transpose_count_kernel, dim3(eblocks), dim3(THREADS), 0, s, qptr, rptr, (int)B, (int)k, idx, ne,
                       (long long)num_ref, cnt);
    hipLaunchKernelGGL(list_sum_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, (long long)num_ref, part);
    hipLaunchKernelGGL(list_scan_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, (long long)num_ref, part, tptr);
    hipLaunchKernelGGL(transpose_fill_kernel, dim3(eblocks), dim3(THREADS), 0, s, qptr, rptr, (int)B, (int)k, idx, ne,
                       (long long)num_ref, cnt, unordered);
    hipLaunchKernelGGL(transpose_rank_kernel, dim3(eblocks), dim3(THREADS), 0, s, qptr, rptr, (int)B, (int)k, idx, d2, ne,
                       (long long)num_ref, tptr, unordered, tedge, tcoef);
    DC_CHECK_LAUNCH("dc_knn_cross_transpose");
    return DC_OK;
}

DC_EXPORT int dc_knn_interpolate_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                                          int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge,
                                          const float* tcoef, int64_t num_edges, int64_t edge_base, float* dx, int64_t ldx,
                                          void* stream) {
    const dccross::Call c{"dc_knn_interpolate_backward", "ldg", "dx", "ldx", "g, tedge, tcoef", tedge && tcoef, nullptr};
    return dccross::launch_bwd(c, g, ldg, num_g_rows, C, rptr, B, max_ref_cloud, k, tptr, num_edges, false, dx, ldx,
                               InterpT{g, ldg, num_g_rows, k, edge_base, tedge, tcoef}, stream);
}
