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
// end returns, block-uniformly:
//   knn_cross_kernel    one query per thread.  The reference cloud is staged through LDS in SoA tiles of 2048 points (24 KiB)
//                       and read as broadcasts; the sorted top-K list lives in registers (the sorted-insertion kernel of knn.hip,
//                       P = 1), K in {1, 4, 8, 16} by dispatch.  VALU-bound: Nq x Nr distance evaluations per pair.
//   interpolate_kernel  thread = (query, group of 4 channels), consecutive threads on consecutive groups of one query: the k
//                       reference rows are read 16 bytes at a time where x, ldx and C allow, scalar otherwise (any C >= 1).
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
//   interpolate_backward_kernel   thread = (reference row, group of 4 channels) on the grid (chunks of 256 / (C/4) reference rows
//                        up to max_ref_cloud: about one item a thread) x (cloud pairs); it walks the row's in-edges in order,
//                        four loads in flight, and reads g 16 bytes at a time where g, ldg and C allow, scalar otherwise.
//                        Gather-bound, the cost of a thread is its list length.
#include "common.h"
#include "interp_math.h"
#include "list_scan.h"

namespace {

constexpr int IT_THREADS = 256;               // queries of a workgroup
constexpr int IT_TILE = 2048;                 // reference points staged per LDS tile: 3 x 2048 x 4 B = 24 KiB
constexpr long long IT_MAX_REF = 0x7fffffffll;   // idx is int32, local to the reference cloud

template <int K>
__global__ __launch_bounds__(IT_THREADS) void knn_cross_kernel(const float* __restrict__ query, const int64_t* __restrict__ qptr,
                                                               const float* __restrict__ ref, const int64_t* __restrict__ rptr,
                                                               int k, int32_t* __restrict__ idx, float* __restrict__ d2) {
    __shared__ float tx[IT_TILE], ty[IT_TILE], tz[IT_TILE];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long qbase = qptr[b], nq = qptr[b + 1] - qbase;
    const long long rbase = rptr[b];
    long long nr = rptr[b + 1] - rbase;
    nr = nr < 0 ? 0 : (nr > IT_MAX_REF ? IT_MAX_REF : nr);
    const long long q0 = (long long)blockIdx.x * IT_THREADS;
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
        for (int c = tid; c < tn; c += IT_THREADS) {
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

__global__ __launch_bounds__(IT_THREADS) void interpolate_kernel(const float* __restrict__ x, long long ldx, int C,
                                                                 const int64_t* __restrict__ qptr,
                                                                 const int64_t* __restrict__ rptr, int k,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ d2,
                                                                 float* __restrict__ out, long long ldo, int vec_in, int vec_out) {
    const int b = blockIdx.y;
    const long long qbase = qptr[b], nq = qptr[b + 1] - qbase;
    const long long rbase = rptr[b];
    long long nr = rptr[b + 1] - rbase;
    nr = nr < 0 ? 0 : (nr > IT_MAX_REF ? IT_MAX_REF : nr);
    const long long q0 = (long long)blockIdx.x * IT_THREADS;
    if (q0 >= nq) return;                     // block-uniform
    const int rows = (int)(nq - q0 < IT_THREADS ? nq - q0 : IT_THREADS);
    const int groups = (C + 3) >> 2;
    const float* xr = x + rbase * ldx;        // the rows of this pair's reference cloud
    for (int item = threadIdx.x; item < rows * groups; item += IT_THREADS) {
        const int r = item / groups, g = item - r * groups;
        const long long row = qbase + q0 + r;
        const int c0 = 4 * g, nc = C - c0 < 4 ? C - c0 : 4;
        float v[4];
        dcinterp::interp4(xr, ldx, nr, k, idx + row * k, d2 + row * k, c0, nc, vec_in && nc == 4, v);
        float* o = out + row * ldo + c0;
        if (vec_out && nc == 4) {
            dc_f32x4 t = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<dc_f32x4*>(o) = t;
        } else {
            for (int c = 0; c < nc; ++c) o[c] = v[c];
        }
    }
}

// ---- backward: transposed lists -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IT_THREADS) void transpose_count_kernel(const int64_t* __restrict__ qptr,
                                                                     const int64_t* __restrict__ rptr, int B, int k,
                                                                     const int32_t* __restrict__ idx, long long ne,
                                                                     long long num_ref, u64* __restrict__ cnt) {
    const long long e = (long long)blockIdx.x * IT_THREADS + threadIdx.x;
    if (e >= ne) return;
    const long long r = dcinterp::pick(qptr, rptr, B, k, idx, e);
    if (r >= 0 && r < num_ref) atomicAdd(cnt + r, 1ull);
}

__global__ __launch_bounds__(IT_THREADS) void transpose_fill_kernel(const int64_t* __restrict__ qptr,
                                                                    const int64_t* __restrict__ rptr, int B, int k,
                                                                    const int32_t* __restrict__ idx, long long ne,
                                                                    long long num_ref, u64* __restrict__ cursor,
                                                                    int64_t* __restrict__ unordered) {
    const long long e = (long long)blockIdx.x * IT_THREADS + threadIdx.x;
    if (e >= ne) return;
    const long long r = dcinterp::pick(qptr, rptr, B, k, idx, e);
    if (r < 0 || r >= num_ref) return;
    const u64 at = atomicAdd(cursor + r, 1ull);
    if (at < (u64)ne) unordered[at] = e;      // (always: the counts came from the same inputs)
}

__global__ __launch_bounds__(IT_THREADS) void transpose_rank_kernel(const int64_t* __restrict__ qptr,
                                                                    const int64_t* __restrict__ rptr, int B, int k,
                                                                    const int32_t* __restrict__ idx, const float* __restrict__ d2,
                                                                    long long ne, long long num_ref,
                                                                    const int64_t* __restrict__ tptr,
                                                                    const int64_t* __restrict__ unordered,
                                                                    int64_t* __restrict__ tedge, float* __restrict__ tcoef) {
    const long long t = (long long)blockIdx.x * IT_THREADS + threadIdx.x;
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

__global__ __launch_bounds__(IT_THREADS) void interpolate_backward_kernel(const float* __restrict__ g, long long ldg,
                                                                          long long g_rows, int C,
                                                                          const int64_t* __restrict__ rptr, int k,
                                                                          const int64_t* __restrict__ tptr,
                                                                          const int64_t* __restrict__ tedge,
                                                                          const float* __restrict__ tcoef, long long num_edges,
                                                                          long long edge_base, float* __restrict__ dx,
                                                                          long long ldx, int rpb, int vec_in, int vec_out) {
    const int b = blockIdx.y;
    const long long rbase = rptr[b], nr = rptr[b + 1] - rbase;
    const long long r0 = (long long)blockIdx.x * rpb;
    if (r0 >= nr) return;                     // block-uniform (covers nr <= 0)
    const int rows = (int)(nr - r0 < rpb ? nr - r0 : rpb);
    const int groups = (C + 3) >> 2;
    for (int item = threadIdx.x; item < rows * groups; item += IT_THREADS) {
        const int r = item / groups, gi = item - r * groups;
        const long long row = rbase + r0 + r;
        const int c0 = 4 * gi, nc = C - c0 < 4 ? C - c0 : 4;
        long long lo = tptr[row], hi = tptr[row + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > num_edges ? num_edges : hi;
        float v[4];
        dcinterp::bwd4(g, ldg, g_rows, k, edge_base, tedge + lo, tcoef + lo, hi > lo ? hi - lo : 0, c0, nc, vec_in && nc == 4, v);
        float* o = dx + row * ldx + c0;
        if (vec_out && nc == 4) {
            dc_f32x4 t = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<dc_f32x4*>(o) = t;
        } else {
            for (int c = 0; c < nc; ++c) o[c] = v[c];
        }
    }
}

constexpr long long TR_MAX_EDGES = (1ll << 31) * IT_THREADS - IT_THREADS;     // one thread per slot: at most 2^31 - 1 blocks
constexpr long long TR_MAX_REF = (1ll << 31) * SC_THREADS - SC_THREADS;

size_t transpose_bytes(long long num_query, long long num_ref, int k) {
    return 8 * ((size_t)num_ref + (size_t)dc_cdiv(num_ref, SC_THREADS) + (size_t)num_query * (size_t)k);
}

template <int K>
int launch_cross(const float* query, const int64_t* qptr, const float* ref, const int64_t* rptr, int B, long long max_q, int k,
                 int32_t* idx, float* d2, hipStream_t s) {
    hipLaunchKernelGGL((knn_cross_kernel<K>), dim3(dc_cdiv(max_q, IT_THREADS), B), dim3(IT_THREADS), 0, s, query, qptr, ref, rptr, k,
                       idx, d2);
    DC_CHECK_LAUNCH("dc_knn_cross");
    return DC_OK;
}

}  // namespace

DC_EXPORT int dc_knn_cross(const float* query, const int64_t* qptr, const float* ref, const int64_t* rptr, int32_t B,
                           int64_t max_query_cloud, int32_t k, int32_t* idx, float* d2, void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_cross: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_cross: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= (1ll << 31) * IT_THREADS - IT_THREADS,
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
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_interpolate: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_interpolate: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(C >= 1 && C <= (1 << 20), "dc_knn_interpolate: C = %d channels, supported: 1 .. 2^20", C);
    DC_REQUIRE(ldx >= C && ldo >= C, "dc_knn_interpolate: leading dimensions ldx = %lld, ldo = %lld below C = %d", (long long)ldx,
               (long long)ldo, C);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= (1ll << 31) * IT_THREADS - IT_THREADS,
               "dc_knn_interpolate: max_query_cloud = %lld outside [0, 2^39)", (long long)max_query_cloud);
    if (B == 0 || max_query_cloud == 0) return DC_OK;
    DC_REQUIRE(x && qptr && rptr && idx && d2 && out, "dc_knn_interpolate: null pointer (x, qptr, rptr, idx, d2, out)");
    const int vec_in = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (ldx & 3) == 0;
    const int vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (ldo & 3) == 0;
    hipLaunchKernelGGL(interpolate_kernel, dim3(dc_cdiv(max_query_cloud, IT_THREADS), B), dim3(IT_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, (long long)ldx, (int)C, qptr, rptr, (int)k, idx, d2, out, (long long)ldo,
                       vec_in, vec_out);
    DC_CHECK_LAUNCH("dc_knn_interpolate");
    return DC_OK;
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
    const int sblocks = dc_cdiv(num_ref, SC_THREADS), eblocks = dc_cdiv(ne, IT_THREADS);
    u64* cnt = static_cast<u64*>(workspace);
    u64* part = cnt + num_ref;
    int64_t* unordered = reinterpret_cast<int64_t*>(part + sblocks);
    dc_zero_words(cnt, 2 * (long)num_ref, s);
    hipLaunchKernelGGL(transpose_count_kernel, dim3(eblocks), dim3(IT_THREADS), 0, s, qptr, rptr, (int)B, (int)k, idx, ne,
                       (long long)num_ref, cnt);
    hipLaunchKernelGGL(list_sum_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, (long long)num_ref, part);
    hipLaunchKernelGGL(list_scan_kernel, dim3(sblocks), dim3(SC_THREADS), 0, s, cnt, (long long)num_ref, part, tptr);
    hipLaunchKernelGGL(transpose_fill_kernel, dim3(eblocks), dim3(IT_THREADS), 0, s, qptr, rptr, (int)B, (int)k, idx, ne,
                       (long long)num_ref, cnt, unordered);
    hipLaunchKernelGGL(transpose_rank_kernel, dim3(eblocks), dim3(IT_THREADS), 0, s, qptr, rptr, (int)B, (int)k, idx, d2, ne,
                       (long long)num_ref, tptr, unordered, tedge, tcoef);
    DC_CHECK_LAUNCH("dc_knn_cross_transpose");
    return DC_OK;
}

DC_EXPORT int dc_knn_interpolate_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                                          int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge,
                                          const float* tcoef, int64_t num_edges, int64_t edge_base, float* dx, int64_t ldx,
                                          void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_interpolate_backward: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "dc_knn_interpolate_backward: k = %d outside [1, %d]", k, dcinterp::MAX_K);
    DC_REQUIRE(C >= 1 && C <= (1 << 20), "dc_knn_interpolate_backward: C = %d channels, supported: 1 .. 2^20", C);
    DC_REQUIRE(ldg >= C && ldx >= C, "dc_knn_interpolate_backward: leading dimensions ldg = %lld, ldx = %lld below C = %d",
               (long long)ldg, (long long)ldx, C);
    DC_REQUIRE(max_ref_cloud >= 0 && max_ref_cloud < (1ll << 31),
               "dc_knn_interpolate_backward: max_ref_cloud = %lld outside [0, 2^31)", (long long)max_ref_cloud);
    DC_REQUIRE(num_g_rows >= 0 && num_edges >= 0, "dc_knn_interpolate_backward: num_g_rows = %lld, num_edges = %lld below 0",
               (long long)num_g_rows, (long long)num_edges);
    if (B == 0 || max_ref_cloud == 0) return DC_OK;
    DC_REQUIRE(rptr && tptr && dx, "dc_knn_interpolate_backward: null pointer (rptr, tptr, dx)");
    DC_REQUIRE((num_edges == 0 || num_g_rows == 0) || (g && tedge && tcoef),
               "dc_knn_interpolate_backward: null pointer (g, tedge, tcoef)");
    if (!g || !tedge || !tcoef) num_edges = 0;                   // nothing to read: every list is cut to nothing, dx gets zeros
    const int vec_in = (reinterpret_cast<uintptr_t>(g) & 15) == 0 && (ldg & 3) == 0;
    const int vec_out = (reinterpret_cast<uintptr_t>(dx) & 15) == 0 && (ldx & 3) == 0;
    // a thread's cost is its list length, so a workgroup takes only as many reference rows as give each thread about one item
    const int groups = (C + 3) >> 2, rpb = groups >= IT_THREADS ? 1 : IT_THREADS / groups;
    hipLaunchKernelGGL(interpolate_backward_kernel, dim3(dc_cdiv(max_ref_cloud, rpb), B), dim3(IT_THREADS), 0,
                       static_cast<hipStream_t>(stream), g, (long long)ldg, (long long)num_g_rows, (int)C, rptr, (int)k, tptr, tedge,
                       tcoef, (long long)num_edges, (long long)edge_base, dx, (long long)ldx, rpb, vec_in, vec_out);
    DC_CHECK_LAUNCH("dc_knn_interpolate_backward");
    return DC_OK;
}
