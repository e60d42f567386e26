// Geodesic farthest-point sampling of a batch of clouds on the device: what the reference's data preparation does on the host one
// shape at a time (deltaconv/transforms/geodesic_fps.py:14-43 over deltaconv/cpp/sampling.cpp:5-81; here csrc_host/fps.cpp) --
// the k = 10 nearest-neighbour graph, then n_samples - 1 rounds of "shortest paths from the last sample, lower D, take the first
// index of max(D)".  Two launches:
//   fps_knn_kernel     one thread per query point, candidates staged through LDS in tiles, the ten best (d2, j) in registers; writes
//                      the neighbours and the fp64 edge lengths to the workspace
//   fps_sample_kernel  one workgroup per cloud, every round inside the launch.  D lives in LDS as fp64 bit patterns.  In place of the
//                      host's Dijkstra a round relaxes edges until nothing changes (label correcting): D[src] = 0, then sweeps over
//                      the vertices whose D was lowered in the sweep before.  Every value written is the left-to-right fp64 sum
//                      along a real path, fp64 addition is monotone, and the D of the round before is closed under relaxation, so
//                      the fixed point is min(D_old, shortest path from src) -- the host's D, bit for bit, whatever the order.
//                      Concurrent relaxations of one vertex meet in an unsigned 64-bit LDS minimum: non-negative doubles order like
//                      their bit patterns, and a minimum does not depend on the order of its operands.
//   fps_sample_global_kernel  the same rounds for clouds above that kernel's cap (dc_geodesic_fps_large): D lives in the
//                      workspace, only the two frontier bit sets stay in LDS.  Concurrent relaxations meet in an unsigned 64-bit
//                      minimum that executes at L2, so EVERY access to D after its initialisation is an agent-scope atomic (a
//                      plain load could be served from a vector-L1 line fetched before a minimum landed: a missed fixed point).
//                      The frontier is scanned by word, zero words skipped; the order of relaxations does not change the fixed point.
// No floating-point atomics, and the only global atomics are integer minima whose result does not depend on their order: the picks
// are a function of the inputs only.
// LDS of fps_sample_kernel: 8 n bytes of D + two frontier bit sets of n / 8 bytes = 132 KiB at the cap of 16 384 points;
// of fps_sample_global_kernel: the two bit sets alone = 64 KiB at the cap of 262 144 points.
#include "common.h"
#include "fps_math.h"

namespace {

constexpr int FK = dcfps::K;
constexpr int KNN_T = 256;                    // queries of a workgroup = candidates of a tile
typedef unsigned long long u64;

template <typename T>
__global__ __launch_bounds__(KNN_T) void fps_knn_kernel(const T* __restrict__ pos, const int64_t* __restrict__ ptr,
                                                        int32_t* __restrict__ nbr, double* __restrict__ w) {
    __shared__ double tile[KNN_T * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long base = ptr[b];
    const int n = (int)(ptr[b + 1] - base);
    const int q0 = blockIdx.x * KNN_T;
    if (q0 >= n) return;                       // the whole workgroup: no barrier is left behind
    const int i = q0 + tid;
    const bool live = i < n;
    double px = 0, py = 0, pz = 0;
    if (live) {
        const T* p = pos + 3 * (base + i);
        px = (double)p[0]; py = (double)p[1]; pz = (double)p[2];
    }
    double d[FK];
    int id[FK];
    dcfps::topk_clear(d, id);
    for (int j0 = 0; j0 < n; j0 += KNN_T) {
        const int nj = n - j0 < KNN_T ? n - j0 : KNN_T;
        __syncthreads();                       // the scan of the tile before is over
        for (int e = tid; e < 3 * nj; e += KNN_T) tile[e] = (double)pos[3 * (base + j0) + e];
        __syncthreads();
        if (live) {
            for (int t = 0; t < nj; ++t) {
                const int j = j0 + t;
                const double d2 = dcfps::dist2(px, py, pz, tile[3 * t], tile[3 * t + 1], tile[3 * t + 2]);
                if (j != i) dcfps::topk_insert(d, id, d2, j);
            }
        }
    }
    if (live) {
        const long long o = (base + i) * FK;
#pragma unroll
        for (int s = 0; s < FK; ++s) {         // slots past min(10, n - 1) stay (-1, +inf) and are never read
            nbr[o + s] = id[s];
            w[o + s] = sqrt(d[s]);
        }
    }
}

__global__ __launch_bounds__(1024) void fps_sample_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ nbr, const double* __restrict__ w,
                                                          int32_t* __restrict__ out, int n_samples) {
    extern __shared__ u64 s_dyn[];
    __shared__ double s_val[16];
    __shared__ int s_idx[16];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    const long long base = ptr[b];
    const int n = (int)(ptr[b + 1] - base);
    const int kk = n - 1 < FK ? n - 1 : FK;
    const int words = (n + 31) >> 5;
    u64* D = s_dyn;                                                  // [n] fp64 bit patterns
    unsigned* cur = reinterpret_cast<unsigned*>(s_dyn + n);          // [words] vertices lowered in the sweep before
    unsigned* nxt = cur + words;                                     // [words] vertices lowered in this sweep
    const int32_t* nb = nbr + base * FK;
    const double* wb = w + base * FK;
    for (int u = tid; u < n; u += T) D[u] = (u64)__double_as_longlong(dcfps::inf());
    for (int e = tid; e < 2 * words; e += T) cur[e] = 0u;
    int src = start[b];
    if (tid == 0) out[(long long)b * n_samples] = src;
    for (int r = 1; r < n_samples; ++r) {
        __syncthreads();                       // D and the bit sets are initialised / the arg-max of the round before has read D
        if (tid == 0) {
            D[src] = 0ull;
            cur[src >> 5] = 1u << (src & 31);
        }
        __syncthreads();
        for (;;) {
            int lowered = 0;
            for (int u = tid; u < n; u += T) {
                const unsigned bit = 1u << (u & 31);
                if (!(cur[u >> 5] & bit)) continue;
                atomicAnd(&cur[u >> 5], ~bit);
                const double du = __longlong_as_double((long long)__hip_atomic_load(&D[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                for (int s = 0; s < kk; ++s) {
                    const int v = nb[(long long)u * FK + s];
                    if (v < 0 || v >= n) continue;                   // a slot the graph kernel could not fill (NaN positions)
                    const u64 nd = (u64)__double_as_longlong(dcfps::relax(du, wb[(long long)u * FK + s]));
                    if (nd < atomicMin(&D[v], nd)) {
                        atomicOr(&nxt[v >> 5], 1u << (v & 31));
                        lowered = 1;
                    }
                }
            }
            const int any = __syncthreads_or(lowered);
            unsigned* t = cur; cur = nxt; nxt = t;                   // every bit of the old `cur` was cleared by its reader
            if (!any) break;
        }
        // first index of max(D): per thread in ascending order, then across lanes and waves with the (value, index) combine
        double bv = -1.0;
        int bi = 0x7fffffff;
        for (int u = tid; u < n; u += T) dcfps::argmax_combine(bv, bi, __longlong_as_double((long long)D[u]), u);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            dcfps::argmax_combine(bv, bi, ov, oi);
        }
        if (lane == 0) { s_val[wave] = bv; s_idx[wave] = bi; }
        __syncthreads();
        bv = s_val[0]; bi = s_idx[0];
        for (int k = 1; k < waves; ++k) dcfps::argmax_combine(bv, bi, s_val[k], s_idx[k]);
        src = bi;                                                    // the same in every thread
        if (tid == 0) out[(long long)b * n_samples + r] = src;
    }
}

// One workgroup of 1024 threads per cloud, any cloud of 1 .. LARGE_MAX_POINTS points.  D = Dall + ptr[b]: [n] fp64 bit patterns in
// global memory, touched by this workgroup only.
__global__ __launch_bounds__(1024) void fps_sample_global_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ start,
                                                                 const int32_t* __restrict__ nbr, const double* __restrict__ w,
                                                                 u64* Dall, int32_t* __restrict__ out, int n_samples) {
    extern __shared__ unsigned s_bits[];
    __shared__ double s_val[16];
    __shared__ int s_idx[16];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    const long long base = ptr[b];
    const int n = (int)(ptr[b + 1] - base);
    const int kk = n - 1 < FK ? n - 1 : FK;
    const int words = dcfps::bitset_words(n);
    u64* D = Dall + base;
    unsigned* cur = s_bits;                                          // [words] vertices lowered in the sweep before
    unsigned* nxt = cur + words;                                     // [words] vertices lowered in this sweep
    const int32_t* nb = nbr + base * FK;
    const double* wb = w + base * FK;
    const u64 inf_bits = (u64)__double_as_longlong(dcfps::inf());
    for (int u = tid; u < n; u += T) D[u] = inf_bits;                // plain stores, before the first atomic
    for (int e = tid; e < 2 * words; e += T) cur[e] = 0u;
    __threadfence();                                                 // once: the +inf are at L2 before any minimum or atomic load
    int src = start[b];
    if (tid == 0) out[(long long)b * n_samples] = src;
    for (int r = 1; r < n_samples; ++r) {
        __syncthreads();                       // D and the bit sets are initialised / the arg-max of the round before has read D
        if (tid == 0) {
            __hip_atomic_store(&D[src], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cur[src >> 5] = 1u << (src & 31);
        }
        __syncthreads();
        for (;;) {
            int lowered = 0;
            for (int wd = tid; wd < words; wd += T) {                // a word of `cur` has one reader, and no writer in this sweep
                unsigned bits = cur[wd];
                if (!bits) continue;
                cur[wd] = 0u;
                do {
                    const int u = (wd << 5) + __builtin_ctz(bits);   // u < n: only bits of vertices are ever set
                    bits &= bits - 1;
                    const double du = __longlong_as_double((long long)__hip_atomic_load(&D[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    // all loads of a vertex in flight together; D only falls, so a candidate not below the value read now is not
                    // below the value a minimum would meet: it is dropped without one
                    int vs[FK];
                    u64 nd[FK], dv[FK];
#pragma unroll
                    for (int s = 0; s < FK; ++s) {
                        const int v = s < kk ? nb[(long long)u * FK + s] : -1;
                        const bool ok = v >= 0 && v < n;             // else a slot the graph kernel could not fill (NaN positions)
                        vs[s] = ok ? v : -1;
                        nd[s] = ok ? (u64)__double_as_longlong(dcfps::relax(du, wb[(long long)u * FK + s])) : 0ull;
                        dv[s] = ok ? __hip_atomic_load(&D[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                    }
#pragma unroll
                    for (int s = 0; s < FK; ++s) {
                        if (vs[s] < 0 || !(nd[s] < dv[s])) continue;
                        if (nd[s] < __hip_atomic_fetch_min(&D[vs[s]], nd[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                            atomicOr(&nxt[vs[s] >> 5], 1u << (vs[s] & 31));
                            lowered = 1;
                        }
                    }
                } while (bits);
            }
            const int any = __syncthreads_or(lowered);               // every minimum above has returned: its value was used
            unsigned* t = cur; cur = nxt; nxt = t;                   // every word of the old `cur` was cleared by its reader
            if (!any) break;
        }
        // first index of max(D): per thread in ascending order, then across lanes and waves with the (value, index) combine
        double bv = -1.0;
        int bi = 0x7fffffff;
        for (int u = tid; u < n; u += T)
            dcfps::argmax_combine(bv, bi, __longlong_as_double((long long)__hip_atomic_load(&D[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)), u);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            dcfps::argmax_combine(bv, bi, ov, oi);
        }
        if (lane == 0) { s_val[wave] = bv; s_idx[wave] = bi; }
        __syncthreads();
        bv = s_val[0]; bi = s_idx[0];
        for (int k = 1; k < waves; ++k) dcfps::argmax_combine(bv, bi, s_val[k], s_idx[k]);
        src = bi;                                                    // the same in every thread
        if (tid == 0) out[(long long)b * n_samples + r] = src;
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Both entry points: the same checks (all in front of the first device call), the same graph launch, then the sampling kernel of
// the size class.  `fn`: the entry's name for messages; `large`: D in the workspace and the cap of fps_sample_global_kernel.
int fps_run(const char* fn, bool large, const void* pos, int32_t pos_is_f64, const int64_t* ptr, int32_t B, int32_t max_cloud_size,
            int32_t n_samples, const int32_t* start, int32_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    const int cap = large ? dcfps::LARGE_MAX_POINTS : dcfps::MAX_POINTS;
    const char* cap_name = large ? "DC_FPS_LARGE_MAX_POINTS" : "DC_FPS_MAX_POINTS";
    DC_REQUIRE(B >= 0 && B <= 65535, "%s: B = %d clouds, supported: 0 .. 65535 per launch", fn, B);
    DC_REQUIRE(n_samples >= 1, "%s: n_samples = %d, at least 1", fn, n_samples);
    if (B == 0) return DC_OK;
    DC_REQUIRE(pos && ptr && start && out && workspace, "%s: null pointer (pos, ptr, start, out, workspace)", fn);
    DC_REQUIRE(ptr[0] == 0, "%s: ptr[0] = %lld, the offsets start at 0 (row 0 of pos)", fn, (long long)ptr[0]);
    int largest = 0;
    for (int b = 0; b < B; ++b) {
        const long long n = ptr[b + 1] - ptr[b];
        DC_REQUIRE(n >= 1, "%s: cloud %d is empty (ptr %lld .. %lld)", fn, b, (long long)ptr[b], (long long)ptr[b + 1]);
        DC_REQUIRE(n <= cap, "%s: cloud %d has %lld points, the device sampler takes at most %d (%s)", fn, b, n, cap, cap_name);
        DC_REQUIRE(start[b] >= 0 && start[b] < n, "%s: start[%d] = %d outside its cloud of %lld points", fn, b, start[b], n);
        if (n > largest) largest = (int)n;
    }
    DC_REQUIRE(max_cloud_size >= largest && max_cloud_size <= cap,
               "%s: max_cloud_size = %d, the largest cloud has %d points, the cap is %d", fn, max_cloud_size, largest, cap);
    const long long N = ptr[B];
    const unsigned long long need = large ? dcfps::large_workspace_bytes(N) : dcfps::workspace_bytes(N);
    if (workspace_bytes < need) {
        dc_set_error("%s: workspace of %zu bytes, %llu needed for %lld points", fn, workspace_bytes, need, N);
        return DC_ERR_WORKSPACE;
    }
    DC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", fn);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // workspace: edge lengths | neighbours | offsets | start points | (large) distance patterns
    char* ws = static_cast<char*>(workspace);
    double* w = reinterpret_cast<double*>(ws);
    ws += align256((size_t)N * FK * 8);
    int32_t* nbr = reinterpret_cast<int32_t*>(ws);
    ws += align256((size_t)N * FK * 4);
    int64_t* d_ptr = reinterpret_cast<int64_t*>(ws);
    ws += align256((size_t)(B + 1) * 8);
    int32_t* d_start = reinterpret_cast<int32_t*>(ws);
    ws += align256((size_t)B * 4);
    u64* D = reinterpret_cast<u64*>(ws);                             // [N], read and written by the large kernel only
    // ptr and start are host arrays (the checks above read them): uploaded in stream order
    if (hipMemcpyAsync(d_ptr, ptr, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_start, start, (size_t)B * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
        dc_set_error("%s: upload of ptr / start: %s", fn, hipGetErrorString(hipGetLastError()));
        return DC_ERR_LAUNCH;
    }
    const dim3 kgrid(dc_cdiv(largest, KNN_T), B);
    if (pos_is_f64)
        hipLaunchKernelGGL(fps_knn_kernel<double>, kgrid, dim3(KNN_T), 0, s, static_cast<const double*>(pos), d_ptr, nbr, w);
    else
        hipLaunchKernelGGL(fps_knn_kernel<float>, kgrid, dim3(KNN_T), 0, s, static_cast<const float*>(pos), d_ptr, nbr, w);
    char what[64];
    snprintf(what, sizeof what, "%s (graph)", fn);
    DC_CHECK_LAUNCH(what);
    if (large) {
        static unsigned long long attr_done_large = 0;
        if (!dc_ensure_lds(&attr_done_large, reinterpret_cast<const void*>(&fps_sample_global_kernel),
                           (size_t)dcfps::large_lds_bytes(dcfps::LARGE_MAX_POINTS), fn)) {
            DC_CHECK_LAUNCH(fn);
        }
        hipLaunchKernelGGL(fps_sample_global_kernel, dim3(B), dim3(1024), (size_t)dcfps::large_lds_bytes(largest), s, d_ptr, d_start,
                           nbr, w, D, out, n_samples);
    } else {
        const int threads = largest <= 256 ? 64 : (largest <= 2048 ? 256 : 1024);
        const size_t lds = (size_t)largest * 8 + (size_t)((largest + 31) / 32) * 8;
        static unsigned long long attr_done = 0;
        if (!dc_ensure_lds(&attr_done, reinterpret_cast<const void*>(&fps_sample_kernel),
                           (size_t)dcfps::MAX_POINTS * 8 + (size_t)(dcfps::MAX_POINTS / 32) * 8, fn)) {
            DC_CHECK_LAUNCH(fn);
        }
        hipLaunchKernelGGL(fps_sample_kernel, dim3(B), dim3(threads), lds, s, d_ptr, d_start, nbr, w, out, n_samples);
    }
    snprintf(what, sizeof what, "%s (sampling)", fn);
    DC_CHECK_LAUNCH(what);
    return DC_OK;
}

}  // namespace

DC_EXPORT size_t dc_geodesic_fps_workspace_bytes(int64_t N) { return (size_t)dcfps::workspace_bytes(N); }
DC_EXPORT size_t dc_geodesic_fps_large_workspace_bytes(int64_t N) { return (size_t)dcfps::large_workspace_bytes(N); }

DC_EXPORT int dc_geodesic_fps_batch(const void* pos, int32_t pos_is_f64, const int64_t* ptr, int32_t B, int32_t max_cloud_size,
                                    int32_t n_samples, const int32_t* start, int32_t* out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    return fps_run("dc_geodesic_fps_batch", false, pos, pos_is_f64, ptr, B, max_cloud_size, n_samples, start, out, workspace,
                   workspace_bytes, stream);
}

DC_EXPORT int dc_geodesic_fps_large(const void* pos, int32_t pos_is_f64, const int64_t* ptr, int32_t B, int32_t max_cloud_size,
                                    int32_t n_samples, const int32_t* start, int32_t* out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    return fps_run("dc_geodesic_fps_large", true, pos, pos_is_f64, ptr, B, max_cloud_size, n_samples, start, out, workspace,
                   workspace_bytes, stream);
}
