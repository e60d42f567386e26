// Two-set nearest-neighbour search and inverse-squared-distance interpolation, batched over cloud pairs -- replaces
// torch_cluster.knn(x, y, k, batch_x, batch_y) and torch_geometric.nn.knn_interpolate (PointNet++ feature propagation): the way
// back up from a sampled cloud to the points or vertices it was sampled from.  Inference only: no backward kernel.
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
#include "common.h"
#include "interp_math.h"

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
