// The frame of the cross-cloud kernels (interp.hip, interp_transport.hip), on the pattern of ell_stage.h: which rows a workgroup
// owns, the (row, group of 4 channels) item loop and the 16-byte-or-scalar store live here once, with the argument checks of the
// apply entry points; the arithmetic of an item is a small functor over interp_math.h / interp_transport_math.h.
//
// Grid conventions: (chunks up to the largest cloud) x (cloud pairs), at most 65 535 pairs a launch; a workgroup past its cloud's
// end returns, block-uniformly.  Plain vector loads and stores, no atomics, no LDS: the outputs are a function of the inputs only.
//   cross_fwd_kernel   chunks of 256 query rows; thread = (query, group of 4 channels), consecutive threads on consecutive groups
//                      of one query
//   cross_bwd_kernel   chunks of rpb = 256 / (C/4) reference rows, about one item a thread (the cost of a thread is the length of
//                      its in-edge list); thread = (reference row, group of 4 channels), the list cut to [0, num_edges]
#pragma once
#include "common.h"
#include "interp_math.h"

namespace dccross {

constexpr int THREADS = 256;                                        // threads, and query rows or slots, of a workgroup
constexpr long long MAX_REF = 0x7fffffffll;                         // idx is int32, local to the reference cloud
constexpr long long MAX_ITEMS = (1ll << 31) * THREADS - THREADS;    // 256 items a workgroup, at most 2^31 - 1 workgroups: < 2^39

// The cloud pair of blockIdx.y: its first query / reference row and their counts, nr cut to what an int32 idx can name.
struct Span {
    long long qbase, nq, rbase, nr;
};
__device__ __forceinline__ Span pair_span(const int64_t* qptr, const int64_t* rptr) {
    const int b = blockIdx.y;
    const long long qbase = qptr[b], nq = qptr[b + 1] - qbase;
    const long long rbase = rptr[b], nr = rptr[b + 1] - rbase;
    return Span{qbase, nq, rbase, nr < 0 ? 0 : (nr > MAX_REF ? MAX_REF : nr)};
}

__device__ __forceinline__ void store4(float* o, const float* v, int nc, bool vec) {
    if (vec) {
        dc_f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<dc_f32x4*>(o) = t;
    } else {
        for (int c = 0; c < nc; ++c) o[c] = v[c];
    }
}

// BODY: ROWS output rows per query row (1: scalar features, 2: the two coefficients of a tangent vector), and
//   __device__ __forceinline__ void operator()(const Span& p, long long row, int c0, int nc, bool vec, float (*v)[4]) const
// fills channels c0 .. c0+nc-1 of the ROWS output rows of query row `row` (absolute) of pair p; vec: the rows it reads allow
// 16-byte loads and nc = 4.
template <class BODY>
__global__ __launch_bounds__(THREADS) void cross_fwd_kernel(const int64_t* __restrict__ qptr, const int64_t* __restrict__ rptr, int C,
                                                            float* __restrict__ out, long long ldo, int vec_in, int vec_out, BODY body) {
    const Span p = pair_span(qptr, rptr);
    const long long q0 = (long long)blockIdx.x * THREADS;
    if (q0 >= p.nq) return;                   // block-uniform (covers nq <= 0)
    const int rows = (int)(p.nq - q0 < THREADS ? p.nq - q0 : THREADS);
    const int groups = (C + 3) >> 2;
    for (int item = threadIdx.x; item < rows * groups; item += THREADS) {
        const int r = item / groups, g = item - r * groups;
        const long long row = p.qbase + q0 + r;
        const int c0 = 4 * g, nc = C - c0 < 4 ? C - c0 : 4;
        float v[BODY::ROWS][4];
        body(p, row, c0, nc, vec_in && nc == 4, v);
        float* o = out + (BODY::ROWS * row) * ldo + c0;
#pragma unroll
        for (int a = 0; a < BODY::ROWS; ++a) store4(o + a * ldo, v[a], nc, vec_out && nc == 4);
    }
}

// BODY: ROWS, and
//   __device__ __forceinline__ void operator()(long long lo, long long n, int c0, int nc, bool vec, float (*v)[4]) const
// fills channels c0 .. c0+nc-1 of the ROWS gradient rows of one reference row from its in-edges [lo, lo + n) of the lists.
// (__forceinline__: inlined late, the scalar backward body costs 6 VGPRs and a wave of occupancy.)
template <class BODY>
__global__ __launch_bounds__(THREADS) void cross_bwd_kernel(const int64_t* __restrict__ rptr, const int64_t* __restrict__ tptr,
                                                            long long num_edges, int C, float* __restrict__ dx, long long ldx,
                                                            int rpb, int vec_in, int vec_out, BODY body) {
    const int b = blockIdx.y;
    const long long rbase = rptr[b], nr = rptr[b + 1] - rbase;
    const long long r0 = (long long)blockIdx.x * rpb;
    if (r0 >= nr) return;                     // block-uniform (covers nr <= 0)
    const int rows = (int)(nr - r0 < rpb ? nr - r0 : rpb);
    const int groups = (C + 3) >> 2;
    for (int item = threadIdx.x; item < rows * groups; item += THREADS) {
        const int r = item / groups, g = item - r * groups;
        const long long row = rbase + r0 + r;
        const int c0 = 4 * g, nc = C - c0 < 4 ? C - c0 : 4;
        long long lo = tptr[row], hi = tptr[row + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > num_edges ? num_edges : hi;
        float v[BODY::ROWS][4];
        body(lo, hi > lo ? hi - lo : 0, c0, nc, vec_in && nc == 4, v);
        float* o = dx + (BODY::ROWS * row) * ldx + c0;
#pragma unroll
        for (int a = 0; a < BODY::ROWS; ++a) store4(o + a * ldx, v[a], nc, vec_out && nc == 4);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// What an apply entry point tells its launcher about itself: its name (the first word of every message), the names of the leading
// dimension of the rows it reads, of the rows it writes and of their leading dimension, the argument list of its null-pointer
// message with whether the pointers the launcher does not see are there, the table its body reads 16 bytes at a time (null: none)
// and the name of that argument in its entry point's message.
struct Call {
    const char *fn, *ld_in, *out, *ld_out, *nulls;
    bool others;
    const void* table;
    const char* table_name = "tmat";
};

inline int check_shape(const Call& c, int B, int k, int C, long long ld_in, long long ld_out) {
    DC_REQUIRE(B >= 0 && B <= 65535, "%s: B = %d cloud pairs, supported: 0 .. 65535 per launch", c.fn, B);
    DC_REQUIRE(k >= 1 && k <= dcinterp::MAX_K, "%s: k = %d outside [1, %d]", c.fn, k, dcinterp::MAX_K);
    DC_REQUIRE(C >= 1 && C <= (1 << 20), "%s: C = %d channels, supported: 1 .. 2^20", c.fn, C);
    DC_REQUIRE(ld_in >= C && ld_out >= C, "%s: leading dimensions %s = %lld, %s = %lld below C = %d", c.fn, c.ld_in, ld_in, c.ld_out,
               ld_out, C);
    return DC_OK;
}

inline int rows_vec(const void* p, long long ld) { return aligned_to(p, 16) && (ld & 3) == 0; }

// in [.., ld_in] -> out [ROWS * query rows, ld_out]
template <class BODY>
int launch_fwd(const Call& c, const float* in, long long ld_in, int C, const int64_t* qptr, const int64_t* rptr, int B,
               long long max_query_cloud, int k, float* out, long long ld_out, BODY body, void* stream) {
    if (int rc = check_shape(c, B, k, C, ld_in, ld_out)) return rc;
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= MAX_ITEMS, "%s: max_query_cloud = %lld outside [0, 2^39)", c.fn,
               max_query_cloud);
    if (B == 0 || max_query_cloud == 0) return DC_OK;
    DC_REQUIRE(in && qptr && rptr && c.others && out, "%s: null pointer (%s)", c.fn, c.nulls);
    DC_REQUIRE(aligned_to(c.table, 16), "%s: %s must be 16-byte aligned", c.fn, c.table_name);
    hipLaunchKernelGGL((cross_fwd_kernel<BODY>), dim3(dc_cdiv(max_query_cloud, THREADS), B), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), qptr, rptr, C, out, ld_out, rows_vec(in, ld_in), rows_vec(out, ld_out), body);
    DC_CHECK_LAUNCH(c.fn);
    return DC_OK;
}

// g [ROWS * num_g_rows, ld_in] -> dx [ROWS * reference rows, ld_out] over the lists tptr; c.others: the lists and weights the body
// reads are there.  `empty`: the call has nothing to read whatever the pointers say.  Without anything to read every list is cut
// to nothing and dx gets zeros.
template <class BODY>
int launch_bwd(const Call& c, const float* g, long long ld_in, long long num_g_rows, int C, const int64_t* rptr, int B,
               long long max_ref_cloud, int k, const int64_t* tptr, long long num_edges, bool empty, float* dx, long long ld_out,
               BODY body, void* stream) {
    if (int rc = check_shape(c, B, k, C, ld_in, ld_out)) return rc;
    DC_REQUIRE(max_ref_cloud >= 0 && max_ref_cloud <= MAX_REF, "%s: max_ref_cloud = %lld outside [0, 2^31)", c.fn, max_ref_cloud);
    DC_REQUIRE(num_g_rows >= 0 && num_edges >= 0, "%s: num_g_rows = %lld, num_edges = %lld below 0", c.fn, num_g_rows, num_edges);
    if (B == 0 || max_ref_cloud == 0) return DC_OK;
    DC_REQUIRE(rptr && tptr && dx, "%s: null pointer (rptr, tptr, %s)", c.fn, c.out);
    const bool readable = g && c.others;
    DC_REQUIRE(empty || num_edges == 0 || num_g_rows == 0 || readable, "%s: null pointer (%s)", c.fn, c.nulls);
    DC_REQUIRE(aligned_to(c.table, 16), "%s: %s must be 16-byte aligned", c.fn, c.table_name);
    if (!readable) num_edges = 0;
    const int groups = (C + 3) >> 2, rpb = groups >= THREADS ? 1 : THREADS / groups;
    hipLaunchKernelGGL((cross_bwd_kernel<BODY>), dim3(dc_cdiv(max_ref_cloud, rpb), B), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), rptr, tptr, num_edges, C, dx, ld_out, rpb, rows_vec(g, ld_in),
                       rows_vec(dx, ld_out), body);
    DC_CHECK_LAUNCH(c.fn);
    return DC_OK;
}

}  // namespace dccross
