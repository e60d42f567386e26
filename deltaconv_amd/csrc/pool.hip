// Pooling of scalar features from a cloud down to a sampled one, batched over cloud pairs -- stands in for a torch_cluster.knn
// search followed by torch_scatter.scatter(x[col], row, reduce = "max" | "min" | "sum" | "mean"): the set-abstraction step of
// PointNet++, the scalar stream's way DOWN between resolutions (dc_knn_interpolate is its way up).  Every sampled point reduces
// the rows of its k nearest points of the full cloud; the search is dc_knn_cross with the sampled cloud as the query.  The
// reference has no such call site.  The arithmetic is csrc/pool_math.h (shared with tests/hostcheck_pool).
//
// Mapping: the frame of cross_stage.h, nothing else -- the grid conventions of interp.hip: (chunks up to the largest cloud) x
// (cloud pairs), at most 65 535 pairs a launch; a workgroup past its cloud's end returns, block-uniformly.
//   cross_fwd_kernel<PoolF>   thread = (query, group of 4 channels): the k reference rows are read 16 bytes at a time where x, ldx
//                             and C allow, scalar otherwise (any C >= 1).  Beside the frame's store of the pooled row the body
//                             writes the group's four slot numbers (max / min: one 32-bit store where arg and ldarg allow, byte
//                             stores otherwise) and, from the thread of channel group 0, the query's count of valid slots
//   cross_bwd_kernel<PoolT>   thread = (reference row, group of 4 channels): it walks the row's in-edges (the lists of
//                             dc_knn_cross_transpose) in order, four edges in flight; per edge one row of g, and the four slot
//                             numbers (max / min) or the count (mean) of the edge's query
// Plain vector loads and stores, no atomics, no LDS: the outputs are a function of the inputs only.
#include "common.h"
#include "cross_stage.h"
#include "pool_math.h"

namespace {

// The reduction over a query's k reference rows, with its side outputs (cross_stage.h: cross_fwd_kernel).
struct PoolF {
    static constexpr int ROWS = 1;
    const float* __restrict__ x;
    long long ldx;
    int k, mode;
    const int32_t* __restrict__ idx;
    unsigned char* __restrict__ arg;          // null: sum / mean without one
    long long ldarg;
    unsigned char* __restrict__ cnt;
    int word;                                 // arg + 4 g is 4-byte aligned in every row
    __device__ __forceinline__ void operator()(const dccross::Span& p, long long row, int c0, int nc, bool vec, float (*v)[4]) const {
        unsigned char a[4];
        const int n = dcpool::fwd4(x + p.rbase * ldx, ldx, p.nr, k, idx + row * k, mode, c0, nc, vec, v[0], a);
        if (arg && mode <= dcpool::MODE_MIN) dcpool::store_arg4(arg + row * ldarg + c0, a, nc, word && nc == 4);
        if (c0 == 0) cnt[row] = (unsigned char)n;
    }
};

// The ordered sum over a reference row's in-edges (cross_stage.h: cross_bwd_kernel); MODE_MAX serves max and min.
template <int MODE>
struct PoolT {
    static constexpr int ROWS = 1;
    const float* __restrict__ g;
    long long ldg, g_rows;
    int k;
    const int64_t* __restrict__ tedge;
    const unsigned char* __restrict__ arg;
    long long ldarg;
    const unsigned char* __restrict__ cnt;
    int word;
    __device__ __forceinline__ void operator()(long long lo, long long n, int c0, int nc, bool vec, float (*v)[4]) const {
        dcpool::bwd4<MODE>(g, ldg, g_rows, k, tedge + lo, n, arg, ldarg, cnt, c0, nc, vec, word && nc == 4, v[0]);
    }
};

inline int arg_words(const void* arg, long long ldarg) { return arg && aligned_to(arg, 4) && (ldarg & 3) == 0; }

}  // namespace

DC_EXPORT int dc_knn_pool(const float* x, int64_t ldx, int32_t C, const int64_t* qptr, const int64_t* rptr, int32_t B,
                          int64_t max_query_cloud, int32_t k, const int32_t* idx, int32_t mode, float* out, int64_t ldo,
                          uint8_t* arg, int64_t ldarg, uint8_t* cnt, void* stream) {
    DC_REQUIRE(mode >= 0 && mode <= 3, "dc_knn_pool: mode = %d outside 0 .. 3 (max, min, sum, mean)", mode);
    DC_REQUIRE(!arg || ldarg >= C, "dc_knn_pool: leading dimension ldarg = %lld below C = %d", (long long)ldarg, C);
    DC_REQUIRE(cnt && (arg || mode >= dcpool::MODE_SUM), "dc_knn_pool: null pointer (cnt; arg unless mode is sum or mean)");
    const dccross::Call c{"dc_knn_pool", "ldx", "out", "ldo", "x, qptr, rptr, idx, out", idx != nullptr, nullptr};
    return dccross::launch_fwd(c, x, ldx, C, qptr, rptr, B, max_query_cloud, k, out, ldo,
                               PoolF{x, ldx, k, mode, idx, arg, ldarg, cnt, arg_words(arg, ldarg)}, stream);
}

DC_EXPORT int dc_knn_pool_backward(const float* g, int64_t ldg, int64_t num_g_rows, int32_t C, const int64_t* rptr, int32_t B,
                                   int64_t max_ref_cloud, int32_t k, const int64_t* tptr, const int64_t* tedge, int64_t num_edges,
                                   int32_t mode, const uint8_t* arg, int64_t ldarg, const uint8_t* cnt, float* dx, int64_t ldx,
                                   void* stream) {
    DC_REQUIRE(mode >= 0 && mode <= 3, "dc_knn_pool_backward: mode = %d outside 0 .. 3 (max, min, sum, mean)", mode);
    DC_REQUIRE(!arg || ldarg >= C, "dc_knn_pool_backward: leading dimension ldarg = %lld below C = %d", (long long)ldarg, C);
    DC_REQUIRE(cnt && (arg || mode >= dcpool::MODE_SUM), "dc_knn_pool_backward: null pointer (cnt; arg unless mode is sum or mean)");
    const dccross::Call c{"dc_knn_pool_backward", "ldg", "dx", "ldx", "g, tedge", tedge != nullptr, nullptr};
    const auto run = [&](auto body) {
        return dccross::launch_bwd(c, g, ldg, num_g_rows, C, rptr, B, max_ref_cloud, k, tptr, num_edges, false, dx, ldx, body, stream);
    };
    const int word = arg_words(arg, ldarg);
    if (mode <= dcpool::MODE_MIN) return run(PoolT<dcpool::MODE_MAX>{g, ldg, num_g_rows, k, tedge, arg, ldarg, cnt, word});
    if (mode == dcpool::MODE_SUM) return run(PoolT<dcpool::MODE_SUM>{g, ldg, num_g_rows, k, tedge, arg, ldarg, cnt, word});
    return run(PoolT<dcpool::MODE_MEAN>{g, ldg, num_g_rows, k, tedge, arg, ldarg, cnt, word});
}
