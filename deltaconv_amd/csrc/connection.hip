// Parallel transport between tangent frames (reference: deltaconv/geometry/connection.py): the per-edge connection as one
// elementwise launch, its two helpers, and the sum of transported neighbour vectors with its transpose.  The arithmetic is
// connection_math.h, shared with the g++ build of tests/hostcheck_connection.
// All of it streams: build_transport reads 60 B and writes 16 B per pair (graph form: the k edges of a point share the
// target's rows); the sums move 16 E + 4 E + 8 C N bytes in and 8 C N out and gather rows exactly as dc_apply_div does.
#include <initializer_list>
#include "common.h"
#include "ell_stage.h"
#include "connection_math.h"

namespace {
using namespace dcconn;
using namespace dcstage;

// one thread per edge m.  nbr == nullptr: the pair form, row m of all five arrays; else target row m / k, source row nbr[m]
__global__ __launch_bounds__(256) void build_transport_kernel(const float* __restrict__ tn, const float* __restrict__ tx,
                                                              const float* __restrict__ ty, const float* sn, const float* sx,
                                                              const int* __restrict__ nbr, int k, long M, int non_oriented,
                                                              int vec, float* __restrict__ out) {
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const long t = nbr ? m / k : m;
    const long s = nbr ? (long)nbr[m] : m;
    const R4 r = transport(ld3(tn + 3 * t), ld3(tx + 3 * t), ld3(ty + 3 * t), ld3(sn + 3 * s), ld3(sx + 3 * s), non_oriented);
    if (vec) {
        *reinterpret_cast<R4*>(out + 4 * m) = r;
    } else {
        out[4 * m] = r.r00;
        out[4 * m + 1] = r.r01;
        out[4 * m + 2] = r.r10;
        out[4 * m + 3] = r.r11;
    }
}

__global__ __launch_bounds__(256) void angle_in_plane_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                             const float* __restrict__ normal, long M, float* __restrict__ out) {
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    out[m] = angle_in_plane(ld3(u + 3 * m), ld3(v + 3 * m), ld3(normal + 3 * m));
}

__global__ __launch_bounds__(256) void rotate_around_kernel(const float* __restrict__ v, const float* __restrict__ axis,
                                                            const float* __restrict__ angle, long M, float* __restrict__ out) {
    const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const F3 r = rotate_around(ld3(v + 3 * m), ld3(axis + 3 * m), angle[m]);
    out[3 * m] = r.x;
    out[3 * m + 1] = r.y;
    out[3 * m + 2] = r.z;
}

// forward body of the staged skeleton (ell_stage.h): the ids come from LDS; the connection of a slot is one 16-byte load, the
// same address on every channel lane of a point
template <int V>
struct TransportSumF {
    const R4* coef; const float* v; long ldv; float scale; float* out; long ldo;
    __device__ void operator()(long i, int c0, Row r, int k) const {
        transport_sum_fwd<V>(i, c0, r.ids, coef + i * k, k, v, ldv, scale, out, ldo);
    }
};
}  // namespace

DC_EXPORT int dc_build_transport(const float* tn, const float* tx, const float* ty, const float* sn, const float* sx,
                                 const int32_t* nbr, int32_t k, int64_t M, int32_t non_oriented, float* out, void* stream) {
    DC_REQUIRE(M >= 0, "dc_build_transport: M = %lld", (long long)M);
    DC_REQUIRE(!nbr || (k >= 1 && k <= 255), "dc_build_transport: k = %d outside 1 .. 255", k);
    if (M == 0) return DC_OK;
    DC_REQUIRE(tn && tx && ty && sn && sx && out, "dc_build_transport: null pointer");
    hipLaunchKernelGGL(build_transport_kernel, dim3(dc_cdiv(M, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), tn, tx, ty,
                       sn, sx, nbr, nbr ? k : 1, (long)M, non_oriented, aligned_to(out, 16) ? 1 : 0, out);
    DC_CHECK_LAUNCH("dc_build_transport");
    return DC_OK;
}

DC_EXPORT int dc_angle_in_plane(const float* u, const float* v, const float* normal, int64_t M, float* out, void* stream) {
    DC_REQUIRE(M >= 0, "dc_angle_in_plane: M = %lld", (long long)M);
    if (M == 0) return DC_OK;
    DC_REQUIRE(u && v && normal && out, "dc_angle_in_plane: null pointer");
    hipLaunchKernelGGL(angle_in_plane_kernel, dim3(dc_cdiv(M, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), u, v, normal,
                       (long)M, out);
    DC_CHECK_LAUNCH("dc_angle_in_plane");
    return DC_OK;
}

DC_EXPORT int dc_rotate_around(const float* v, const float* axis, const float* angle, int64_t M, float* out, void* stream) {
    DC_REQUIRE(M >= 0, "dc_rotate_around: M = %lld", (long long)M);
    if (M == 0) return DC_OK;
    DC_REQUIRE(v && axis && angle && out, "dc_rotate_around: null pointer");
    hipLaunchKernelGGL(rotate_around_kernel, dim3(dc_cdiv(M, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), v, axis, angle,
                       (long)M, out);
    DC_CHECK_LAUNCH("dc_rotate_around");
    return DC_OK;
}

DC_EXPORT int dc_transport_sum(const int32_t* nbr, int32_t n, int32_t k, const float* coef, const float* v, int32_t C,
                               int64_t ldv, float scale, float* out, int64_t ldo, void* stream) {
    DC_REQUIRE(n >= 0 && k >= 1 && k <= 255 && C >= 0, "dc_transport_sum: bad size (1 <= k <= 255)");
    if (n == 0 || C == 0) return DC_OK;
    DC_REQUIRE(nbr && coef && v && out, "dc_transport_sum: null pointer");
    DC_REQUIRE(aligned_to(coef, 16), "dc_transport_sum: coef must be 16-byte aligned");
    DC_REQUIRE(ldv >= C && ldo >= C, "dc_transport_sum: leading dimension smaller than the row");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const R4* cf = reinterpret_cast<const R4*>(coef);
    if (pick_v(C, {(long)ldv, (long)ldo}, {v, out}) == 4)
        launch_fwd<4>(n, C, nullptr, nbr, k, TransportSumF<4>{cf, v, (long)ldv, scale, out, (long)ldo}, s);
    else
        launch_fwd<1>(n, C, nullptr, nbr, k, TransportSumF<1>{cf, v, (long)ldv, scale, out, (long)ldo}, s);
    DC_CHECK_LAUNCH("dc_transport_sum");
    return DC_OK;
}

DC_EXPORT int dc_transport_sum_backward(const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const float* coef,
                                        const float* g, int32_t C, int64_t ldg, float scale, float* dv, int64_t ldv,
                                        int32_t accumulate, void* stream) {
    DC_REQUIRE(n >= 0 && k >= 1 && k <= 255 && C >= 0, "dc_transport_sum_backward: bad size (1 <= k <= 255)");
    if (n == 0 || C == 0) return DC_OK;
    DC_REQUIRE(tptr && tedge && coef && g && dv, "dc_transport_sum_backward: null pointer");
    DC_REQUIRE(aligned_to(coef, 16), "dc_transport_sum_backward: coef must be 16-byte aligned");
    DC_REQUIRE(ldg >= C && ldv >= C, "dc_transport_sum_backward: leading dimension smaller than the row");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const R4* cf = reinterpret_cast<const R4*>(coef);
    if (pick_v(C, {(long)ldg, (long)ldv}, {g, dv}) == 4)
        launch_T<4>(n, C, nullptr, tptr, tedge, k, TransportSumT<4>{cf, k, g, (long)ldg, scale, dv, (long)ldv, accumulate, C}, s);
    else
        launch_T<1>(n, C, nullptr, tptr, tedge, k, TransportSumT<1>{cf, k, g, (long)ldg, scale, dv, (long)ldv, accumulate, C}, s);
    DC_CHECK_LAUNCH("dc_transport_sum_backward");
    return DC_OK;
}
