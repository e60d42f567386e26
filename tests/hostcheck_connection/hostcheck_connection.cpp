// g++ build of deltaconv_amd/csrc/connection_math.h -- the per-thread code of dc_build_transport, dc_angle_in_plane,
// dc_rotate_around, dc_transport_sum and dc_transport_sum_backward (connection.hip), looped over edges / points / channel groups on
// the CPU (tests/test_connection_host.py).  Built without contraction, as the library is.
#include <stdint.h>

#include "../../deltaconv_amd/csrc/connection_math.h"

using namespace dcconn;

extern "C" {

// nbr == nullptr: the pair form; else target row m / k, source row nbr[m]
void hc_build_transport(const float* tn, const float* tx, const float* ty, const float* sn, const float* sx, const int32_t* nbr,
                        int32_t k, int64_t M, int32_t non_oriented, float* out) {
    for (int64_t m = 0; m < M; ++m) {
        const int64_t t = nbr ? m / k : m, s = nbr ? (int64_t)nbr[m] : m;
        const R4 r = transport(ld3(tn + 3 * t), ld3(tx + 3 * t), ld3(ty + 3 * t), ld3(sn + 3 * s), ld3(sx + 3 * s), non_oriented);
        out[4 * m] = r.r00;
        out[4 * m + 1] = r.r01;
        out[4 * m + 2] = r.r10;
        out[4 * m + 3] = r.r11;
    }
}

void hc_angle_in_plane(const float* u, const float* v, const float* normal, int64_t M, float* out) {
    for (int64_t m = 0; m < M; ++m) out[m] = angle_in_plane(ld3(u + 3 * m), ld3(v + 3 * m), ld3(normal + 3 * m));
}

void hc_rotate_around(const float* v, const float* axis, const float* angle, int64_t M, float* out) {
    for (int64_t m = 0; m < M; ++m) {
        const F3 r = rotate_around(ld3(v + 3 * m), ld3(axis + 3 * m), angle[m]);
        out[3 * m] = r.x;
        out[3 * m + 1] = r.y;
        out[3 * m + 2] = r.z;
    }
}

// channels in groups of 4 (vec: rows 16-byte aligned, C a multiple of 4) or one by one, as the kernel's threads take them
void hc_transport_sum(const int32_t* nbr, int32_t n, int32_t k, const float* coef, const float* v, int32_t C, int64_t ldv,
                      float scale, int32_t vec, float* out, int64_t ldo) {
    const R4* cf = reinterpret_cast<const R4*>(coef);
    for (long i = 0; i < n; ++i) {
        if (vec)
            for (int c0 = 0; c0 < C; c0 += 4) transport_sum_fwd<4>(i, c0, nbr + i * k, cf + i * k, k, v, ldv, scale, out, ldo);
        else
            for (int c0 = 0; c0 < C; ++c0) transport_sum_fwd<1>(i, c0, nbr + i * k, cf + i * k, k, v, ldv, scale, out, ldo);
    }
}

void hc_transport_sum_backward(const int32_t* tptr, const int32_t* tedge, int32_t n, int32_t k, const float* coef, const float* g,
                               int32_t C, int64_t ldg, float scale, int32_t vec, float* dv, int64_t ldv, int32_t accumulate) {
    const R4* cf = reinterpret_cast<const R4*>(coef);
    for (long j = 0; j < n; ++j) {
        if (vec)
            for (int c0 = 0; c0 < C; c0 += 4)
                dcell::walk_column(TransportSumT<4>{cf, k, g, ldg, scale, dv, ldv, accumulate, C}, j, c0, nullptr, tptr, tedge, k);
        else
            for (int c0 = 0; c0 < C; ++c0)
                dcell::walk_column(TransportSumT<1>{cf, k, g, ldg, scale, dv, ldv, accumulate, C}, j, c0, nullptr, tptr, tedge, k);
    }
}

}  // extern "C"
