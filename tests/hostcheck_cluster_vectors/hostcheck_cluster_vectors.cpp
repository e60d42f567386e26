// g++ build of deltaconv_amd/csrc/cluster_vectors_math.h -- the rules of dc_cluster_rotation / dc_cluster_pool_vectors /
// dc_cluster_pool_vectors_backward / dc_cluster_unpool_vectors / dc_cluster_unpool_vectors_backward (cluster_vectors.hip) -- with
// the kernels' grids as plain serial loops on the CPU: one iteration per point, per (cell, group of 4 channels), per (point, group
// of 4 channels) (tests/test_cluster_vectors_host.py).
#include <stdint.h>

#include "../../deltaconv_amd/csrc/cluster_vectors_math.h"

namespace {
bool vec16(const void* p, long long ld) { return p && ((uintptr_t)p & 15) == 0 && (ld & 3) == 0; }

template <bool TRANSPOSED>
void walk(const float* v, int64_t ldv, int64_t n, int32_t C, const int64_t* cptr, const int64_t* members, int64_t m, const float* rmat,
          int32_t mode, float* out, int64_t ldo, int32_t* arg, int64_t ldarg) {
    const bool vec = vec16(v, ldv);
    for (int64_t j = 0; j < m; ++j)
        for (int c0 = 0; c0 < C; c0 += 4) {
            const int nc = C - c0 < 4 ? C - c0 : 4;
            float a[4], b[4];
            int at[4];
            dcclv::walk4<TRANSPOSED>(v, ldv, n, members + cptr[j], cptr[j + 1] - cptr[j], reinterpret_cast<const dcconn::R4*>(rmat), mode,
                                     c0, nc, vec && nc == 4, a, b, at);
            for (int c = 0; c < nc; ++c) {
                out[(2 * j) * ldo + c0 + c] = a[c];
                out[(2 * j + 1) * ldo + c0 + c] = b[c];
                if (arg) arg[j * ldarg + c0 + c] = at[c];
            }
        }
}

template <bool TRANSPOSED>
void gather(const float* g, int64_t ldg, int64_t m, int32_t C, const int64_t* cluster, int64_t n, const int64_t* cptr, const float* rmat,
            const int32_t* arg, int64_t ldarg, int32_t mode, float* out, int64_t ldo) {
    const bool vec = vec16(g, ldg);
    for (int64_t i = 0; i < n; ++i)
        for (int c0 = 0; c0 < C; c0 += 4) {
            const int nc = C - c0 < 4 ? C - c0 : 4;
            float a[4], b[4];
            dcclv::gather4<TRANSPOSED>(g, ldg, m, cluster[i], i, reinterpret_cast<const dcconn::R4*>(rmat)[i], cptr, arg, ldarg, mode, c0,
                                       nc, vec && nc == 4, a, b);
            for (int c = 0; c < nc; ++c) {
                out[(2 * i) * ldo + c0 + c] = a[c];
                out[(2 * i + 1) * ldo + c0 + c] = b[c];
            }
        }
}
}  // namespace

extern "C" {

int32_t hcv_mode_ok(int32_t mode) { return dcclv::mode_ok(mode) ? 1 : 0; }

// rmat [n,4], 16-byte aligned
void hcv_rotation(const int64_t* cluster, int64_t n, int64_t m, const float* fn, const float* fx, const float* fy, const float* cn,
                  const float* cx, const float* cy, int32_t to_cell, int32_t non_oriented, float* rmat) {
    for (int64_t i = 0; i < n; ++i)
        reinterpret_cast<dcconn::R4*>(rmat)[i] = dcclv::rotation(i, cluster[i], m, fn, fx, fy, cn, cx, cy, to_cell, non_oriented);
}

void hcv_pool(const float* v, int64_t ldv, int64_t n, int32_t C, const int64_t* cptr, const int64_t* members, int64_t m,
              const float* rmat, int32_t mode, float* out, int64_t ldo, int32_t* arg, int64_t ldarg) {
    walk<false>(v, ldv, n, C, cptr, members, m, rmat, mode, out, ldo, arg, ldarg);
}

void hcv_pool_backward(const float* g, int64_t ldg, int64_t m, int32_t C, const int64_t* cluster, int64_t n, const int64_t* cptr,
                       const float* rmat, const int32_t* arg, int64_t ldarg, int32_t mode, float* dv, int64_t ldv) {
    gather<true>(g, ldg, m, C, cluster, n, cptr, rmat, arg, ldarg, mode, dv, ldv);
}

void hcv_unpool(const float* x, int64_t ldx, int64_t m, int32_t C, const int64_t* cluster, int64_t n, const float* rmat, float* out,
                int64_t ldo) {
    gather<false>(x, ldx, m, C, cluster, n, nullptr, rmat, nullptr, 0, dcclv::MODE_SUM, out, ldo);
}

void hcv_unpool_backward(const float* g, int64_t ldg, int64_t n, int32_t C, const int64_t* cptr, const int64_t* members, int64_t m,
                         const float* rmat, float* dx, int64_t ldx) {
    walk<true>(g, ldg, n, C, cptr, members, m, rmat, dcclv::MODE_SUM, dx, ldx, nullptr, 0);
}

}  // extern "C"
