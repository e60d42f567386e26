// g++ build of deltaconv_amd/csrc/cluster_math.h -- the rules of dc_cluster_lists / dc_cluster_pool / dc_cluster_pool_backward /
// dc_cluster_gather / dc_cluster_mean3 / dc_cluster_majority (cluster.hip) -- with the kernels' grids as plain serial loops on the
// CPU: one iteration per fill position, per (cell, group of 4 channels), per (point, group of 4 channels), per cell
// (tests/test_cluster_host.py).  The unordered fill runs over the rows BACKWARDS, so that the ranking has something to put right.
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/cluster_math.h"

namespace {
bool vec16(const void* p, long long ld) { return p && ((uintptr_t)p & 15) == 0 && (ld & 3) == 0; }
}  // namespace

extern "C" {

int32_t hcl_max_classes(void) { return dccl::MAX_CLASSES; }
int32_t hcl_mode(int32_t which) { return which == 0 ? dccl::MODE_MAX : which == 1 ? dccl::MODE_MIN : which == 2 ? dccl::MODE_SUM : dccl::MODE_MEAN; }

// cluster [n], m cells -> cptr [m+1], members [n] (entries from cptr[m] on: -1)
void hcl_lists(const int64_t* cluster, int64_t n, int64_t m, int64_t* cptr, int64_t* members) {
    std::vector<int64_t> cursor((size_t)m + 1, 0), unordered((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i)
        if (dccl::in_cell(cluster[i], m)) ++cursor[(size_t)cluster[i]];
    int64_t run = 0;
    for (int64_t j = 0; j < m; ++j) {
        cptr[j] = run;
        run += cursor[(size_t)j];
        cursor[(size_t)j] = cptr[j];
    }
    cptr[m] = run;
    for (int64_t i = n - 1; i >= 0; --i)
        if (dccl::in_cell(cluster[i], m)) unordered[(size_t)cursor[(size_t)cluster[i]]++] = i;
    for (int64_t t = 0; t < n; ++t) {
        if (t >= cptr[m]) {
            members[t] = -1;
            continue;
        }
        const int64_t e = unordered[(size_t)t], c = cluster[e];
        members[cptr[c] + dccl::rank_of(unordered.data(), cptr[c], cptr[c + 1], e)] = e;
    }
}

void hcl_pool(const float* x, int64_t ldx, int64_t n, int32_t C, const int64_t* cptr, const int64_t* members, int64_t m, int32_t mode,
              float* out, int64_t ldo, int32_t* arg, int64_t ldarg) {
    const bool vec = vec16(x, ldx);
    for (int64_t j = 0; j < m; ++j)
        for (int c0 = 0; c0 < C; c0 += 4) {
            const int nc = C - c0 < 4 ? C - c0 : 4;
            float v[4];
            int a[4];
            dccl::fwd4(x, ldx, n, members + cptr[j], cptr[j + 1] - cptr[j], mode, c0, nc, vec && nc == 4, v, a);
            for (int c = 0; c < nc; ++c) {
                out[j * ldo + c0 + c] = v[c];
                if (arg) arg[j * ldarg + c0 + c] = a[c];
            }
        }
}

// mode 2 with cptr = arg = null is the un-pooling (dc_cluster_gather)
void hcl_pool_backward(const float* g, int64_t ldg, int64_t m, int32_t C, const int64_t* cluster, int64_t n, const int64_t* cptr,
                       const int32_t* arg, int64_t ldarg, int32_t mode, float* dx, int64_t ldx) {
    const bool vec = vec16(g, ldg);
    for (int64_t i = 0; i < n; ++i)
        for (int c0 = 0; c0 < C; c0 += 4) {
            const int nc = C - c0 < 4 ? C - c0 : 4;
            float v[4];
            dccl::bwd4(g, ldg, m, cluster[i], i, cptr, arg, ldarg, mode, c0, nc, vec && nc == 4, v);
            for (int c = 0; c < nc; ++c) dx[i * ldx + c0 + c] = v[c];
        }
}

void hcl_mean3(const float* p, int64_t n, const int64_t* cptr, const int64_t* members, int64_t m, int32_t normalize, float* out) {
    for (int64_t j = 0; j < m; ++j) dccl::mean3(p, n, members + cptr[j], cptr[j + 1] - cptr[j], normalize, out + 3 * j);
}

void hcl_majority(const int64_t* labels, int64_t n, const int64_t* cptr, const int64_t* members, int64_t m, int32_t num_classes,
                  int64_t* out) {
    for (int64_t j = 0; j < m; ++j) out[j] = dccl::majority(labels, n, members + cptr[j], cptr[j + 1] - cptr[j], num_classes);
}

}  // extern "C"
