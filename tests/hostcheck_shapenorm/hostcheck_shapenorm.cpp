// g++ build of deltaconv_amd/csrc/shape_norm_math.h -- the parameter pass and the apply pass of the per-shape normalisation
// (shape_norm.hip) for ONE shape, serially on the CPU: the workgroup's strided partials are an array of NORM_T doubles, its
// reduction is dcnorm::tree_sum (tests/test_shape_norm_host.py).
#include <stdint.h>

#include <vector>

#include "../../deltaconv_amd/csrc/shape_norm_math.h"

namespace {

using dcnorm::Op;

struct Partials {
    std::vector<double> v;
    Partials() : v(dcnorm::NORM_T, 0.0) {}
    void add(long long i, double x) { v[i % dcnorm::NORM_T] = v[i % dcnorm::NORM_T] + x; }
    double sum() { return dcnorm::tree_sum(v.data()); }
};

void row_after(const float* pos, long long i, const Op* ops, int k, float* r) { dcnorm::apply_chain(ops, k, pos + 3 * i, r); }

}  // namespace

extern "C" {

int32_t hn_threads(void) { return dcnorm::NORM_T; }

// pos [V,3], face [F,3] or null, op_codes [n_ops], op_params [n_ops,2] -> pos_out [V,3] (may alias pos), norm [V,3] in place or
// null, stats [n_ops,8].  -> 0, or -1 for what dc_shape_normalize refuses.
int hn_normalize(const float* pos, int64_t V, const int32_t* face, int64_t F, const int32_t* op_codes, const float* op_params,
                 int32_t n_ops, float* pos_out, float* norm, float* stats) {
    if (n_ops < 1 || n_ops > dcnorm::MAX_OPS) return -1;
    Op ops[dcnorm::MAX_OPS];
    const double inf = __builtin_huge_val();
    for (int k = 0; k < n_ops; ++k) {
        const int code = op_codes[k];
        const float ord = op_params[2 * k], factor = op_params[2 * k + 1];
        Op cur = dcnorm::identity_op();
        if (code == dcnorm::OP_AXES) {
            Partials sx[3], sxx[3];
            double mx[3] = {-inf, -inf, -inf}, var[3];
            for (int64_t i = 0; i < V; ++i) {
                float r[3];
                row_after(pos, i, ops, k, r);
                for (int j = 0; j < 3; ++j) {
                    const double x = (double)r[j];
                    sx[j].add(i, x);
                    sxx[j].add(i, x * x);
                    mx[j] = dcnorm::omax(mx[j], x);
                }
            }
            for (int j = 0; j < 3; ++j) var[j] = dcnorm::axes_var(sx[j].sum(), sxx[j].sum(), V);
            dcnorm::axes_perm(var, cur.perm);
            cur.s = dcnorm::axes_scale((float)mx[cur.perm[2]]);
        } else if (code == dcnorm::OP_SCALE || code == dcnorm::OP_AREA) {
            double mx[3] = {-inf, -inf, -inf}, mn[3] = {inf, inf, inf};
            for (int64_t i = 0; i < V; ++i) {
                float r[3];
                row_after(pos, i, ops, k, r);
                for (int j = 0; j < 3; ++j) {
                    mx[j] = dcnorm::omax(mx[j], (double)r[j]);
                    mn[j] = dcnorm::omin(mn[j], (double)r[j]);
                }
            }
            for (int j = 0; j < 3; ++j) cur.c[j] = dcnorm::centre_of((float)mx[j], (float)mn[j]);
            if (code == dcnorm::OP_SCALE) {
                const bool oi = ord > 3.0e38f;
                if (!oi && ord != 2.0f) return -1;
                float ref = factor;
                if (factor != factor) {
                    double d = 0.0;
                    for (int64_t i = 0; i < V; ++i) {
                        float r[3];
                        row_after(pos, i, ops, k, r);
                        for (int j = 0; j < 3; ++j) r[j] = r[j] - cur.c[j];
                        d = dcnorm::omax(d, oi ? dcnorm::row_norm_inf(r) : dcnorm::row_norm2(r));
                    }
                    ref = dcnorm::scale_ref(d, oi);
                }
                cur.s = dcnorm::scale_of_ref(ref);
            } else {
                if (!face) return -1;
                Partials acc;
                for (int64_t f = 0; f < F; ++f) {
                    const long long id[3] = {face[3 * f], face[3 * f + 1], face[3 * f + 2]};
                    double a = 0.0;
                    if (id[0] >= 0 && id[0] < V && id[1] >= 0 && id[1] < V && id[2] >= 0 && id[2] < V) {
                        float q[3][3];
                        for (int c = 0; c < 3; ++c) {
                            row_after(pos, id[c], ops, k, q[c]);
                            for (int j = 0; j < 3; ++j) q[c][j] = q[c][j] - cur.c[j];
                        }
                        a = dcnorm::face_area_rows(q[0], q[1], q[2]);
                    }
                    acc.add(f, a);
                }
                cur.s = dcnorm::area_scale(acc.sum());
            }
        } else {
            return -1;
        }
        ops[k] = cur;
        dcnorm::write_stats(stats + dcnorm::STAT_WORDS * k, cur);
    }
    for (int64_t i = 0; i < V; ++i) {
        float v[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, n[3] = {0.f, 0.f, 0.f};
        if (norm) for (int j = 0; j < 3; ++j) n[j] = norm[3 * i + j];
        for (int k = 0; k < n_ops; ++k) {
            const Op op = dcnorm::read_stats(stats + dcnorm::STAT_WORDS * k);
            dcnorm::apply_op(op, v, v);
            const float m[3] = {dcnorm::pick3(n, op.perm[0]), dcnorm::pick3(n, op.perm[1]), dcnorm::pick3(n, op.perm[2])};
            n[0] = m[0]; n[1] = m[1]; n[2] = m[2];
        }
        for (int j = 0; j < 3; ++j) {
            pos_out[3 * i + j] = v[j];
            if (norm) norm[3 * i + j] = n[j];
        }
    }
    return 0;
}

}  // extern "C"
