// Per-shape normalisation of a device-resident store of clouds or meshes: what the head of the reference's pre_transform does on
// the host one shape at a time (deltaconv/transforms/normalize_scale.py:12-21 in experiments/train_modelnet.py:30-34 and
// train_shapenet.py:30-33; normalize_area.py:12-20 and normalize_axes.py:17-26 in train_shapeseg.py:28-34).  A chain of 1 to 4
// ops per call, two launches:
//   shape_params_kernel  one workgroup of NORM_T threads per shape.  For every op of the chain in turn it loops over the shape's
//                        rows (or face rows), recomputing the earlier ops per element from the table built so far, and reduces what
//                        the op needs: bounding box and largest row norm (SCALE), bounding box and the fp64 sum of the face areas
//                        (AREA), the fp64 sums of x and x*x and the column maxima (AXES).  Strided per-thread partials, the xor
//                        butterfly of a wave, then the halving tree over the wave values in LDS: the fixed order of
//                        shape_norm_math.h.  One row of 8 floats per (shape, op) goes to the table.
//   shape_apply_kernel   chunks of 256 rows of the call through LDS: the flat [N,3] array is read and written coalesced, every
//                        output element is the chain applied to its row.  pos_out may alias pos (a chunk is read whole before
//                        any of it is written); normals are permuted as the positions are.
// Plain loops, no waiting across workgroups, no atomics; every per-shape value is written with a plain store.  The arithmetic is
// csrc/shape_norm_math.h (shared with tests/hostcheck_shapenorm).
#include "common.h"
#include "shape_norm_math.h"

namespace {

using dcnorm::Op;
constexpr int NORM_T = dcnorm::NORM_T;
constexpr int NORM_WAVES = dcnorm::NORM_WAVES;
constexpr int APPLY_T = 256;                  // rows of an apply chunk, one thread per row and three flat elements per thread

struct OpList {
    int n;
    int code[dcnorm::MAX_OPS];
    int ord_inf[dcnorm::MAX_OPS];             // SCALE: the row norm is max |.| instead of the 2-norm
    int has_ref[dcnorm::MAX_OPS];             // SCALE: ref is the constant below
    float ref[dcnorm::MAX_OPS];
};

struct SumF { __device__ double operator()(double a, double b) const { return a + b; } };
struct MaxF { __device__ double operator()(double a, double b) const { return dcnorm::omax(a, b); } };
struct MinF { __device__ double operator()(double a, double b) const { return dcnorm::omin(a, b); } };

// the same value in every thread; s_red [NORM_WAVES] is free again on return
template <class F>
__device__ __forceinline__ double block_reduce(double v, double* s_red, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = f(v, __shfl_xor(v, o, 64));
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    double w[NORM_WAVES];
#pragma unroll
    for (int k = 0; k < NORM_WAVES; ++k) w[k] = s_red[k];
#pragma unroll
    for (int o = NORM_WAVES / 2; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < o; ++i) w[i] = f(w[i], w[i + o]);
    __syncthreads();
    return w[0];
}

__device__ __forceinline__ void load_row(const float* __restrict__ p, long long i, float* r) {
    r[0] = p[3 * i]; r[1] = p[3 * i + 1]; r[2] = p[3 * i + 2];
}

__global__ __launch_bounds__(NORM_T) void shape_params_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr,
                                                              const int32_t* __restrict__ face, const int64_t* __restrict__ fptr,
                                                              OpList ops, float* __restrict__ table) {
    __shared__ double s_red[NORM_WAVES];
    __shared__ Op s_ops[dcnorm::MAX_OPS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long base = ptr[b], V = ptr[b + 1] - base;
    const float* p = pos + 3 * base;
    const double inf = __builtin_huge_val();
    for (int k = 0; k < ops.n; ++k) {
        const int code = ops.code[k];
        Op cur = dcnorm::identity_op();
        if (code == dcnorm::OP_AXES) {
            double sx[3] = {0.0, 0.0, 0.0}, sxx[3] = {0.0, 0.0, 0.0}, mx[3] = {-inf, -inf, -inf};
            for (long long i = tid; i < V; i += NORM_T) {
                float r[3];
                load_row(p, i, r);
                dcnorm::apply_chain(s_ops, k, r, r);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double x = (double)r[j];
                    sx[j] = sx[j] + x;
                    sxx[j] = sxx[j] + x * x;
                    mx[j] = dcnorm::omax(mx[j], x);
                }
            }
            double var[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                sx[j] = block_reduce(sx[j], s_red, SumF());
                sxx[j] = block_reduce(sxx[j], s_red, SumF());
                mx[j] = block_reduce(mx[j], s_red, MaxF());
                var[j] = dcnorm::axes_var(sx[j], sxx[j], V);
            }
            dcnorm::axes_perm(var, cur.perm);
            const double last = cur.perm[2] == 0 ? mx[0] : (cur.perm[2] == 1 ? mx[1] : mx[2]);
            cur.s = dcnorm::axes_scale((float)last);
        } else {                                                 // SCALE, AREA: the centre first
            double mx[3] = {-inf, -inf, -inf}, mn[3] = {inf, inf, inf};
            for (long long i = tid; i < V; i += NORM_T) {
                float r[3];
                load_row(p, i, r);
                dcnorm::apply_chain(s_ops, k, r, r);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    mx[j] = dcnorm::omax(mx[j], (double)r[j]);
                    mn[j] = dcnorm::omin(mn[j], (double)r[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                mx[j] = block_reduce(mx[j], s_red, MaxF());
                mn[j] = block_reduce(mn[j], s_red, MinF());
                cur.c[j] = dcnorm::centre_of((float)mx[j], (float)mn[j]);
            }
            if (code == dcnorm::OP_SCALE) {
                float ref = ops.ref[k];
                if (!ops.has_ref[k]) {
                    const bool oi = ops.ord_inf[k] != 0;
                    double d = 0.0;
                    for (long long i = tid; i < V; i += NORM_T) {
                        float r[3];
                        load_row(p, i, r);
                        dcnorm::apply_chain(s_ops, k, r, r);
#pragma unroll
                        for (int j = 0; j < 3; ++j) r[j] = r[j] - cur.c[j];
                        d = dcnorm::omax(d, oi ? dcnorm::row_norm_inf(r) : dcnorm::row_norm2(r));
                    }
                    ref = dcnorm::scale_ref(block_reduce(d, s_red, MaxF()), oi);
                }
                cur.s = dcnorm::scale_of_ref(ref);
            } else {                                             // AREA: the ordered sum over the face rows
                const long long fbase = fptr[b], F = fptr[b + 1] - fbase;
                const int32_t* fc = face + 3 * fbase;
                double acc = 0.0;
                for (long long f = tid; f < F; f += NORM_T) {
                    const long long id[3] = {fc[3 * f], fc[3 * f + 1], fc[3 * f + 2]};
                    double a = 0.0;
                    if (id[0] >= 0 && id[0] < V && id[1] >= 0 && id[1] < V && id[2] >= 0 && id[2] < V) {
                        float q[3][3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            load_row(p, id[c], q[c]);
                            dcnorm::apply_chain(s_ops, k, q[c], q[c]);
#pragma unroll
                            for (int j = 0; j < 3; ++j) q[c][j] = q[c][j] - cur.c[j];
                        }
                        a = dcnorm::face_area_rows(q[0], q[1], q[2]);
                    }
                    acc = acc + a;
                }
                cur.s = dcnorm::area_scale(block_reduce(acc, s_red, SumF()));
            }
        }
        if (tid == 0) {
            s_ops[k] = cur;
            dcnorm::write_stats(table + ((long long)b * ops.n + k) * dcnorm::STAT_WORDS, cur);
        }
        __syncthreads();                                         // the next op reads s_ops[k]
    }
}

// the last shape of [lo, hi] whose first row is at or before `row` (empty shapes in front of it are passed over)
__device__ __forceinline__ int shape_of(const int64_t* __restrict__ ptr, int lo, int hi, long long row) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (ptr[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(APPLY_T) void shape_apply_kernel(const float* pos, const int64_t* __restrict__ ptr, int B,
                                                              long long n_rows, const float* __restrict__ table, int n_ops,
                                                              float* pos_out, float* norm) {
    __shared__ float s_pos[3 * APPLY_T];
    __shared__ float s_nrm[3 * APPLY_T];
    const int tid = threadIdx.x;
    const long long first = ptr[0], end = ptr[B];
    const long long row0 = first + (long long)blockIdx.x * APPLY_T;
    long long left = n_rows - (long long)blockIdx.x * APPLY_T;
    if (end - row0 < left) left = end - row0;                   // nothing past the last shape of the call is touched
    if (left <= 0) return;                                       // the whole workgroup
    const int rows = left < APPLY_T ? (int)left : APPLY_T, count = 3 * rows;
    const long long e0 = 3 * row0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = tid + APPLY_T * k;
        if (e < count) {
            s_pos[e] = pos[e0 + e];
            if (norm) s_nrm[e] = norm[e0 + e];
        }
    }
    __syncthreads();
    const int b_lo = shape_of(ptr, 0, B - 1, row0), b_hi = shape_of(ptr, b_lo, B - 1, row0 + rows - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = tid + APPLY_T * k;
        if (e >= count) continue;
        const int r = e / 3, j = e - 3 * r;
        const int b = b_lo == b_hi ? b_lo : shape_of(ptr, b_lo, b_hi, row0 + r);
        const float* t = table + (long long)b * n_ops * dcnorm::STAT_WORDS;
        float v[3] = {s_pos[3 * r], s_pos[3 * r + 1], s_pos[3 * r + 2]};
        float n[3] = {0.f, 0.f, 0.f};
        if (norm) { n[0] = s_nrm[3 * r]; n[1] = s_nrm[3 * r + 1]; n[2] = s_nrm[3 * r + 2]; }
        for (int i = 0; i < n_ops; ++i) {
            const Op op = dcnorm::read_stats(t + i * dcnorm::STAT_WORDS);
            dcnorm::apply_op(op, v, v);
            const float m[3] = {dcnorm::pick3(n, op.perm[0]), dcnorm::pick3(n, op.perm[1]), dcnorm::pick3(n, op.perm[2])};
            n[0] = m[0]; n[1] = m[1]; n[2] = m[2];
        }
        pos_out[e0 + e] = dcnorm::pick3(v, j);
        if (norm) norm[e0 + e] = dcnorm::pick3(n, j);
    }
}

}  // namespace

DC_EXPORT int32_t dc_shape_normalize_threads(void) { return NORM_T; }

DC_EXPORT int dc_shape_normalize(const float* pos, const int64_t* ptr, const int32_t* face, const int64_t* fptr, int32_t B,
                                 int64_t n_rows, const int32_t* op_codes, const float* op_params, int32_t n_ops, float* pos_out,
                                 float* norm, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    DC_REQUIRE(n_ops >= 1 && n_ops <= dcnorm::MAX_OPS, "dc_shape_normalize: n_ops = %d, supported: 1 .. %d", n_ops, dcnorm::MAX_OPS);
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_shape_normalize: B = %d shapes, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(n_rows >= 0 && n_rows < (1ll << 39), "dc_shape_normalize: n_rows = %lld outside [0, 2^39)", (long long)n_rows);
    DC_REQUIRE(op_codes && op_params, "dc_shape_normalize: null pointer (op_codes, op_params)");
    OpList ops{};
    ops.n = n_ops;
    bool permutes = false;
    for (int k = 0; k < n_ops; ++k) {
        const int code = op_codes[k];
        const float ord = op_params[2 * k], ref = op_params[2 * k + 1];
        DC_REQUIRE(code == dcnorm::OP_SCALE || code == dcnorm::OP_AREA || code == dcnorm::OP_AXES,
                   "dc_shape_normalize: op %d has the unknown code %d (1 scale, 2 area, 3 axes)", k, code);
        ops.code[k] = code;
        if (code == dcnorm::OP_SCALE) {
            const bool oi = ord > 3.0e38f;                       // +inf
            DC_REQUIRE(oi || ord == 2.0f, "dc_shape_normalize: op %d: norm_ord = %g, supported: 2 and inf", k, (double)ord);
            ops.ord_inf[k] = oi;
            ops.has_ref[k] = ref == ref;                         // NaN: no scaling_factor
            ops.ref[k] = ref;
        }
        DC_REQUIRE(code != dcnorm::OP_AREA || (face && fptr), "dc_shape_normalize: op %d is an area op and needs face and fptr", k);
        permutes = permutes || code == dcnorm::OP_AXES;
    }
    if (B == 0) return DC_OK;
    DC_REQUIRE(pos && ptr && pos_out, "dc_shape_normalize: null pointer (pos, ptr, pos_out)");
    float* table = stats;
    if (!table) {
        const size_t need = (size_t)B * n_ops * dcnorm::STAT_WORDS * sizeof(float);
        if (!workspace || workspace_bytes < need) {
            dc_set_error("dc_shape_normalize: without stats the parameter table needs a workspace of %zu bytes (32 per shape and "
                         "op), got %zu", need, workspace ? workspace_bytes : (size_t)0);
            return DC_ERR_WORKSPACE;
        }
        DC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "dc_shape_normalize: workspace must be 4-byte aligned");
        table = static_cast<float*>(workspace);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(shape_params_kernel, dim3(B), dim3(NORM_T), 0, s, pos, ptr, face, fptr, ops, table);
    DC_CHECK_LAUNCH("dc_shape_normalize (parameters)");
    if (n_rows == 0) return DC_OK;
    hipLaunchKernelGGL(shape_apply_kernel, dim3(dc_cdiv(n_rows, APPLY_T)), dim3(APPLY_T), 0, s, pos, ptr, (int)B, (long long)n_rows,
                       table, (int)n_ops, pos_out, permutes ? norm : nullptr);
    DC_CHECK_LAUNCH("dc_shape_normalize (apply)");
    return DC_OK;
}
