// Batch assembly from a device-resident dataset, augmentation included, in ONE launch: what the reference's loops do on the host
// per shape and per batch (/root/reference/experiments/train_modelnet.py:37-50,99, train_shapenet.py:36-50,
// train_scanobjectnn.py:47-62, train_shapeseg.py:37-61, train_shrec.py:37-52: `transform` inside Dataset.__getitem__, the
// DataLoader's collate, `data.to(device)`).  The prepared dataset ("store": all clouds concatenated, offsets store_ptr[S+1]) stays in
// HBM; a batch is the clouds idx[0..B) gathered into pos / norm / x / batch / ptr / y / category, each point run through the op list
// of batch_math.h on its way.  Clouds may differ in size: grid = (chunks of 256 points up to max_cloud) x (B slots); every workgroup
// sums the sizes of the slots before its own in LDS to find where its cloud starts -- no second launch, no host-computed offsets.
// The draws depend on the cloud's DATASET index, never on its slot: a cloud's rows are the same bits in whatever batch it lands.
// Launch-bound: 56 bytes per point with normals (12 + 12 read, 12 + 12 + 8 written) plus labels and F * 8 bytes of features --
// 1.8 MB for 32 clouds x 1024 points, microseconds of HBM time.  Plain loads, vector stores, no atomics, no scratch.
#include "common.h"
#include "batch_math.h"

namespace {

constexpr int BA_THREADS = 256;               // = points per workgroup

struct BatchArgs {
    const float* s_pos; const float* s_norm; const float* s_x;
    const int64_t* s_ypt; const int64_t* s_ycl; const float* s_cat; const int64_t* s_ptr;
    const int64_t* idx;
    float* pos; float* norm; float* x; int64_t* batch; int32_t* ptr; int64_t* y; float* cat;
    long long S, Nt, step;
    int B, max_cloud, F, Cc, n_ops;
    unsigned seed;
    int codes[dcbatch::MAX_OPS];
    float prm[dcbatch::MAX_OPS * 3];
};

// size of the cloud in slot `slot`; an index outside the store counts as an empty cloud (nothing read, nothing written)
__device__ __forceinline__ long long ba_size(const BatchArgs& a, int slot, long long& ci, long long& start) {
    ci = a.idx[slot];
    if (ci < 0 || ci >= a.S) { start = 0; return 0; }
    start = a.s_ptr[ci];
    long long n = a.s_ptr[ci + 1] - start;
    n = n < 0 ? 0 : n;
    return n > a.max_cloud ? (long long)a.max_cloud : n;
}

__global__ __launch_bounds__(BA_THREADS) void batch_assemble_kernel(BatchArgs a) {
    __shared__ long long part[BA_THREADS / 64];
    __shared__ int codes[dcbatch::MAX_OPS];
    __shared__ float prm[dcbatch::MAX_OPS * 3], cw[dcbatch::MAX_OPS * 3];
    const int slot = blockIdx.y, tid = threadIdx.x;

    // where this cloud starts in the batch: the sizes of the slots before it
    long long mine = 0, ci, start;
    for (int s = tid; s < slot; s += BA_THREADS) mine += ba_size(a, s, ci, start);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = mine;
    const long long n = ba_size(a, slot, ci, start);
    if (tid < a.n_ops) {                       // the ops and their per-cloud draws, once per workgroup
        const int code = a.codes[tid];
        float p[3] = {a.prm[3 * tid], a.prm[3 * tid + 1], a.prm[3 * tid + 2]}, c[3];
        dcbatch::cloud_draw(code, p, a.seed, a.step, (unsigned)ci, tid, c);
        codes[tid] = code;
        prm[3 * tid] = p[0]; prm[3 * tid + 1] = p[1]; prm[3 * tid + 2] = p[2];
        cw[3 * tid] = c[0]; cw[3 * tid + 1] = c[1]; cw[3 * tid + 2] = c[2];
    }
    __syncthreads();
    long long off = 0;
#pragma unroll
    for (int w = 0; w < BA_THREADS / 64; ++w) off += part[w];

    if (blockIdx.x == 0) {                     // per-cloud outputs, by the cloud's first workgroup
        if (tid == 0) {
            if (slot == 0) a.ptr[0] = 0;
            const long long end = off + n;
            a.ptr[slot + 1] = (int32_t)(end < a.Nt ? end : a.Nt);
            if (a.s_ycl) a.y[slot] = (ci >= 0 && ci < a.S) ? a.s_ycl[ci] : 0;
        }
        if (a.s_cat && ci >= 0 && ci < a.S)
            for (int c = tid; c < a.Cc; c += BA_THREADS) a.cat[(long long)slot * a.Cc + c] = a.s_cat[ci * a.Cc + c];
    }

    const long long p = (long long)blockIdx.x * BA_THREADS + tid;      // point inside the cloud
    const long long row = off + p;                                     // its row in the batch
    if (p >= n || row >= a.Nt) return;
    const long long src = start + p;
    float px = a.s_pos[3 * src], py = a.s_pos[3 * src + 1], pz = a.s_pos[3 * src + 2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    const int has_norm = a.s_norm != nullptr;
    if (has_norm) { nx = a.s_norm[3 * src]; ny = a.s_norm[3 * src + 1]; nz = a.s_norm[3 * src + 2]; }
    for (int o = 0; o < a.n_ops; ++o)
        dcbatch::apply_op(codes[o], prm + 3 * o, cw + 3 * o, a.seed, a.step, (unsigned)ci, o, (unsigned)p, has_norm, px, py, pz, nx,
                          ny, nz);
    a.pos[3 * row] = px; a.pos[3 * row + 1] = py; a.pos[3 * row + 2] = pz;
    if (has_norm) { a.norm[3 * row] = nx; a.norm[3 * row + 1] = ny; a.norm[3 * row + 2] = nz; }
    a.batch[row] = slot;
    if (a.s_ypt) a.y[row] = a.s_ypt[src];
    if (a.s_x)
        for (int f = 0; f < a.F; ++f) a.x[row * a.F + f] = a.s_x[src * a.F + f];
}

}  // namespace

// Store: store_pos [Ns,3]; store_norm [Ns,3] or null; store_x [Ns,F] or null; store_y_point [Ns] or null; store_y_cloud [S] or
// null (at most one of the two); store_category [S,Cc] or null; store_ptr [S+1].  idx [B]: DEVICE array of cloud indices.
// B, Nt (= sum of the chosen clouds' sizes), max_cloud (>= the largest of them): host-known.  op_codes [n_ops] / op_params
// [n_ops,3]: HOST arrays (n_ops <= 8, batch_math.h).  Outputs with a null store counterpart are not touched.
DC_EXPORT int dc_batch_assemble(const float* store_pos, const float* store_norm, const float* store_x, int32_t F,
                                const int64_t* store_y_point, const int64_t* store_y_cloud, const float* store_category,
                                int32_t Cc, const int64_t* store_ptr, int64_t S, const int64_t* idx, int32_t B, int64_t Nt,
                                int32_t max_cloud, const int32_t* op_codes, const float* op_params, int32_t n_ops, int64_t seed,
                                int64_t step, float* pos, float* norm, float* x, int64_t* batch, int32_t* ptr, int64_t* y,
                                float* category, void* stream) {
    DC_REQUIRE(B >= 0 && Nt >= 0 && max_cloud >= 0 && S >= 0 && F >= 0 && Cc >= 0, "dc_batch_assemble: negative size");
    if (B == 0) return DC_OK;
    DC_REQUIRE(store_pos && store_ptr && idx && pos && batch && ptr, "dc_batch_assemble: null pointer");
    DC_REQUIRE(B <= 65535 && Nt < 2147483647L, "dc_batch_assemble: batch too large (B <= 65535 clouds, Nt < 2^31 points)");
    DC_REQUIRE(!store_norm || norm, "dc_batch_assemble: the store has normals, the output has none");
    DC_REQUIRE(!store_x || (x && F > 0), "dc_batch_assemble: the store has features, the output has none (or F = 0)");
    DC_REQUIRE(!(store_y_point && store_y_cloud), "dc_batch_assemble: labels per point AND per cloud");
    DC_REQUIRE(!(store_y_point || store_y_cloud) || y, "dc_batch_assemble: the store has labels, the output has none");
    DC_REQUIRE(!store_category || (category && Cc > 0), "dc_batch_assemble: the store has categories, the output has none (or Cc = 0)");
    DC_REQUIRE(n_ops >= 0 && n_ops <= dcbatch::MAX_OPS && (n_ops == 0 || (op_codes && op_params)),
               "dc_batch_assemble: at most 8 ops, as host arrays");
    DC_REQUIRE(seed >= 0 && seed <= 0xFFFFFFFFL && step >= 0 && step < (1LL << 61), "dc_batch_assemble: seed in [0, 2^32), step in [0, 2^61)");
    BatchArgs a;
    a.s_pos = store_pos; a.s_norm = store_norm; a.s_x = store_x; a.s_ypt = store_y_point; a.s_ycl = store_y_cloud;
    a.s_cat = store_category; a.s_ptr = store_ptr; a.idx = idx;
    a.pos = pos; a.norm = norm; a.x = x; a.batch = batch; a.ptr = ptr; a.y = y; a.cat = category;
    a.S = S; a.Nt = Nt; a.step = step; a.B = B; a.max_cloud = max_cloud; a.F = F; a.Cc = Cc; a.n_ops = n_ops;
    a.seed = (unsigned)seed;
    for (int i = 0; i < dcbatch::MAX_OPS; ++i) {
        a.codes[i] = 0;
        a.prm[3 * i] = a.prm[3 * i + 1] = a.prm[3 * i + 2] = 0.f;
    }
    for (int i = 0; i < n_ops; ++i) {
        const int code = op_codes[i];
        DC_REQUIRE(code >= dcbatch::OP_SCALE && code <= dcbatch::OP_POINT_JITTER, "dc_batch_assemble: unknown op code %d", code);
        DC_REQUIRE(code != dcbatch::OP_NORMAL_JITTER || store_norm, "dc_batch_assemble: normal jitter on a store without normals");
        if (code == dcbatch::OP_ROTATE) {
            const float ax = op_params[3 * i + 2];
            DC_REQUIRE(ax == 0.f || ax == 1.f || ax == 2.f, "dc_batch_assemble: rotation axis must be 0, 1 or 2");
        }
        a.codes[i] = code;
        for (int j = 0; j < 3; ++j) a.prm[3 * i + j] = op_params[3 * i + j];
    }
    const int chunks = max_cloud > 0 ? dc_cdiv(max_cloud, BA_THREADS) : 1;      // chunk 0 also writes ptr / y / category
    hipLaunchKernelGGL(batch_assemble_kernel, dim3(chunks, B), dim3(BA_THREADS), 0, static_cast<hipStream_t>(stream), a);
    DC_CHECK_LAUNCH("dc_batch_assemble");
    return DC_OK;
}
