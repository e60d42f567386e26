// Surface sampling of a batch of device-resident triangle meshes: what the reference's data preparation does on the host one
// shape at a time (deltaconv/transforms/sample_points.py:22-59 inside the pre_transform of experiments/train_modelnet.py:30-34,
// train_shrec.py:30-34, train_shapeseg.py:28-34).  Two launches:
//   mesh_cdf_kernel     one workgroup per mesh.  Pass 1 loops over the faces and forms the largest fp64 area (wave shuffles, then
//                       LDS); pass 2 recomputes the area, cuts it to an integer weight in [0, 2^32] and writes the inclusive
//                       uint64 sums to the workspace -- a workgroup scan of MESH_SCAN_FACES faces per iteration with a running
//                       carry.  Integer sums and a maximum do not depend on their order: the cdf is a function of the mesh only.
//   mesh_sample_kernel  (chunks of 256 samples) x (meshes), one sample per thread: Philox draw, binary search of the mesh's cdf,
//                       gather of the three vertex rows, point / normal / label / face id written.
// Plain loops, no waiting across workgroups, no atomics.  The arithmetic is csrc/mesh_math.h (shared with tests/hostcheck_mesh).
#include "common.h"
#include "mesh_math.h"

namespace {

typedef dcmesh::u64 u64;
constexpr int CDF_T = 1024;                   // threads of a cdf workgroup
constexpr int MESH_SCAN_FACES = CDF_T;        // faces one scan iteration covers: one per thread (dc_mesh_scan_faces)
constexpr int SAMPLE_T = 256;                 // samples of a sampling workgroup
constexpr int CDF_WAVES = CDF_T / 64;

__device__ __forceinline__ double area_of(const float* __restrict__ v, long long V, const int32_t* __restrict__ fc, long long f) {
    return dcmesh::face_area(v, V, fc[3 * f], fc[3 * f + 1], fc[3 * f + 2]);
}

// cap: faces the workspace holds.  A mesh whose cdf would not fit (a caller that sized the workspace for fewer faces than fptr
// spans) is skipped and reports total = -1; the sampling kernel skips it too.
__global__ __launch_bounds__(CDF_T) void mesh_cdf_kernel(const float* __restrict__ vert, const int32_t* __restrict__ face,
                                                         const int64_t* __restrict__ vptr, const int64_t* __restrict__ fptr,
                                                         u64* __restrict__ cdf, long long cap, int64_t* __restrict__ total) {
    __shared__ double s_max[CDF_WAVES];
    __shared__ u64 s_sum[CDF_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long vbase = vptr[b], V = vptr[b + 1] - vbase;
    const long long fbase = fptr[b], F = fptr[b + 1] - fbase, rel = fbase - fptr[0];
    if (F <= 0 || V <= 0 || rel < 0 || rel + F > cap) {          // the whole workgroup: no barrier is left behind
        if (tid == 0 && total) total[b] = (F <= 0 || V <= 0) ? 0 : -1;
        return;
    }
    const float* v = vert + 3 * vbase;
    const int32_t* fc = face + 3 * fbase;
    u64* out = cdf + rel;
    // pass 1: the largest area
    double m = 0.0;
    for (long long f = tid; f < F; f += CDF_T) m = fmax(m, area_of(v, V, fc, f));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    double amax = s_max[0];
#pragma unroll
    for (int k = 1; k < CDF_WAVES; ++k) amax = fmax(amax, s_max[k]);
    // pass 2: weights and their inclusive sums
    u64 carry = 0;                                               // the same in every thread
    for (long long f0 = 0; f0 < F; f0 += MESH_SCAN_FACES) {
        const long long f = f0 + tid;
        u64 s = f < F ? dcmesh::face_weight(area_of(v, V, fc, f), amax) : 0ull;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 up = __shfl_up(s, o, 64);
            if (lane >= o) s += up;
        }
        if (lane == 63) s_sum[wave] = s;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < CDF_WAVES; ++k) {
            const u64 t = s_sum[k];
            if (k < wave) before += t;
            all += t;
        }
        if (f < F) out[f] = carry + before + s;
        carry += all;
        __syncthreads();                                         // s_sum is read before the next iteration writes it
    }
    if (tid == 0 && total) total[b] = (int64_t)carry;
}

__global__ __launch_bounds__(SAMPLE_T) void mesh_sample_kernel(const float* __restrict__ vert, const int32_t* __restrict__ face,
                                                               const int64_t* __restrict__ vptr, const int64_t* __restrict__ fptr,
                                                               const u64* __restrict__ cdf, long long cap, unsigned first_mesh,
                                                               int num, unsigned seed, long long round,
                                                               const int64_t* __restrict__ y_vert, float* __restrict__ pos,
                                                               float* __restrict__ norm, int64_t* __restrict__ y,
                                                               int32_t* __restrict__ face_id) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * SAMPLE_T + threadIdx.x;
    if (j >= num) return;
    const long long vbase = vptr[b], V = vptr[b + 1] - vbase;
    const long long fbase = fptr[b], F = fptr[b + 1] - fbase, rel = fbase - fptr[0];
    const long long o = (long long)b * num + j;
    float p[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, f12[2];
    long long lab = -1;
    int fid = -1;
    if (F > 0 && V > 0 && rel >= 0 && rel + F <= cap)
        dcmesh::sample_one(vert + 3 * vbase, V, face + 3 * fbase, F, cdf + rel,
                           (y && y_vert) ? reinterpret_cast<const long long*>(y_vert + vbase) : nullptr, seed, round,
                           first_mesh + (unsigned)b, (unsigned)j, p, n, &lab, &fid, f12);
    pos[3 * o] = p[0]; pos[3 * o + 1] = p[1]; pos[3 * o + 2] = p[2];
    if (norm) { norm[3 * o] = n[0]; norm[3 * o + 1] = n[1]; norm[3 * o + 2] = n[2]; }
    if (y) y[o] = lab;
    if (face_id) face_id[o] = fid;
}

}  // namespace

DC_EXPORT size_t dc_mesh_sample_workspace_bytes(int64_t F_total) { return (size_t)dcmesh::workspace_bytes(F_total); }

DC_EXPORT int32_t dc_mesh_scan_faces(void) { return MESH_SCAN_FACES; }

DC_EXPORT int dc_mesh_sample(const float* vert, const int32_t* face, const int64_t* vptr, const int64_t* fptr, int32_t B,
                             int64_t first_mesh_index, int32_t num, int64_t seed, int64_t round, const int64_t* y_vert, float* pos,
                             float* norm, int64_t* y, int32_t* face_id, int64_t* total, void* workspace, size_t workspace_bytes,
                             void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_mesh_sample: B = %d meshes, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(num >= 1, "dc_mesh_sample: num = %d samples per mesh, at least 1", num);
    DC_REQUIRE(seed >= 0 && seed < (1ll << 32), "dc_mesh_sample: seed = %lld outside [0, 2^32)", (long long)seed);
    DC_REQUIRE(round >= 0, "dc_mesh_sample: round = %lld is negative", (long long)round);
    DC_REQUIRE(first_mesh_index >= 0 && first_mesh_index <= (1ll << 32) - B,
               "dc_mesh_sample: dataset indices from %lld on for %d meshes leave [0, 2^32)", (long long)first_mesh_index, B);
    if (B == 0) return DC_OK;
    DC_REQUIRE(vert && face && vptr && fptr && pos, "dc_mesh_sample: null pointer (vert, face, vptr, fptr, pos)");
    DC_REQUIRE(!y || y_vert, "dc_mesh_sample: y needs the per-vertex labels y_vert");
    // every mesh has at least one face: the least a workspace for B meshes can be.  The offsets live on the device, so the kernels
    // hold every mesh to the capacity handed over (a mesh that does not fit is skipped and reports total = -1).
    if (!workspace || workspace_bytes < dcmesh::workspace_bytes(B)) {
        dc_set_error("dc_mesh_sample: workspace of %zu bytes for %d meshes; it holds 8 bytes per face of the call "
                     "(dc_mesh_sample_workspace_bytes)", workspace ? workspace_bytes : (size_t)0, B);
        return DC_ERR_WORKSPACE;
    }
    DC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "dc_mesh_sample: workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    u64* cdf = static_cast<u64*>(workspace);
    const long long cap = (long long)(workspace_bytes / 8);
    hipLaunchKernelGGL(mesh_cdf_kernel, dim3(B), dim3(CDF_T), 0, s, vert, face, vptr, fptr, cdf, cap, total);
    DC_CHECK_LAUNCH("dc_mesh_sample (cdf)");
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(dc_cdiv(num, SAMPLE_T), B), dim3(SAMPLE_T), 0, s, vert, face, vptr, fptr, cdf, cap,
                       (unsigned)first_mesh_index, (int)num, (unsigned)seed, (long long)round, y_vert, pos, norm, y, face_id);
    DC_CHECK_LAUNCH("dc_mesh_sample (sampling)");
    return DC_OK;
}
