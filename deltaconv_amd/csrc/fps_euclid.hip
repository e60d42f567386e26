// Euclidean farthest-point sampling of a batch of clouds inside the step: what torch_cluster.fps / PointNet++ set abstraction do,
// with the rules of fps_euclid_math.h (the contract's fp32 distance, first index of the maximum), so the picks are a function of
// the inputs only and a numpy restatement reproduces them.  One launch, one workgroup per cloud, every pick inside the launch.
//
//   registers  a thread owns PPT points, ids tid, tid + T, tid + 2T, ...: x, y, z and the running minimum md, 4 VGPRs per point.
//              PPT and the workgroup size T are template parameters picked on the host from max_cloud, so every array index is
//              static and nothing goes to scratch (16 points x 4 + temporaries stays below the 128 VGPRs 1024 threads leave).
//              Slots past the cloud hold md = PAD, below every real point, and are never picked.
//   a pick     every thread updates its points against the pick's coordinates and folds them into its largest 64-bit key
//              (image(md) << 32 | ~id: one unsigned maximum = largest md, then lowest id), keeping that point's coordinates
//              beside it.  Four DPP steps and four lane reads give the wave's key (wave_max; against six __shfl_xor steps, which
//              compile to ds_bpermute pairs: 7 .. 19 % of a pick); the one lane that holds it writes key and
//              coordinates to the wave's LDS slot.  ONE barrier; then every thread takes the maximum over the waves' slots and
//              reads the winner's coordinates: the next pick, the same in every thread.  The slots are double-buffered by the
//              parity of the pick, so a slot is rewritten only after a barrier that every reader of it has passed.
//   LDS        2 x waves x (8 + 12) bytes.  No global atomics, no workspace, nothing read on the host: launch sizes depend on
//              B and max_cloud alone, and a captured launch replays on positions written in place.
#include "common.h"
#include "fps_euclid_math.h"
#include "wave_key.h"

namespace {

template <int PPT, int T>
__global__ __launch_bounds__(T) void fps_euclid_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr,
                                                        const int64_t* __restrict__ optr, const int32_t* __restrict__ start,
                                                        int64_t* __restrict__ rows, int max_samples) {
    constexpr int W = T / 64;
    __shared__ u64 s_key[2][W];
    __shared__ float s_c[2][W][3];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const long long base = ptr[b];
    long long nn = ptr[b + 1] - base;
    nn = nn < 0 ? 0 : (nn > PPT * T ? PPT * T : nn);           // a cloud above max_cloud: its first PPT * T points (never out of bounds)
    const int n = (int)nn;
    const long long o = optr[b];
    long long mm = optr[b + 1] - o;
    mm = mm < 0 ? 0 : (mm > max_samples ? max_samples : mm);
    const int picks = mm < n ? (int)mm : n;

    float x[PPT], y[PPT], z[PPT], md[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int id = j * T + tid;
        const bool live = id < n;
        const float* p = pos + 3 * (base + (live ? id : 0));
        x[j] = live ? p[0] : 0.f;
        y[j] = live ? p[1] : 0.f;
        z[j] = live ? p[2] : 0.f;
        md[j] = live ? dcfpse::init_md(x[j], y[j], z[j]) : dcfpse::PAD;
    }
    int cur = 0;
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (n > 0) {
        cur = dcfpse::clamp_start(start ? start[b] : 0, n);
        const float* p = pos + 3 * (base + cur);
        cx = p[0]; cy = p[1]; cz = p[2];
    }
    for (int r = 0; r < picks; ++r) {
        if (tid == 0) rows[o + r] = base + cur;
        if (r + 1 == picks) break;                             // the last pick selects nothing
        // a thread's ids ascend with j and md is never NaN: "largest md, then lowest id" inside the thread is a strict
        // greater-than in ascending j; the 64-bit key is formed once, for the thread's winner
        const bool mine = tid == (cur & (T - 1));
        const int cj = cur / T;
        float bmd = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bj = 0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            md[j] = dcfpse::update(md[j], mine && cj == j, x[j], y[j], z[j], cx, cy, cz);
            const bool better = j == 0 || md[j] > bmd;
            bmd = better ? md[j] : bmd;
            bx = better ? x[j] : bx;
            by = better ? y[j] : by;
            bz = better ? z[j] : bz;
            bj = better ? j : bj;
        }
        const u64 bk = dcfpse::key(bmd, bj * T + tid);
        const u64 wk = wave_max(bk);
        const int par = r & 1;
        if (bk == wk) {                                        // one lane: the ids in the keys are pairwise distinct
            s_key[par][wave] = wk;
            s_c[par][wave][0] = bx;
            s_c[par][wave][1] = by;
            s_c[par][wave][2] = bz;
        }
        __syncthreads();
        u64 best = s_key[par][0];
        int bw = 0;
#pragma unroll
        for (int w = 1; w < W; ++w) {
            const u64 k = s_key[par][w];
            const bool better = k > best;
            best = better ? k : best;
            bw = better ? w : bw;
        }
        cur = dcfpse::key_id(best);
        cx = s_c[par][bw][0];
        cy = s_c[par][bw][1];
        cz = s_c[par][bw][2];
    }
    for (long long r = picks + tid; r < mm; r += T) rows[o + r] = -1;      // pick indices past the cloud
}

template <int PPT, int T>
void fps_euclid_launch(const float* pos, const int64_t* ptr, const int64_t* optr, int B, const int32_t* start, int64_t* rows,
                       int max_samples, hipStream_t s) {
    hipLaunchKernelGGL((fps_euclid_kernel<PPT, T>), dim3(B), dim3(T), 0, s, pos, ptr, optr, start, rows, max_samples);
}

}  // namespace

DC_EXPORT int dc_fps_batch(const float* pos, const int64_t* ptr, const int64_t* optr, int32_t B, int32_t max_cloud,
                           int32_t max_samples, const int32_t* start, int64_t* rows, void* stream) {
    DC_REQUIRE(B >= 0, "dc_fps_batch: B = %d clouds", B);
    DC_REQUIRE(max_cloud >= 0 && max_cloud <= dcfpse::MAX_POINTS,
               "dc_fps_batch: max_cloud = %d, the sampler takes clouds of at most %d points (DC_FPS_EUCLID_MAX_POINTS)", max_cloud,
               dcfpse::MAX_POINTS);
    DC_REQUIRE(max_samples >= 0, "dc_fps_batch: max_samples = %d", max_samples);
    if (B == 0 || max_samples == 0) return DC_OK;
    DC_REQUIRE(pos && ptr && optr && rows, "dc_fps_batch: null pointer (pos, ptr, optr, rows)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (max_cloud <= 64) fps_euclid_launch<1, 64>(pos, ptr, optr, B, start, rows, max_samples, s);
    else if (max_cloud <= 1024) fps_euclid_launch<4, 256>(pos, ptr, optr, B, start, rows, max_samples, s);
    else if (max_cloud <= 2048) fps_euclid_launch<8, 256>(pos, ptr, optr, B, start, rows, max_samples, s);
    else if (max_cloud <= 4096) fps_euclid_launch<4, 1024>(pos, ptr, optr, B, start, rows, max_samples, s);
    else if (max_cloud <= 8192) fps_euclid_launch<8, 1024>(pos, ptr, optr, B, start, rows, max_samples, s);
    else fps_euclid_launch<16, 1024>(pos, ptr, optr, B, start, rows, max_samples, s);
    DC_CHECK_LAUNCH("dc_fps_batch");
    return DC_OK;
}
