// Exact Euclidean farthest-point sampling over a uniform cell grid: dc_fps_grid, the arguments and outputs of dc_fps_batch
// (fps_euclid.hip) for clouds above the 16 384 points that fit the registers of one workgroup, up to DC_FPS_GRID_MAX_POINTS.  The
// same picks bit for bit: state, update and selection key are fps_euclid_math.h's; the grid only decides which points a pick
// looks at.  The rule, its proof and the serial reference are csrc/fps_grid_math.h (shared with the g++ host check,
// tests/hostcheck_fps_grid).
//
// Six launches, stream-ordered, every launch size from host-known sizes (capturable; nothing is read on the host):
//   the grid build of knn_grid.hip (knn_grid_build.h: box, zero, count, sum / scan, fill) -> per cloud its Grid, the cell starts and
//   the points in cell order (Pt, 16 bytes)
//   fps_grid_kernel   ONE workgroup of 1 024 threads per cloud, every pick inside the launch.  A cloud never leaves its workgroup:
//                     nothing is handed between workgroups, nothing waits on another workgroup.  Per cloud in the workspace: md in
//                     cell order (4 bytes a point) and one 64-bit key per cell (the maximum of dcfpse::key over its points); in
//                     LDS one key per block of 64 consecutive cells, at most 64 KiB for the 2 n cells of a cloud at the cap.
//     init    md = +inf (only finite points have a slot), then the cell keys and the block keys of the whole grid
//     a pick  (a1) the box as runs of consecutive cells = contiguous runs of points: a wave per run, a lane per point (runs of 512
//                  cells and more: the whole workgroup per run -- the whole grid is ONE run, a flat pass); update, store the md that
//                  changed
//             (a2) barrier; the cells of the box, 64 at a time per wave: a lane folds its cell's points into the cell key; a cell of
//                  more than 16 points is taken by the whole wave instead, 64 points a pass and wave_max
//             (b)  barrier; a wave per block that holds a cell of a run: wave_max over its 64 cell keys -> LDS.  Two runs that
//                  land in one block write the same value
//             (c)  barrier; the maximum over the block keys (per thread, wave_max, one slot per wave, barrier) is the next pick:
//                  its id is in the key, D = its md is in the key, its coordinates are read from pos, its cell is cell_axis of them
//     tail    when the maximum is no live key, the rows with a non-finite coordinate in ascending id (an ordered compaction)
// md and the cell keys are written and read by different waves of the workgroup across __syncthreads(): every access is a relaxed
// workgroup-scope atomic load / store (vector path, nothing cached in registers across a barrier, never the scalar cache); the
// pointers carry no const / __restrict__.  No read-modify-write atomics outside the shared grid build, no floating-point atomics.
// stats: the box's populations and cell counts, whatever shape the walk takes (fps_grid_math.h).
#include "common.h"
#include "fps_grid_math.h"
#include "knn_grid_build.h"
#include "wave_key.h"

namespace {
using dcgrid::Grid;
using dcgrid::Pt;
using dcfpsg::Box;

constexpr int T = 1024, W = T / 64;
constexpr int COOP_CELLS = 512;               // a run of this many cells is walked by the whole workgroup
constexpr int HEAVY = 16;                     // a cell of more points is folded by its whole wave
constexpr size_t LDS_HEAD = 2 * W * 8;        // the waves' key slots and counters, ahead of the block keys

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
struct Layout {
    size_t md, ckey, total;
};
Layout layout(long long n, long long B) {
    Layout L;
    L.md = up16(dc_grid_build_bytes(n, B));
    L.ckey = up16(L.md + (size_t)n * 4);
    L.total = L.ckey + (size_t)(2 * n + B) * 8;
    return L;
}
long long capacity(size_t bytes, long long B) {
    if (layout(0, B).total > bytes) return -1;
    long long lo = 0, hi = 0x7fffffffll;
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (layout(mid, B).total <= bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
size_t lds_bytes(long long max_cloud) { return LDS_HEAD + (size_t)dcfpsg::blocks_of((int)(max_cloud > 0 ? 2 * max_cloud : 1)) * 8; }

__device__ __forceinline__ float ld_md(float* p) {
    return __uint_as_float(__hip_atomic_load(reinterpret_cast<unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
__device__ __forceinline__ void st_md(float* p, float v) {
    __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ u64 ld_key(u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_key(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// One cloud's view of the workspace
struct Cloud {
    Grid G;
    const int64_t* cstart;                    // [cells + 1] slots of pts / md
    const Pt* pts;
    float* md;
    u64* ckey;                                // [cells]
    u64* s_blk;                               // LDS [blocks_of(cells)]
    long long cap;
    int tid, lane, wave;
    // first slot of cell c, cut to the workspace (a slot is never indexed outside [0, cap))
    __device__ __forceinline__ long long slot(int c) const {
        const long long v = cstart[c];
        return v < 0 ? 0 : (v > cap ? cap : v);
    }
    __device__ __forceinline__ u64 key_at(long long j) const { return dcfpse::key(ld_md(md + j), pts[j].id); }
};

// (a1) every point of the box against the pick -> this thread's share of the box's population (lane 0 of a wave / thread 0 counts)
__device__ __forceinline__ long long update_box(const Cloud& c, const Box& box, int cur, float cx, float cy, float cz) {
    long long pop = 0;
    const bool coop = box.run_cells >= COOP_CELLS;
    const int first = coop ? 0 : c.wave, step = coop ? 1 : W, width = coop ? T : 64, me = coop ? c.tid : c.lane;
    for (int i = first; i < box.runs; i += step) {
        const int c0 = dcfpsg::run_first(c.G, box, i);
        const long long s = c.slot(c0), e = c.slot(c0 + box.run_cells);
        for (long long j = s + me; j < e; j += width) {
            const Pt p = c.pts[j];
            const float old = ld_md(c.md + j);
            const float now = dcfpse::update(old, p.id == cur, p.x, p.y, p.z, cx, cy, cz);
            if (now != old) st_md(c.md + j, now);
        }
        if (me == 0 && e > s) pop += e - s;
    }
    return pop;
}

// (a2) the key of every cell of the box from the md of its points
__device__ __forceinline__ void cell_keys(const Cloud& c, const Box& box) {
    const long long total = dcfpsg::box_cells(box);
    for (long long g = (long long)c.wave * 64; g < total; g += W * 64) {          // wave-uniform
        const long long i = g + c.lane;
        const bool have = i < total;
        const int cell = have ? dcfpsg::box_cell(c.G, box, i) : 0;
        const long long s = have ? c.slot(cell) : 0, e = have ? c.slot(cell + 1) : 0;
        const bool heavy = e - s > HEAVY;
        u64 k = 0ull;
        if (!heavy)
            for (long long j = s; j < e; ++j) {
                const u64 kj = c.key_at(j);
                k = kj > k ? kj : k;
            }
        u64 todo = __ballot(heavy);
        while (todo) {                                                            // wave-uniform: all 64 lanes reach wave_max
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const long long hs = __shfl(s, src, 64), he = __shfl(e, src, 64);
            u64 kk = 0ull;
            for (long long j = hs + c.lane; j < he; j += 64) {
                const u64 kj = c.key_at(j);
                kk = kj > kk ? kj : kk;
            }
            kk = wave_max(kk);
            k = c.lane == src ? kk : k;
        }
        if (have) st_key(c.ckey + cell, k);
    }
}

// (b) the key of every block that holds a cell of the box
__device__ __forceinline__ void block_keys(const Cloud& c, const Box& box) {
    const int per_run = (box.run_cells + dcfpsg::BLOCK_CELLS - 2) / dcfpsg::BLOCK_CELLS + 1;      // blocks a run can touch
    const long long items = (long long)box.runs * per_run;
    for (long long it = c.wave; it < items; it += W) {                            // wave-uniform
        const int c0 = dcfpsg::run_first(c.G, box, (int)(it / per_run));
        const int blk = c0 / dcfpsg::BLOCK_CELLS + (int)(it % per_run);
        if (blk > (c0 + box.run_cells - 1) / dcfpsg::BLOCK_CELLS) continue;
        const int cell = blk * dcfpsg::BLOCK_CELLS + c.lane;
        const u64 k = wave_max(cell < c.G.cells ? ld_key(c.ckey + cell) : 0ull);
        if (c.lane == 0) c.s_blk[blk] = k;
    }
}

// (c) the maximum over the block keys, the same in every thread
__device__ __forceinline__ u64 select(const Cloud& c, u64* s_slot) {
    __syncthreads();                                                              // the block keys are written; the slots are read
    u64 k = 0ull;
    const int nblk = dcfpsg::blocks_of(c.G.cells);
    for (int i = c.tid; i < nblk; i += T) k = c.s_blk[i] > k ? c.s_blk[i] : k;
    k = wave_max(k);
    if (c.lane == 0) s_slot[c.wave] = k;
    __syncthreads();
    u64 best = s_slot[0];
#pragma unroll
    for (int w = 1; w < W; ++w) best = s_slot[w] > best ? s_slot[w] : best;
    return best;
}

__global__ __launch_bounds__(T) void fps_grid_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr,
                                                     const int64_t* __restrict__ optr, const int32_t* __restrict__ start,
                                                     int64_t* __restrict__ rows, int64_t* __restrict__ stats, int max_samples,
                                                     int max_cloud, const Grid* __restrict__ grids, const int64_t* __restrict__ lptr,
                                                     const Pt* __restrict__ pts, long long cap, float* md, u64* ckey) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* s_slot = reinterpret_cast<u64*>(smem);                                   // [W]
    long long* s_cnt = reinterpret_cast<long long*>(smem + W * 8);                // [W]
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long base = ptr[b], n64 = ptr[b + 1] - base, off = base - ptr[0];
    // a cloud the build left out (outside the workspace's capacity) or larger than max_cloud claims (the LDS table is sized by it)
    const bool ok = n64 >= 0 && off >= 0 && off + n64 <= cap && n64 <= max_cloud;
    const int n = ok ? (int)n64 : 0;
    const long long o = optr[b];
    long long mm = optr[b + 1] - o;
    mm = mm < 0 ? 0 : (mm > max_samples ? max_samples : mm);
    const int count = mm < n ? (int)mm : n;
    long long pop = 0, ncell = 0;
    if (count > 0) {                                                              // block-uniform
        Cloud c;
        c.G = grids[b];
        c.cstart = lptr + 2 * off + b;
        c.pts = pts;
        c.md = md;
        c.ckey = ckey + 2 * off + b;
        c.s_blk = reinterpret_cast<u64*>(smem + LDS_HEAD);
        c.cap = cap;
        c.tid = tid;
        c.lane = tid & 63;
        c.wave = tid >> 6;
        const Box all = dcfpsg::make_box(c.G, 0, 0, 0, dcgrid::MAX_AXIS);
        for (long long j = c.slot(0) + tid, e = c.slot(c.G.cells); j < e; j += T) st_md(md + j, dcfpse::inf());
        __syncthreads();
        cell_keys(c, all);
        __syncthreads();
        block_keys(c, all);

        const int s0 = dcfpse::clamp_start(start ? start[b] : 0, n);
        int cur = s0, r = 0;
        float D = dcfpse::inf();
        bool tail = false;
        for (;;) {
            if (tid == 0) rows[o + r] = base + cur;
            if (++r == count) break;                                              // the last pick updates nothing
            const float* p = pos + 3 * (base + cur);
            const float cx = p[0], cy = p[1], cz = p[2];
            if (dcgrid::finite3(cx, cy, cz)) {
                const int ix = dcgrid::cell_axis(cx, c.G.lo[0], c.G.inv_h[0], c.G.g[0]);
                const int iy = dcgrid::cell_axis(cy, c.G.lo[1], c.G.inv_h[1], c.G.g[1]);
                const int iz = dcgrid::cell_axis(cz, c.G.lo[2], c.G.inv_h[2], c.G.g[2]);
                const int R = dcfpsg::box_radius(D, c.G.min_h, dcfpsg::cover_radius(c.G, ix, iy, iz));
                const Box box = dcfpsg::make_box(c.G, ix, iy, iz, R);
                pop += update_box(c, box, cur, cx, cy, cz);
                ncell += dcfpsg::box_cells(box);
                __syncthreads();
                cell_keys(c, box);
                __syncthreads();
                block_keys(c, box);
            }
            const u64 best = select(c, s_slot);
            if (!dcfpsg::key_live(best)) {
                tail = true;
                break;
            }
            cur = dcfpse::key_id(best);
            D = dcfpsg::key_md(best);
        }
        if (tail) {                                // every finite point is taken: the non-finite rows in ascending id, without the start
            int* s_w = reinterpret_cast<int*>(s_cnt);
            for (int i0 = 0; i0 < n && r < count; i0 += T) {                      // r is block-uniform
                const int i = i0 + tid;
                bool flag = false;
                if (i < n && i != s0) {
                    const float* p = pos + 3 * (base + i);
                    flag = !dcgrid::finite3(p[0], p[1], p[2]);
                }
                const u64 bal = __ballot(flag);
                if (c.lane == 0) s_w[c.wave] = __popcll(bal);
                __syncthreads();
                int before = __popcll(bal & ((1ull << c.lane) - 1ull)), total = 0;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    before += w < c.wave ? s_w[w] : 0;
                    total += s_w[w];
                }
                if (flag && r + before < count) rows[o + r + before] = base + i;
                r = r + total < count ? r + total : count;
                __syncthreads();
            }
        }
    }
    for (long long r = count + tid; r < mm; r += T) rows[o + r] = -1;             // pick indices past the cloud
    if (stats) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) pop += __shfl_xor(pop, s, 64);
        __syncthreads();
        if ((tid & 63) == 0) s_cnt[tid >> 6] = pop;
        __syncthreads();
        if (tid == 0) {
            long long sum = 0;
            for (int w = 0; w < W; ++w) sum += s_cnt[w];
            stats[2 * b] = sum;
            stats[2 * b + 1] = ncell;
        }
    }
}

bool good_target(float t) { return t > 0.f && dcgrid::finite1(t); }

}  // namespace

DC_EXPORT size_t dc_fps_grid_workspace_bytes(int64_t num_points, int32_t num_clouds) {
    if (num_points < 0 || num_points > 0x7fffffffll || num_clouds < 0) return 0;
    return layout(num_points, num_clouds).total;
}

DC_EXPORT int dc_fps_grid(const float* pos, const int64_t* ptr, const int64_t* optr, int32_t B, int32_t max_cloud, int32_t max_samples,
                          const int32_t* start, float target, int64_t* rows, int64_t* stats, void* workspace, size_t workspace_bytes,
                          void* stream) {
    DC_REQUIRE(B >= 0, "dc_fps_grid: B = %d clouds", B);
    DC_REQUIRE(max_cloud >= 0 && max_cloud <= dcfpsg::MAX_POINTS,
               "dc_fps_grid: max_cloud = %d, the sampler takes clouds of at most %d points (DC_FPS_GRID_MAX_POINTS)", max_cloud,
               dcfpsg::MAX_POINTS);
    DC_REQUIRE(max_samples >= 0, "dc_fps_grid: max_samples = %d", max_samples);
    DC_REQUIRE(good_target(target), "dc_fps_grid: target = %g must be positive and finite", (double)target);
    if (B == 0 || max_samples == 0) return DC_OK;
    DC_REQUIRE(pos && ptr && optr && rows, "dc_fps_grid: null pointer (pos, ptr, optr, rows)");
    DC_REQUIRE(workspace, "dc_fps_grid: null workspace");
    DC_REQUIRE(aligned_to(workspace, 16), "dc_fps_grid: workspace must be 16-byte aligned");
    long long cap = capacity(workspace_bytes, B);
    DC_REQUIRE(cap >= max_cloud, "dc_fps_grid: workspace of %zu bytes is too small (dc_fps_grid_workspace_bytes of all points of the call)",
               workspace_bytes);
    const long long most = (long long)B * max_cloud;                              // no call holds more points than this
    cap = cap < most ? cap : most;
    const Layout L = layout(cap, B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DcGridBuild g;
    const int rc = dc_grid_build("dc_fps_grid", pos, ptr, B, target, workspace, cap, s, &g);
    if (rc != DC_OK) return rc;
    char* w = static_cast<char*>(workspace);
    static unsigned long long attr_done = 0;      // > 64 KiB of dynamic LDS at the cap needs an explicit opt-in (per kernel and device)
    if (!dc_ensure_lds(&attr_done, reinterpret_cast<const void*>(&fps_grid_kernel), lds_bytes(dcfpsg::MAX_POINTS), "dc_fps_grid")) {
        DC_CHECK_LAUNCH("dc_fps_grid");
    }
    hipLaunchKernelGGL(fps_grid_kernel, dim3(B), dim3(T), lds_bytes(max_cloud), s, pos, ptr, optr, start, rows, stats, max_samples,
                       max_cloud, g.grids, g.cell_start, g.pts, g.cap, reinterpret_cast<float*>(w + L.md),
                       reinterpret_cast<u64*>(w + L.ckey));
    DC_CHECK_LAUNCH("dc_fps_grid");
    return DC_OK;
}
