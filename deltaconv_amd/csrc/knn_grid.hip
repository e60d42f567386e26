// Exact k-nearest-neighbour search over a uniform cell grid: dc_knn_grid (the arguments and outputs of dc_knn) and
// dc_knn_cross_grid (those of dc_knn_cross) for clouds where the n^2 distance evaluations of the brute-force kernels dominate.
// The same neighbours in the same order, bit for bit: the arithmetic, the grid rule and the proof of the stopping bound are
// csrc/knn_grid_math.h (shared with the g++ host check, tests/hostcheck_knn_grid).
//
// Seven launches, stream-ordered, every launch size from host-known sizes (capturable; the bounding boxes live on the device):
//   grid_box_kernel     one workgroup per reference cloud: fp32 min / max and count over the points with three finite coordinates
//                       (order-independent), then one thread runs dcgrid::make_grid -> the cloud's 48-byte Grid record
//   dc_zero_words       the per-cell counters of all clouds
//   grid_count_kernel   one thread per reference row: its cloud by bisection of the offsets, its cell, an integer atomic on the counter
//   list_sum / list_scan (list_scan.h)  exclusive scan of the counters over ALL cells of the call -> cell starts and fill cursors
//   grid_fill_kernel    one thread per reference row: takes a slot of its cell, writes (x, y, z, local id) there -- the points IN CELL
//                       ORDER, 16 bytes each, so a search reads contiguous runs.  The order inside a cell depends on the atomics;
//                       it cannot reach the result, which is sorted by the explicit key (d2, id)
//   grid_self_kernel / grid_cross_kernel   one query per thread, dcgrid::search: rings of cells, a sorted list of K keys in
//                       registers.  The self form takes its queries IN CELL ORDER (thread i of a cloud owns the i-th point of the
//                       cell-ordered array), so the lanes of a wave walk the same cells and their loads coalesce into broadcasts;
//                       the cross form takes its queries as they come (a sampled cloud is small next to its reference).
// Cell c of cloud b is counter 2 * (ptr[b] - ptr[0]) + b + c: a cloud of n points has at most max(1, 2 n) cells, so the layout
// needs no pass of its own and 2 N + B counters serve any call of N points in B clouds.
//
// Latency-bound rather than bandwidth-bound: per query about `target` * 27 .. 125 candidates of 16 bytes from L2.  What the grid
// does not help with: one far outlier stretches the box until the cloud falls into a few cells; the search then degrades towards
// brute force on one thread per query -- correct, slow.
#include "common.h"
#include "knn_grid_build.h"
#include "knn_grid_math.h"
#include "list_scan.h"

namespace {
using dcgrid::Grid;
using dcgrid::Pt;

constexpr int G_THREADS = 256;
constexpr int BOX_THREADS = 1024;
constexpr long long G_MAX_POINTS = 0x7fffffffll;     // ids are int32
static_assert(sizeof(Grid) == 48 && sizeof(Pt) == 16, "workspace layout");

struct Layout {
    size_t grids, cnt, part, lptr, pts, total;
    long long rows;
};
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
Layout layout(long long n, long long B) {
    Layout L;
    L.rows = 2 * n + B;
    L.grids = 0;
    L.cnt = up16((size_t)B * sizeof(Grid));
    L.part = L.cnt + (size_t)L.rows * 8;
    L.lptr = L.part + (size_t)((L.rows + SC_THREADS - 1) / SC_THREADS) * 8;
    L.pts = up16(L.lptr + (size_t)(L.rows + 1) * 8);
    L.total = L.pts + (size_t)n * sizeof(Pt);
    return L;
}
// the largest point count whose layout fits `bytes` (-1: not even an empty call)
long long capacity(size_t bytes, long long B) {
    if (layout(0, B).total > bytes) return -1;
    long long lo = 0, hi = G_MAX_POINTS;
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (layout(mid, B).total <= bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Reference cloud b of the call: first row, rows, offset behind the call's first row; ok: it lies inside the workspace's capacity
struct Cloud {
    long long base, n, off;
    bool ok;
};
template <class PtrT>
__device__ __forceinline__ Cloud cloud_of(const PtrT* __restrict__ ptr, int b, long long cap) {
    Cloud c;
    c.base = ptr[b];
    c.n = (long long)ptr[b + 1] - c.base;
    c.off = c.base - (long long)ptr[0];
    c.ok = c.n >= 0 && c.off >= 0 && c.off + c.n <= cap;
    return c;
}
// the cloud of absolute row `row`: the last b with ptr[b] <= row (empty clouds are passed over), -1 outside every cloud
template <class PtrT>
__device__ __forceinline__ int cloud_index(const PtrT* __restrict__ ptr, int B, long long row) {
    int lo = 0, hi = B;                       // first b in [0, B] with ptr[b] > row
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)ptr[mid] <= row) lo = mid + 1;
        else hi = mid;
    }
    const int b = lo - 1;
    return (b >= 0 && b < B && row < (long long)ptr[b + 1]) ? b : -1;
}

template <class PtrT>
__global__ __launch_bounds__(BOX_THREADS) void grid_box_kernel(const float* __restrict__ pos, const PtrT* __restrict__ ptr,
                                                               long long cap, float target, Grid* __restrict__ grids) {
    __shared__ float red[6][BOX_THREADS / 64];
    __shared__ int redc[BOX_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Cloud c = cloud_of(ptr, b, cap);
    const long long n = c.ok ? c.n : 0;
    float lo[3] = {dcgrid::inf(), dcgrid::inf(), dcgrid::inf()};
    float hi[3] = {-dcgrid::inf(), -dcgrid::inf(), -dcgrid::inf()};
    int m = 0;
    for (long long i = tid; i < n; i += BOX_THREADS) {
        const float* p = pos + 3 * (c.base + i);
        const float x = p[0], y = p[1], z = p[2];
        if (dcgrid::finite3(x, y, z)) {
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
            ++m;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
        m += __shfl_xor(m, o, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            red[a][tid >> 6] = lo[a];
            red[3 + a][tid >> 6] = hi[a];
        }
        redc[tid >> 6] = m;
    }
    __syncthreads();
    if (tid == 0) {
        m = 0;
        for (int w = 0; w < BOX_THREADS / 64; ++w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], red[a][w]);
                hi[a] = fmaxf(hi[a], red[3 + a][w]);
            }
            m += redc[w];
        }
        Grid G;
        dcgrid::make_grid(m, lo, hi, target, G);
        grids[b] = G;
    }
}

// COUNT: add one to the cell's counter; otherwise take a slot of the cell and write the point there
template <class PtrT, bool COUNT>
__global__ __launch_bounds__(G_THREADS) void grid_bin_kernel(const float* __restrict__ pos, const PtrT* __restrict__ ptr, int B,
                                                             long long cap, const Grid* __restrict__ grids, u64* __restrict__ cnt,
                                                             Pt* __restrict__ pts) {
    const long long t = (long long)blockIdx.x * G_THREADS + threadIdx.x;
    if (t >= cap) return;
    const long long row = (long long)ptr[0] + t;
    const int b = cloud_index(ptr, B, row);
    if (b < 0) return;
    const Cloud c = cloud_of(ptr, b, cap);
    if (!c.ok) return;
    const float* p = pos + 3 * row;
    const float x = p[0], y = p[1], z = p[2];
    if (!dcgrid::finite3(x, y, z)) return;
    const Grid& G = grids[b];
    const int cell = dcgrid::cell_of(G, dcgrid::cell_axis(x, G.lo[0], G.inv_h[0], G.g[0]),
                                     dcgrid::cell_axis(y, G.lo[1], G.inv_h[1], G.g[1]),
                                     dcgrid::cell_axis(z, G.lo[2], G.inv_h[2], G.g[2]));
    u64* counter = cnt + 2 * c.off + b + cell;           // cell < max(1, 2 n): inside the cloud's 2 n + 1 counters
    if (COUNT) {
        atomicAdd(counter, 1ull);
    } else {
        const u64 at = atomicAdd(counter, 1ull);
        if (at < (u64)cap) pts[at] = Pt{x, y, z, (int)(row - c.base)};
    }
}

template <int K>
__global__ __launch_bounds__(G_THREADS) void grid_self_kernel(const float* __restrict__ pos, const int* __restrict__ cloud_ptr,
                                                              long long cap, const Grid* __restrict__ grids,
                                                              const int64_t* __restrict__ lptr, const Pt* __restrict__ pts, int k,
                                                              int* __restrict__ nbr) {
    const int b = blockIdx.y;
    const Cloud c = cloud_of(cloud_ptr, b, cap);
    if (!c.ok) return;                        // block-uniform
    const long long i = (long long)blockIdx.x * G_THREADS + threadIdx.x;
    if (i >= c.n) return;
    // a point with a non-finite coordinate is in no cell and owns no search: its row names itself (ids stay inside the cloud)
    const float* p = pos + 3 * (c.base + i);
    if (!dcgrid::finite3(p[0], p[1], p[2])) {
        int* out = nbr + (c.base + i) * k;
        for (int s = 0; s < k; ++s) out[s] = (int)(c.base + i);
    }
    const Grid G = grids[b];
    if (i >= G.m) return;
    const int64_t* cstart = lptr + 2 * c.off + b;
    const long long at = cstart[0] + i;       // the i-th of the cloud's points in cell order
    if (at < 0 || at >= cap) return;
    const Pt q = pts[at];
    if (q.id < 0 || q.id >= c.n) return;
    dcgrid::TopKLex<K> best;
    best.init();
    dcgrid::search<K>(G, pts, cstart, cap, q.x, q.y, q.z, k, best);
    int* out = nbr + (c.base + q.id) * k;
#pragma unroll
    for (int s = 0; s < K; ++s)               // a slot nothing could fill (fewer than k finite points, overflowed distances): the query
        if (s < k) out[s] = (int)c.base + (best.id[s] == 0x7fffffff ? q.id : best.id[s]);
}

template <int K>
__global__ __launch_bounds__(G_THREADS) void grid_cross_kernel(const float* __restrict__ query, const int64_t* __restrict__ qptr,
                                                               const int64_t* __restrict__ rptr, long long cap,
                                                               const Grid* __restrict__ grids, const int64_t* __restrict__ lptr,
                                                               const Pt* __restrict__ pts, int k, int32_t* __restrict__ idx,
                                                               float* __restrict__ d2) {
    const int b = blockIdx.y;
    const long long qbase = qptr[b], nq = qptr[b + 1] - qbase;
    const long long q = (long long)blockIdx.x * G_THREADS + threadIdx.x;
    if (q >= nq) return;
    const Cloud c = cloud_of(rptr, b, cap);
    const float* p = query + 3 * (qbase + q);
    const float px = p[0], py = p[1], pz = p[2];
    dcgrid::TopKLex<K> best;
    best.init();
    if (c.ok && dcgrid::finite3(px, py, pz)) {
        const Grid G = grids[b];
        dcgrid::search<K>(G, pts, lptr + 2 * c.off + b, cap, px, py, pz, k, best);
    }
    int32_t* oi = idx + (qbase + q) * k;
    float* od = d2 + (qbase + q) * k;
#pragma unroll
    for (int s = 0; s < K; ++s)
        if (s < k) {
            oi[s] = best.id[s] == 0x7fffffff ? -1 : best.id[s];
            od[s] = best.d[s];
        }
}

struct Work {
    Grid* grids;
    u64 *cnt, *part;
    int64_t* lptr;
    Pt* pts;
    long long cap, rows;
};
Work carve(void* workspace, long long cap, long long B) {
    const Layout L = layout(cap, B);
    char* w = static_cast<char*>(workspace);
    return Work{reinterpret_cast<Grid*>(w + L.grids), reinterpret_cast<u64*>(w + L.cnt), reinterpret_cast<u64*>(w + L.part),
                reinterpret_cast<int64_t*>(w + L.lptr), reinterpret_cast<Pt*>(w + L.pts), cap, L.rows};
}

// box, zero, count, scan, fill: the grid of every reference cloud of the call and its points in cell order
template <class PtrT>
int build(const char* name, const float* ref, const PtrT* ptr, int B, float target, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL((grid_box_kernel<PtrT>), dim3(B), dim3(BOX_THREADS), 0, s, ref, ptr, w.cap, target, w.grids);
    DC_CHECK_LAUNCH(name);
    dc_zero_words(w.cnt, 2 * w.rows, s);
    DC_CHECK_LAUNCH(name);
    const int bins = dc_cdiv(w.cap, G_THREADS), scans = dc_cdiv(w.rows, SC_THREADS);
    if (bins > 0) {
        hipLaunchKernelGGL((grid_bin_kernel<PtrT, true>), dim3(bins), dim3(G_THREADS), 0, s, ref, ptr, B, w.cap, w.grids, w.cnt, w.pts);
        DC_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(list_sum_kernel, dim3(scans), dim3(SC_THREADS), 0, s, w.cnt, w.rows, w.part);
    DC_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(list_scan_kernel, dim3(scans), dim3(SC_THREADS), 0, s, w.cnt, w.rows, w.part, w.lptr);
    DC_CHECK_LAUNCH(name);
    if (bins > 0) {
        hipLaunchKernelGGL((grid_bin_kernel<PtrT, false>), dim3(bins), dim3(G_THREADS), 0, s, ref, ptr, B, w.cap, w.grids, w.cnt, w.pts);
        DC_CHECK_LAUNCH(name);
    }
    return DC_OK;
}

template <int K>
int launch_self(const float* pos, const int* cloud_ptr, int B, int max_cloud, int k, int* nbr, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL((grid_self_kernel<K>), dim3(dc_cdiv(max_cloud, G_THREADS), B), dim3(G_THREADS), 0, s, pos, cloud_ptr, w.cap,
                       w.grids, w.lptr, w.pts, k, nbr);
    DC_CHECK_LAUNCH("dc_knn_grid");
    return DC_OK;
}

template <int K>
int launch_cross(const float* query, const int64_t* qptr, const int64_t* rptr, int B, long long max_q, int k, int32_t* idx, float* d2,
                 const Work& w, hipStream_t s) {
    hipLaunchKernelGGL((grid_cross_kernel<K>), dim3(dc_cdiv(max_q, G_THREADS), B), dim3(G_THREADS), 0, s, query, qptr, rptr, w.cap,
                       w.grids, w.lptr, w.pts, k, idx, d2);
    DC_CHECK_LAUNCH("dc_knn_cross_grid");
    return DC_OK;
}

bool good_target(float t) { return t > 0.f && dcgrid::finite1(t); }

}  // namespace

// the build for fps_grid.hip (knn_grid_build.h): the same layout, the same five launches
size_t dc_grid_build_bytes(long long num_points, long long num_clouds) { return layout(num_points, num_clouds).total; }
long long dc_grid_build_capacity(size_t bytes, long long num_clouds) { return capacity(bytes, num_clouds); }
int dc_grid_build(const char* name, const float* pos, const int64_t* ptr, int B, float target, void* workspace, long long cap,
                  hipStream_t stream, DcGridBuild* out) {
    const Work w = carve(workspace, cap, B);
    *out = DcGridBuild{w.grids, w.lptr, w.pts, w.cap, w.rows};
    return build(name, pos, ptr, B, target, w, stream);
}

DC_EXPORT size_t dc_knn_grid_workspace_bytes(int64_t num_points, int32_t num_clouds) {
    if (num_points < 0 || num_points > G_MAX_POINTS || num_clouds < 0) return 0;
    return layout(num_points, num_clouds).total;
}

DC_EXPORT int dc_knn_grid(const float* pos, const int32_t* cloud_ptr, int32_t num_clouds, int32_t max_cloud_size, int32_t k,
                          float target, int32_t* nbr, void* workspace, size_t workspace_bytes, void* stream) {
    DC_REQUIRE(pos && cloud_ptr && nbr, "dc_knn_grid: null pointer (pos, cloud_ptr, nbr)");
    DC_REQUIRE(k >= 1 && k <= 64, "dc_knn_grid: k=%d outside [1,64]", k);
    DC_REQUIRE(num_clouds >= 0 && num_clouds <= 65535 && max_cloud_size >= 0, "dc_knn_grid: num_clouds = %d outside [0, 65535] or a negative size",
               num_clouds);
    DC_REQUIRE(good_target(target), "dc_knn_grid: target = %g must be positive and finite", (double)target);
    if (num_clouds == 0 || max_cloud_size == 0) return DC_OK;
    DC_REQUIRE(workspace, "dc_knn_grid: null workspace");
    DC_REQUIRE(aligned_to(workspace, 16), "dc_knn_grid: workspace must be 16-byte aligned");
    long long cap = capacity(workspace_bytes, num_clouds);
    DC_REQUIRE(cap >= max_cloud_size, "dc_knn_grid: workspace of %zu bytes is too small (dc_knn_grid_workspace_bytes of all points of the call)",
               workspace_bytes);
    const long long most = (long long)num_clouds * max_cloud_size;       // no call holds more points than this
    cap = cap < most ? cap : most;
    const Work w = carve(workspace, cap, num_clouds);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = build("dc_knn_grid", pos, cloud_ptr, num_clouds, target, w, s);
    if (rc != DC_OK) return rc;
    if (k <= 10) return launch_self<10>(pos, cloud_ptr, num_clouds, max_cloud_size, k, nbr, w, s);
    if (k <= 16) return launch_self<16>(pos, cloud_ptr, num_clouds, max_cloud_size, k, nbr, w, s);
    if (k <= 20) return launch_self<20>(pos, cloud_ptr, num_clouds, max_cloud_size, k, nbr, w, s);
    if (k <= 30) return launch_self<30>(pos, cloud_ptr, num_clouds, max_cloud_size, k, nbr, w, s);
    if (k <= 40) return launch_self<40>(pos, cloud_ptr, num_clouds, max_cloud_size, k, nbr, w, s);
    return launch_self<64>(pos, cloud_ptr, num_clouds, max_cloud_size, k, nbr, w, s);
}

DC_EXPORT int dc_knn_cross_grid(const float* query, const int64_t* qptr, const float* ref, const int64_t* rptr, int32_t B,
                                int64_t max_query_cloud, int32_t k, float target, int32_t* idx, float* d2, void* workspace,
                                size_t workspace_bytes, void* stream) {
    DC_REQUIRE(B >= 0 && B <= 65535, "dc_knn_cross_grid: B = %d cloud pairs, supported: 0 .. 65535 per launch", B);
    DC_REQUIRE(k >= 1 && k <= 16, "dc_knn_cross_grid: k = %d outside [1, 16]", k);
    DC_REQUIRE(max_query_cloud >= 0 && max_query_cloud <= (1ll << 31) * G_THREADS - G_THREADS,
               "dc_knn_cross_grid: max_query_cloud = %lld outside [0, 2^39)", (long long)max_query_cloud);
    DC_REQUIRE(good_target(target), "dc_knn_cross_grid: target = %g must be positive and finite", (double)target);
    if (B == 0 || max_query_cloud == 0) return DC_OK;
    DC_REQUIRE(query && qptr && ref && rptr && idx && d2, "dc_knn_cross_grid: null pointer (query, qptr, ref, rptr, idx, d2)");
    DC_REQUIRE(workspace, "dc_knn_cross_grid: null workspace");
    DC_REQUIRE(aligned_to(workspace, 16), "dc_knn_cross_grid: workspace must be 16-byte aligned");
    const long long cap = capacity(workspace_bytes, B);
    DC_REQUIRE(cap >= 0, "dc_knn_cross_grid: workspace of %zu bytes is too small (dc_knn_grid_workspace_bytes of the reference rows of the call)",
               workspace_bytes);
    const Work w = carve(workspace, cap, B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = build("dc_knn_cross_grid", ref, rptr, B, target, w, s);
    if (rc != DC_OK) return rc;
    if (k == 1) return launch_cross<1>(query, qptr, rptr, B, max_query_cloud, k, idx, d2, w, s);
    if (k <= 4) return launch_cross<4>(query, qptr, rptr, B, max_query_cloud, k, idx, d2, w, s);
    if (k <= 8) return launch_cross<8>(query, qptr, rptr, B, max_query_cloud, k, idx, d2, w, s);
    return launch_cross<16>(query, qptr, rptr, B, max_query_cloud, k, idx, d2, w, s);
}
