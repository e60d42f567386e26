// Voxel-grid subsampling of device-resident clouds: dc_voxel_subsample.  One representative per occupied cell of edge `size`, the
// representatives in row order, and for every point the output row of its cell -- torch_cluster.grid_cluster /
// torch_geometric.nn.voxel_grid followed by consecutive_cluster.  The rules (finite, origin, cell, range, key, order) are
// csrc/voxel_math.h, shared with the g++ host check (tests/hostcheck_voxel).
//
// Seven launches (six when the caller gives the origins), stream-ordered, every launch size from the HOST sizes (N rows, B clouds):
//   vox_fill_kernel     the hash table to all ones (no cell, no representative), the status words
//   vox_box_kernel      one workgroup per cloud: the fp32 minimum over its finite points -> the cloud's origin (order-free)
//   vox_insert_kernel   one thread per row: its cloud by bisection of the offsets, dcvox::bid; the packed cell goes into the cloud's
//                       OWN slice of an open-addressing table (2 n_b + 1 slots of {cell, minimum}, at slot 2 (ptr[b] - ptr[0]) + b:
//                       host-known offsets, as knn_grid.hip lays out its counters) by a 64-bit atomicCAS on the cell word with
//                       linear probing, then a 64-bit atomicMin of the key on the slot's second word; the slot is recorded in
//                       `cluster`, so no later pass probes again.  The probe loop is bounded by the slice length and never waits
//                       on another thread; a cloud holds at most n_b distinct cells, so it cannot run out (if it does: status word)
//   vox_emit_kernel<true>   row i is a representative iff the low word of its slot's minimum is i -> one flag per row
//   list_sum / list_scan (list_scan.h)  exclusive scan of the flags over ALL rows: every representative's output row
//   vox_emit_kernel<false>  rows compacted, cluster[i] = the scan at i's representative, optr read off the scan at the cloud
//                       boundaries, the total next to the status words
// Phases that read what another phase wrote are separate launches: no kernel waits on another workgroup.
// Integer atomics only, on cells and keys: a minimum does not depend on the order of its operands, and WHICH slot a cell lands in
// (the only thing the race decides) is read by nobody but the points of that cell.  So table collisions cannot reach the result.
#include "common.h"
#include "list_scan.h"
#include "voxel_math.h"

namespace {

constexpr int V_THREADS = 256;
constexpr int VBOX_THREADS = 1024;
constexpr long long V_MAX_POINTS = 0x7fffffffll;     // local ids are 32 bits of the key
constexpr int V_MAX_CLOUDS = 1 << 24;

struct Slot {
    u64 cell, best;
};
static_assert(sizeof(Slot) == 16, "workspace layout");

struct Layout {
    size_t table, origin, lptr, part, total;
    long long slots;
};
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
Layout layout(long long n, long long B) {
    Layout L;
    L.slots = 2 * n + B;
    L.table = 0;
    L.origin = (size_t)L.slots * sizeof(Slot);
    L.lptr = up16(L.origin + (size_t)B * 12);
    L.part = L.lptr + (size_t)(n + 1) * 8;
    L.total = up16(L.part + (size_t)((n + SC_THREADS - 1) / SC_THREADS) * 8);
    return L;
}

struct Cloud {
    long long base, n, off;
    bool ok;
};
// cloud b of the call; ok: it lies inside the N rows of pos (and so inside the table)
__device__ __forceinline__ Cloud cloud_of(const int64_t* __restrict__ ptr, int b, long long N) {
    Cloud c;
    c.base = ptr[b];
    c.n = ptr[b + 1] - c.base;
    c.off = c.base - ptr[0];
    c.ok = c.n >= 0 && c.off >= 0 && c.base >= 0 && c.base + c.n <= N && c.n <= V_MAX_POINTS;
    return c;
}
// the cloud of row `row`: the last b with ptr[b] <= row (empty clouds are passed over), -1 outside every cloud
__device__ __forceinline__ int cloud_index(const int64_t* __restrict__ ptr, int B, long long row) {
    int lo = 0, hi = B;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= row) lo = mid + 1;
        else hi = mid;
    }
    const int b = lo - 1;
    return (b >= 0 && b < B && row < ptr[b + 1]) ? b : -1;
}

// info: [0] rows in all (written by the emit pass) | [1] first overflowing cloud, all ones = none | [2] table status, 0 = fine
__global__ __launch_bounds__(V_THREADS) void vox_fill_kernel(u64* __restrict__ table, long long words, u64* __restrict__ info) {
    const long long i = (long long)blockIdx.x * V_THREADS + threadIdx.x;
    if (i < words) table[i] = (u64)dcvox::EMPTY;
    if (i == 0) {
        info[0] = 0ull;
        info[1] = (u64)dcvox::EMPTY;
        info[2] = 0ull;
        info[3] = 0ull;
    }
}

__global__ __launch_bounds__(VBOX_THREADS) void vox_box_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr,
                                                               long long N, float* __restrict__ origin) {
    __shared__ float red[3][VBOX_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Cloud c = cloud_of(ptr, b, N);
    const long long n = c.ok ? c.n : 0;
    float lo[3] = {dcgrid::inf(), dcgrid::inf(), dcgrid::inf()};
    for (long long i = tid; i < n; i += VBOX_THREADS) {
        const float* p = pos + 3 * (c.base + i);
        const float x = p[0], y = p[1], z = p[2];
        if (dcgrid::finite3(x, y, z)) {
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) red[a][tid >> 6] = lo[a];
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < VBOX_THREADS / 64; ++w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], red[a][w]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) origin[3 * b + a] = lo[a] < dcgrid::inf() ? lo[a] : 0.f;      // no finite point: no cell either
    }
}

__device__ __forceinline__ u64 mix64(u64 v) {            // where a cell starts probing; any function gives the same result
    v ^= v >> 30; v *= 0xbf58476d1ce4e5b9ull;
    v ^= v >> 27; v *= 0x94d049bb133111ebull;
    return v ^ (v >> 31);
}

__global__ __launch_bounds__(V_THREADS) void vox_insert_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr, int B,
                                                               long long N, const float* __restrict__ origin, float sx, float sy,
                                                               float sz, int pick, Slot* __restrict__ table, long long slots,
                                                               int64_t* __restrict__ cluster, u64* __restrict__ info) {
    const long long row = (long long)blockIdx.x * V_THREADS + threadIdx.x;
    if (row >= N) return;
    long long mine = -1;                                 // the row's slot; -1: it belongs to no cell
    const int b = cloud_index(ptr, B, row);
    if (b >= 0) {
        const Cloud c = cloud_of(ptr, b, N);
        const long long first = 2 * c.off + b, len = 2 * c.n + 1;
        if (c.ok && first >= 0 && first + len <= slots) {
            const float* p = pos + 3 * row;
            const float o[3] = {origin[3 * b], origin[3 * b + 1], origin[3 * b + 2]};
            const float s[3] = {sx, sy, sz};
            const dcvox::Bid bid = dcvox::bid(p[0], p[1], p[2], o, s, pick, (uint32_t)(row - c.base));
            if (bid.overflow) atomicMin(info + 1, (u64)b);
            if (bid.finite && !bid.overflow) {
                long long at = (long long)__umul64hi(mix64(bid.cell), (u64)len);       // in [0, len)
                for (long long probe = 0; probe < len; ++probe) {
                    Slot* slot = table + first + at;
                    const u64 seen = atomicCAS(&slot->cell, (u64)dcvox::EMPTY, (u64)bid.cell);
                    if (seen == (u64)dcvox::EMPTY || seen == (u64)bid.cell) {
                        atomicMin(&slot->best, (u64)bid.key);
                        mine = first + at;
                        break;
                    }
                    at = at + 1 == len ? 0 : at + 1;
                }
                if (mine < 0) atomicMax(info + 2, 1ull);
            }
        }
    }
    cluster[row] = mine;
}

// FLAG: one flag per row for the scan; otherwise the outputs
template <bool FLAG>
__global__ __launch_bounds__(V_THREADS) void vox_emit_kernel(const int64_t* __restrict__ ptr, int B, long long N,
                                                             const Slot* __restrict__ table, long long slots,
                                                             const int64_t* __restrict__ lptr, u64* __restrict__ flag,
                                                             int64_t* __restrict__ rows, int64_t* __restrict__ optr,
                                                             int64_t* __restrict__ cluster, u64* __restrict__ info) {
    const long long row = (long long)blockIdx.x * V_THREADS + threadIdx.x;
    if (!FLAG) {
        if (row <= B) {
            const long long at = ptr[row];
            optr[row] = lptr[at < 0 ? 0 : (at > N ? N : at)];
        }
        if (row == 0) info[0] = (u64)lptr[N];
    }
    if (row >= N) return;
    const long long mine = cluster[row];
    long long rep = -1;                                  // the row of this row's representative
    if (mine >= 0 && mine < slots) {
        const int b = cloud_index(ptr, B, row);          // a row with a slot lies in a cloud that is ok
        const long long base = b >= 0 ? ptr[b] : 0;
        const long long r = base + (long long)(table[mine].best & 0xffffffffull);
        rep = (b >= 0 && r >= 0 && r < N) ? r : -1;
    }
    if (FLAG) {
        flag[row] = rep == row ? 1ull : 0ull;
    } else {
        const long long out = rep >= 0 ? lptr[rep] : -1;
        if (rep == row && out >= 0 && out < N) rows[out] = row;
        cluster[row] = out;
    }
}

}  // namespace

DC_EXPORT size_t dc_voxel_subsample_workspace_bytes(int64_t num_points, int32_t num_clouds) {
    if (num_points < 0 || num_points > V_MAX_POINTS || num_clouds < 0 || num_clouds > V_MAX_CLOUDS) return 0;
    return layout(num_points, num_clouds).total;
}

DC_EXPORT int dc_voxel_subsample(const float* pos, const int64_t* ptr, int32_t B, int64_t num_points, float size_x, float size_y,
                                 float size_z, const float* origin, int32_t pick, int64_t* rows, int64_t* optr, int64_t* cluster,
                                 int64_t* info, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "dc_voxel_subsample";
    DC_REQUIRE(B >= 0 && B <= V_MAX_CLOUDS, "%s: B = %d clouds, supported: 0 .. %d", fn, B, V_MAX_CLOUDS);
    DC_REQUIRE(num_points >= 0 && num_points <= V_MAX_POINTS, "%s: num_points = %lld outside [0, 2^31)", fn, (long long)num_points);
    DC_REQUIRE(dcgrid::finite1(size_x) && dcgrid::finite1(size_y) && dcgrid::finite1(size_z) && size_x > 0.f && size_y > 0.f &&
                   size_z > 0.f, "%s: size = (%g, %g, %g) must be positive and finite", fn, (double)size_x, (double)size_y, (double)size_z);
    DC_REQUIRE(pick == dcvox::PICK_CENTRE || pick == dcvox::PICK_FIRST, "%s: pick = %d (0: centre, 1: first)", fn, pick);
    DC_REQUIRE(ptr && optr && info, "%s: null pointer (ptr, optr, info)", fn);
    DC_REQUIRE(num_points == 0 || (pos && rows && cluster), "%s: null pointer (pos, rows, cluster)", fn);
    DC_REQUIRE(workspace, "%s: null workspace", fn);
    DC_REQUIRE(aligned_to(workspace, 16), "%s: workspace must be 16-byte aligned", fn);
    const long long N = num_points;
    const Layout L = layout(N, B);
    DC_REQUIRE(workspace_bytes >= L.total, "%s: workspace of %zu bytes is too small (dc_voxel_subsample_workspace_bytes: %zu)", fn,
               workspace_bytes, L.total);
    char* w = static_cast<char*>(workspace);
    Slot* table = reinterpret_cast<Slot*>(w + L.table);
    float* own = reinterpret_cast<float*>(w + L.origin);
    int64_t* lptr = reinterpret_cast<int64_t*>(w + L.lptr);
    u64* part = reinterpret_cast<u64*>(w + L.part);
    u64* flag = reinterpret_cast<u64*>(rows);            // `rows` [N] holds the scan's flags until the emit pass, which reads the scan only
    u64* status = reinterpret_cast<u64*>(info);
    hipStream_t s = static_cast<hipStream_t>(stream);

    const long long words = 2 * L.slots;
    hipLaunchKernelGGL(vox_fill_kernel, dim3(dc_cdiv(words > 0 ? words : 1, V_THREADS)), dim3(V_THREADS), 0, s,
                       reinterpret_cast<u64*>(table), words, status);
    DC_CHECK_LAUNCH(fn);
    if (!origin && B > 0) {
        hipLaunchKernelGGL(vox_box_kernel, dim3(B), dim3(VBOX_THREADS), 0, s, pos, ptr, N, own);
        DC_CHECK_LAUNCH(fn);
    }
    const int blocks = dc_cdiv(N, V_THREADS);
    if (blocks > 0) {
        hipLaunchKernelGGL(vox_insert_kernel, dim3(blocks), dim3(V_THREADS), 0, s, pos, ptr, B, N, origin ? origin : own, size_x,
                           size_y, size_z, pick, table, L.slots, cluster, status);
        DC_CHECK_LAUNCH(fn);
        hipLaunchKernelGGL((vox_emit_kernel<true>), dim3(blocks), dim3(V_THREADS), 0, s, ptr, B, N, table, L.slots, lptr, flag, rows,
                           optr, cluster, status);
        DC_CHECK_LAUNCH(fn);
        const int scans = dc_cdiv(N, SC_THREADS);
        hipLaunchKernelGGL(list_sum_kernel, dim3(scans), dim3(SC_THREADS), 0, s, flag, N, part);
        DC_CHECK_LAUNCH(fn);
        hipLaunchKernelGGL(list_scan_kernel, dim3(scans), dim3(SC_THREADS), 0, s, flag, N, part, lptr);
        DC_CHECK_LAUNCH(fn);
    } else {
        dc_zero_words(lptr, 2, s);                       // no rows: the scan is its one entry, 0
        DC_CHECK_LAUNCH(fn);
    }
    const long long most = N > (long long)B + 1 ? N : (long long)B + 1;
    hipLaunchKernelGGL((vox_emit_kernel<false>), dim3(dc_cdiv(most, V_THREADS)), dim3(V_THREADS), 0, s, ptr, B, N, table, L.slots, lptr,
                       flag, rows, optr, cluster, status);
    DC_CHECK_LAUNCH(fn);
    return DC_OK;
}
