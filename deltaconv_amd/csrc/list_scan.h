// Exclusive scan of per-row counters over ALL rows of a call: the middle of every "count, scan, fill, rank" list build (the in-edge
// lists of interp.hip, the vertex-to-corner lists of mesh_normal.hip).  Two launches on the grid of ceil(num_rows / SC_THREADS)
// workgroups: list_sum_kernel writes one sum per 1024 rows, list_scan_kernel adds the sums of the blocks before its own and scans
// its rows.  Integer arithmetic: any scan shape gives the same values.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int SC_THREADS = 1024;              // rows of a scan block

__device__ __forceinline__ u64 block_sum(u64 v, u64* red) {          // red [SC_THREADS / 64]; every thread gets the sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < SC_THREADS / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(SC_THREADS) void list_sum_kernel(const u64* __restrict__ cnt, long long num_rows,
                                                              u64* __restrict__ part) {
    __shared__ u64 red[SC_THREADS / 64];
    const long long r = (long long)blockIdx.x * SC_THREADS + threadIdx.x;
    const u64 s = block_sum(r < num_rows ? cnt[r] : 0ull, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// exclusive scan of cnt: lptr [num_rows + 1] and the fill cursors (the cursors replace cnt)
__global__ __launch_bounds__(SC_THREADS) void list_scan_kernel(u64* __restrict__ cnt, long long num_rows,
                                                               const u64* __restrict__ part, int64_t* __restrict__ lptr) {
    __shared__ u64 red[SC_THREADS / 64];
    __shared__ u64 sc[SC_THREADS];
    const int tid = threadIdx.x;
    u64 before = 0;
    for (int i = tid; i < (int)blockIdx.x; i += SC_THREADS) before += part[i];
    const u64 base = block_sum(before, red);
    const long long r = (long long)blockIdx.x * SC_THREADS + tid;
    const u64 c = r < num_rows ? cnt[r] : 0ull;
    sc[tid] = c;
    __syncthreads();
    for (int off = 1; off < SC_THREADS; off <<= 1) {      // inclusive Hillis-Steele scan
        const u64 v = tid >= off ? sc[tid - off] : 0ull;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    if (r < num_rows) {
        const u64 excl = base + sc[tid] - c;
        lptr[r] = (int64_t)excl;
        cnt[r] = excl;
        if (r == num_rows - 1) lptr[num_rows] = (int64_t)(excl + c);
    }
}

}  // namespace
