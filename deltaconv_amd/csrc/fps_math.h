// Arithmetic of the device geodesic farthest-point sampler (fps.hip), shared with the g++ host-check build (tests/hostcheck_fps)
// like eval_math.h / batch_math.h.  No HIP types, no LDS, no wave intrinsics.
//
// Reference being restated: deltaconv/cpp/sampling.cpp:5-81 through the host library's restatement
// (csrc_host/fps.cpp) -- every rule below is the one that file follows, so the device picks the host's points:
//   distance   fp64, dx = p[j] - p[i] per axis, ((dx*dx + dy*dy) + dz*dz) without contraction; an edge is sqrt of it
//   graph      the k = 10 candidates smallest in (d2, j), the point itself left out by index (duplicates stay, at distance 0)
//   relax      nd = D[u] + w(u, v), taken where nd < D[v]
//   sample     the FIRST index of max(D)
#pragma once
#include "point_math.h"

namespace dcfps {

constexpr int K = 10;                         // neighbours per point (sampling.cpp:9)
constexpr int MAX_POINTS = 16384;             // points per cloud the sampling kernel holds in LDS (DC_FPS_MAX_POINTS)

DC_HD double inf() { return __builtin_huge_val(); }

// squared length of p[j] - p[i]
DC_HD double dist2(double ix, double iy, double iz, double jx, double jy, double jz) {
    const double dx = jx - ix, dy = jy - iy, dz = jz - iz;
    return (dx * dx + dy * dy) + dz * dz;
}

// The K smallest (d2, j) seen so far, ascending; start from topk_clear and feed the candidates by ASCENDING j.  Strict `<` twice:
// a candidate equal to the last kept one does not displace it, and one equal to an earlier one stops behind it -- the lower index
// stays in front, which is the std::pair order the host sorts by.
DC_HD void topk_clear(double (&d)[K], int (&id)[K]) {
#pragma unroll
    for (int s = 0; s < K; ++s) { d[s] = inf(); id[s] = -1; }
}
DC_HD void topk_insert(double (&d)[K], int (&id)[K], double d2, int j) {
    if (!(d2 < d[K - 1])) return;
    d[K - 1] = d2;
    id[K - 1] = j;
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
        const bool up = d[s] < d[s - 1];
        const double dl = up ? d[s] : d[s - 1], dh = up ? d[s - 1] : d[s];
        const int il = up ? id[s] : id[s - 1], ih = up ? id[s - 1] : id[s];
        d[s - 1] = dl; d[s] = dh;
        id[s - 1] = il; id[s] = ih;
    }
}

// One edge u -> v of length w, from the distance du of u: the candidate distance of v.  It is taken where it is BELOW D[v]; the
// device takes it with an unsigned 64-bit minimum on the bit patterns, which order like the values for non-negative doubles.
DC_HD double relax(double du, double w) { return du + w; }

// (value, index) combine of "first index of the maximum": a is kept unless b is larger, or equal with a lower index.
DC_HD void argmax_combine(double& av, int& ai, double bv, int bi) {
    if (bv > av || (bv == av && bi < ai)) {
        av = bv;
        ai = bi;
    }
}

// bytes of workspace dc_geodesic_fps_batch needs for N points in all: edge lengths [N,K] fp64, neighbours [N,K] int32, and the
// uploaded offsets and start points of at most N clouds (no cloud is empty), each block 256-byte aligned
DC_HD unsigned long long workspace_bytes(long long N) {
    if (N < 0) N = 0;
    const unsigned long long n = (unsigned long long)N;
    return n * K * 8 + n * K * 4 + (n + 1) * 8 + n * 4 + 4 * 256;
}

// ---- the sampler for clouds above MAX_POINTS (fps_sample_global_kernel): D in global memory, the frontier bit sets in LDS ----
constexpr int LARGE_MAX_POINTS = 262144;      // 2 bit sets of n / 8 bytes = 64 KiB of LDS at the cap (DC_FPS_LARGE_MAX_POINTS)

// 32-bit words of one frontier bit set of a cloud of n points; vertex u is bit (u & 31) of word (u >> 5)
DC_HD int bitset_words(int n) { return (n + 31) >> 5; }

// bytes of dynamic LDS of the kernel for a launch whose largest cloud has n points: the two bit sets
DC_HD unsigned long long large_lds_bytes(int n) { return 2ull * (unsigned long long)bitset_words(n) * 4; }

// bytes of workspace dc_geodesic_fps_large needs for N points in all: the blocks above, then D [N] 64-bit patterns, 256-byte aligned
DC_HD unsigned long long large_workspace_bytes(long long N) {
    if (N < 0) N = 0;
    return workspace_bytes(N) + (unsigned long long)N * 8 + 256;
}

}  // namespace dcfps
