// Weight gradient dW[M,N] = A[R,M]^T B[R,N] (both operands reduction-major, R = points) with the bf16 split done ONCE per element,
// where the tile is stored to LDS.  Same contract and numerics class as the A_KM / B_KN instantiations of gemm_kernel (gemm.hip):
// row slabs over grid.y, per-slab partial tiles summed in slab order by gemm_tn.hip; three bf16 planes per operand, the six
// partial products of weight >= 2^-16, fp32 accumulation, v_mfma_f32_32x32x16_bf16; 4 waves (2 x 2), 32 x 32 accumulators.
//
// gemm_kernel stages such operands as fp32 [32][BM]: every MFMA fragment costs eight ds_read_b32, and every element is cut into
// planes in registers by each of the two waves that read it.  Here:
//   * Register-transposed staging.  For the 32x32x16 MFMA, lane (r = l & 31, h = l >> 5) supplies 8 consecutive reduction indices
//     k = 8h .. 8h+7 of output row / column r: 16 bytes of bf16.  In memory these sit in 8 different rows, so a staging thread
//     loads an 8-row x 4-column block -- eight 16-byte loads at the same 4 columns of rows 8q .. 8q+7 (the lanes of one load still
//     cover whole 128-byte row segments) -- and then holds, for each of its 4 columns, one MFMA operand's worth of k.  A 32 x BM
//     tile takes BM threads: thread t < BM stages A, BM <= t < BM + BN stages B.
//   * Split at the store: the thread cuts its 32 values (16 split_pair: pairs = consecutive k of one column) and writes one
//     ds_write_b128 per column and plane, 12 stores.  LDS holds K-contiguous plane images [plane][column][32 k] (64-byte rows, the
//     BM columns of A followed by the BN columns of B).
//   * Fragments are ONE ds_read_b128 per (fragment, plane, 16-deep k-step).
// Image layout (checked lane by lane by tools/tn_planes_layout_sim.py against the LDS bank rules): column c of an operand lives in
// row c ^ ((c >> 4) & 1) and its k-octet s (0..3) in 16-byte slot s ^ ((c >> 2) & 3).  The slot swizzle spreads the 16 lanes of a
// ds_read_b128 group over the 16 slots of a 256-byte bank row; the row swap puts the 8 lanes of a ds_write_b128 group (8 consecutive
// column quads, same octet) on the 8 slots of a 128-byte window.  Both conflict-free.
// K loop (one plane buffer, one staging register set, two barriers per 32-deep tile): the global loads of tile t+1 are issued
// right after tile t's planes are stored; they land while tile t is multiplied; the split of tile t+1 runs between the MFMAs of
// tile t's second k-step (DC_TNP_SHADOW) so that only the 12 LDS stores sit between the two barriers.
// BatchNorm-backward prologue (PRO): A = dh = c_g dz + c_a h + c_b is formed from dy, h and the thread's 20 coefficients (its 4
// columns never change: loaded once) before the split.
#include <algorithm>
#include <type_traits>
#include "common.h"
#include "gemm_split.h"
#include "gemm_tn_planes.h"

namespace {

using namespace dcsplit;

#ifndef DC_TNP_SHADOW
#define DC_TNP_SHADOW 1        // 1: split of the next tile between the MFMAs of the second k-step; 0: after them
#endif
constexpr int BK = 32;         // reduction tile
constexpr int NT = 256;        // threads per workgroup (4 waves, 2 x 2)
constexpr int ROWB = 64;       // bytes of an image row: 32 k of one column and plane

template <int BM, int BN, int PRO>
__global__ __launch_bounds__(NT, 2) void gemm_tn_planes_kernel(DcTnPlanesP p) {
    constexpr int WM = BM / 2, WN = BN / 2;        // wave tile
    constexpr int TM = WM / 32, TN = WN / 32;      // 32 x 32 accumulators per wave
    constexpr int PL = (BM + BN) * ROWB;           // bytes of one plane image (A columns, then B columns)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* img = reinterpret_cast<char*>(smem);     // [3][BM + BN][ROWB]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int tiles_n = p.N / BN;
    const int tm = (int)blockIdx.x / tiles_n, tn = (int)blockIdx.x - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const long kbeg = (long)blockIdx.y * p.rows_per_slab;
    const long kend = min(p.R, kbeg + p.rows_per_slab);
    const int nk = (int)((kend - kbeg) / BK);
    const int wm0 = (wave >> 1) * WM, wn0 = (wave & 1) * WN;

    // ---- staging role (wave-uniform): thread u of an operand = column quad cq of row octet q
    const bool stA = wave * 64 < BM, stB = !stA && wave * 64 < BM + BN;
    const int u = stA ? tid : tid - BM;
    const int qsh = stA ? (BM == 128 ? 5 : 4) : (BN == 128 ? 5 : 4);          // log2(column quads per tile row)
    const int cq = u & ((1 << qsh) - 1), q = (u >> qsh) & 3;
    const float* gsrc = stA ? p.A + m0 : p.B + n0;
    const long ld = stA ? p.lda : p.ldb;
    const unsigned voff = (unsigned)(((long)(8 * q) * ld + 4 * cq) * 4);
    const unsigned voffh = (unsigned)(((long)(8 * q) * p.ldh + 4 * cq) * 4);
    // image byte offset of (column 4 cq + e, octet q): row (4 cq + e) ^ ((cq >> 2) & 1), slot q ^ (cq & 3)
    const int st0 = ((stA ? 0 : BM) + 4 * cq) * ROWB + ((q ^ (cq & 3)) * 16), stf = ((cq >> 2) & 1) * ROWB;
    int st[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) st[e] = st0 + ((e * ROWB) ^ stf);
    // fragment reads: lane (li, lh) of k-step ks reads octet 2 ks + lh of column w0 + 32 i + li
    const int rrow = li ^ ((li >> 4) & 1), rslot = (lh ^ ((li >> 2) & 3)) * 16;
    const int ra0 = (wm0 + rrow) * ROWB + rslot, rb0 = (BM + wn0 + rrow) * ROWB + rslot;      // (k-step 1: ^ 32)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    f32x4 sa[8], sa2[PRO ? 8 : 1], cf[5];
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[i] = f32x4{0.f, 0.f, 0.f, 0.f};           // (waves without a staging role split zeros)
    if (PRO) {
        // B columns pass through the same arithmetic with the identity's coefficients (z = 1 > 0, dh = 1 dy + (0 h + 0)): the
        // split below stays one branch-free instruction stream for all waves
#pragma unroll
        for (int i = 0; i < 8; ++i) sa2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
        cf[0] = zero; cf[1] = one; cf[2] = one; cf[3] = zero; cf[4] = zero;
        if (stA) {
#pragma unroll
            for (int c = 0; c < 5; ++c) cf[c] = uload4(p.coefs + (long)c * p.M + m0, (unsigned)(cq * 16));
        }
    }
    auto load_tile = [&](long k0) {
        if (stA || stB) {
            const float* ub = gsrc + k0 * ld;                                  // wave-uniform
#pragma unroll
            for (int i = 0; i < 8; ++i) sa[i] = uload4(ub, voff, (unsigned)(i * 4) * (unsigned)ld);
        }
        if (PRO && stA) {
            const float* uh = p.h + m0 + k0 * p.ldh;
#pragma unroll
            for (int i = 0; i < 8; ++i) sa2[i] = uload4(uh, voffh, (unsigned)(i * 4) * (unsigned)p.ldh);
        }
    };
    u32x4 pw[3][4];                                 // [plane][column e]: the 8 k of the thread's octet, packed
    // split item n = (column e, k pair j): two consecutive k of one column -> one word of each plane
    auto split_item = [&](int n) {
        const int e = n >> 2, j = n & 3;
        float x0 = sa[2 * j][e], x1 = sa[2 * j + 1][e];
        if (PRO) {
            x0 = bn_bwd_one(x0, sa2[PRO ? 2 * j : 0][e], cf, e, p.slope);
            x1 = bn_bwd_one(x1, sa2[PRO ? 2 * j + 1 : 0][e], cf, e, p.slope);
        }
        unsigned h, m, l;
        split_pair(x0, x1, h, m, l);
        pw[0][e][j] = h; pw[1][e][j] = m; pw[2][e][j] = l;
        // a finished column is materialised HERE: the compiler otherwise sinks the whole split behind the barrier, next to the
        // stores that consume it
        if (j == 3) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) asm volatile("" : "+v"(pw[pl][e]));
        }
    };
    auto split_all = [&]() {
#pragma unroll
        for (int n = 0; n < 16; ++n) split_item(n);
    };
    auto store_all = [&]() {
        if (stA || stB) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4*>(img + st[e] + pl * PL) = pw[pl][e];
        }
    };
    // one 16-deep k-step: 3 (TM + TN) fragment reads, 6 TM TN MFMAs -- smallest partial products first (l.h  h.l  m.m  m.h  h.m
    // h.h), consecutive MFMAs on different accumulators.  shadow: the 16 split items of the NEXT tile go between the MFMAs, in
    // this order (pinned: left alone, the scheduler issues all MFMAs first and the wave then splits with an idle matrix pipe)
    constexpr int NM = 6 * TM * TN;
    // first split item of MFMA slot g: one per slot in the LAST 16 slots where there are that many (the loads of the tile being
    // split get the first slots' time to land), else evenly spread
    auto item_of = [](int g) { return NM >= 16 ? (g > NM - 16 ? g - (NM - 16) : 0) : g * 16 / NM; };
    auto kstep = [&](int ks, auto shadow_tag) {
        constexpr bool SHADOW = decltype(shadow_tag)::value;
        u32x4 fa[TM][3], fb[TN][3];
        const int ra = ks ? ra0 ^ 32 : ra0, rb = ks ? rb0 ^ 32 : rb0;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) fa[i][pl] = *reinterpret_cast<const u32x4*>(img + ra + i * 32 * ROWB + pl * PL);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) fb[j][pl] = *reinterpret_cast<const u32x4*>(img + rb + j * 32 * ROWB + pl * PL);
#pragma unroll
        for (int g = 0; g < NM; ++g) {
            const int pr = g / (TM * TN), i = (g % (TM * TN)) / TN, j = g % TN;
            const int pa = pr == 0 ? 2 : (pr == 2 || pr == 3 ? 1 : 0), pb = pr == 1 ? 2 : (pr == 2 || pr == 4 ? 1 : 0);
            acc[i][j] = mfma_bf16(fa[i][pa], fb[j][pb], acc[i][j]);
            if (SHADOW) {
#pragma unroll
                for (int n = item_of(g); n < item_of(g + 1); ++n) split_item(n);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    load_tile(kbeg);
    split_all();
    store_all();
    if (nk > 1) load_tile(kbeg + BK);
    lds_barrier();
    for (int kt = 0; kt < nk; ++kt) {
        // (past the last tile the staging registers still hold that tile: split and stored once more, read by nobody)
        kstep(0, std::false_type{});
        __builtin_amdgcn_sched_barrier(0);
#if DC_TNP_SHADOW
        kstep(1, std::true_type{});
#else
        kstep(1, std::false_type{});
        __builtin_amdgcn_sched_barrier(0);
        split_all();
#endif
        lds_barrier();                 // every wave has its fragments of tile kt in registers
        store_all();
        if (kt + 2 < nk) load_tile(kbeg + (long)(kt + 2) * BK);
        lds_barrier();                 // tile kt+1 is in LDS
    }
    __syncthreads();                   // (the staging below reuses the plane images)

    // ---- store: as gemm_kernel -- each wave transposes its WM x WN tile through LDS and writes whole rows, 16 bytes per lane.
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* stg = smem + wave * (WM * WN);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                stg[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * WN + j * 32 + li] = acc[i][j][r];
    __syncthreads();
    float* cbase = p.C + (long)blockIdx.y * ((long)p.M * p.N);
    constexpr int RL = WN / 4;                         // lanes per output row
#pragma unroll
    for (int it = 0; it < WM * WN / 4 / 64; ++it) {
        const int idx = it * 64 + lane;
        const int r = idx / RL, c4 = (idx % RL) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(stg + r * WN + c4);
        dc_store16<DC_ST_GEMM>(cbase + (long)(m0 + wm0 + r) * p.N + n0 + wn0 + c4, v);
    }
}

template <int BM, int BN, int PRO>
bool launch_one(const DcTnPlanesP& p, int slabs, hipStream_t s) {
    static unsigned long long configured = 0;
    const size_t lds = std::max((size_t)3 * (BM + BN) * ROWB, (size_t)BM * BN * sizeof(float));      // plane images | output staging
    if (!dc_ensure_lds(&configured, reinterpret_cast<const void*>(&gemm_tn_planes_kernel<BM, BN, PRO>), lds, "weight gradient"))
        return false;
    hipLaunchKernelGGL((gemm_tn_planes_kernel<BM, BN, PRO>), dim3((unsigned)((p.M / BM) * (p.N / BN)), (unsigned)slabs), dim3(NT),
                       lds, s, p);
    return true;
}
template <int PRO>
bool launch_tile(int bm, int bn, const DcTnPlanesP& p, int slabs, hipStream_t s) {
    if (bm == 128 && bn == 128) return launch_one<128, 128, PRO>(p, slabs, s);
    if (bm == 128) return launch_one<128, 64, PRO>(p, slabs, s);
    if (bn == 128) return launch_one<64, 128, PRO>(p, slabs, s);
    return launch_one<64, 64, PRO>(p, slabs, s);
}

}  // namespace

bool dc_tn_planes_launch(int bm, int bn, const DcTnPlanesP& p, int slabs, hipStream_t s) {
    return p.h ? launch_tile<1>(bm, bn, p, slabs, s) : launch_tile<0>(bm, bn, p, slabs, s);
}
