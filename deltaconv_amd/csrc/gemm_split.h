// Device helpers shared by the dense-product kernels (gemm.hip, gemm_tn_planes.hip): 16-byte buffer loads, the LDS-only barrier,
// the BatchNorm-backward operand prologue and the bf16 split (three planes per fp32 value) with its MFMA.
#pragma once
#include "common.h"

namespace dcsplit {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Fast-path load: buffer_load through a descriptor built from the wave-uniform tile origin (SGPRs), a wave-uniform
// byte offset (soff: which of the thread's loads) and ONE 32-bit per-thread byte offset per operand (voff) -- no 64-bit
// per-load address registers and no VALU address arithmetic in the K loop.  num_records = 2^31: no range clipping.
__device__ __forceinline__ f32x4 uload4(const float* ubase, unsigned voff, unsigned soff = 0) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ubase), 0, 0x7FFFFFFF, 0x00020000);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return __builtin_bit_cast(f32x4, v);
}

// BatchNorm / activation backward of four columns: dz = dy (c_sc h + c_sh > 0 ? 1 : slope), dh = c_g dz + c_a h + c_b
__device__ __forceinline__ float bn_bwd_one(float dy, float h, const f32x4 (&cf)[5], int e, float slope) {
    const float z = fmaf(cf[0][e], h, cf[1][e]);
    const float dz = dy * (z > 0.f ? 1.f : slope);
    return fmaf(cf[2][e], dz, fmaf(cf[3][e], h, cf[4][e]));
}
__device__ __forceinline__ f32x4 bn_bwd_vec(const f32x4 dy, const f32x4 h, const f32x4 (&cf)[5], float slope) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = bn_bwd_one(dy[e], h[e], cf, e, slope);
    return o;
}

// Workgroup barrier that orders LDS traffic only: __syncthreads() also drains the vector-memory counter (vmcnt(0)),
// which would make every K tile wait for the global loads issued for the tiles AFTER the next one.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_sched_barrier(0);      // nothing is scheduled across (the MFMAs are not memory operations)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- split products (X3): an fp32 value x is cut into three bfloat16 planes, x = hi + mid + lo up to 2^-25 |x|
// (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); both differences are exact in fp32), and the product
// of two fp32 operands is accumulated from the six partial products of weight >= 2^-16 (lo.hi, hi.lo, mid.mid, mid.hi,
// hi.mid, hi.hi) on the bf16 matrix pipe with fp32 accumulation: v_mfma_f32_32x32x16_bf16 retires 16x the
// multiply-adds per cycle of v_mfma_f32_32x32x2_f32, so six of them cost 6/16 of the exact chain.  The dropped terms
// (mid.lo, lo.mid, lo.lo) are below 2^-23 of |a||b|, and each instruction sums 16 products before the one rounding
// into the accumulator: measured error against fp64 is BELOW the fp32 chain's (profiles/r03o_bf16x3_lab.txt).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {      // v_cvt_pk_bf16_f32 (round to nearest even)
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = pk_bf16(x0, x1);
    const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xFFFF0000u);
    m = pk_bf16(r0, r1);
    const float s0 = r0 - __builtin_bit_cast(float, m << 16), s1 = r1 - __builtin_bit_cast(float, m & 0xFFFF0000u);
    l = pk_bf16(s0, s1);
}
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4 a, const u32x4 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

}  // namespace dcsplit
