// Weight gradient on bf16 plane images in LDS (gemm_tn_planes.hip), selected by dc_tn_lds_launch (gemm.hip).
#pragma once
#include <hip/hip_runtime.h>

struct DcTnPlanesP {
    const float* A; long lda;              // [R, M] (with the prologue: dy)
    const float* B; long ldb;              // [R, N]
    float* C;                              // partial tiles [slabs][M][N]
    int M, N;
    long R, rows_per_slab;                 // both multiples of 32
    // BatchNorm-backward prologue (h != nullptr): A = bn_act_backward(dy, h) with packed coefficients [5][M]
    const float* h; long ldh;
    const float* coefs; float slope;
};

// Whole tiles only: M % bm == 0, N % bn == 0, 16-byte aligned operands and leading dimensions (load_mode() == 0 of gemm.hip).
// Enqueues one launch of (M / bm) (N / bn) x slabs workgroups; false when the device cannot give the LDS (dc_take_lds_failure()).
bool dc_tn_planes_launch(int bm, int bn, const DcTnPlanesP& p, int slabs, hipStream_t s);
