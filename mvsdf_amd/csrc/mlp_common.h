// mlp_common.h -- device-side description of a folded MLP on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).  The MFMA-packed weight layout the kernels
// consume without any LDS staging of weights (MvLayer::wp, Kp = ceil32(K), Np = ceil16(N)) is defined in pack_layout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pack_layout.h"

#define MV_MAXL 12

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MvLayer {
    const float4* wp;   // packed [NT][KB][64] float4
    const float* bias;  // [N]
    int K, N;           // true in / out
    int KB, NT;         // k-blocks of 16, column tiles of 16
};

struct MvNet {
    MvLayer L[MV_MAXL];
    int n_layers;
    unsigned skip_mask; // bit l set: the input of layer l is cat([x, PE]) / sqrt(2)  (idr.py:86-87; the shipped conf: layer 4 only)
    int multires;       // PE frequencies; d_pe = 3 + 6*multires
    int S;              // LDS activation row stride in floats (== 8 mod 64: conflict-free ds_read_b128 A fragments)
};

__host__ __device__ static inline bool mv_skip_at(unsigned mask, int l) { return l >= 0 && ((mask >> l) & 1u) != 0; }
// position of logical column c inside an LDS activation row: 4x4 transpose within each 16-block so that a
// lane's four consecutive k-steps (k = 4s + q) are one contiguous float4 at 4q..4q+3.
__host__ __device__ static inline int mv_perm(int c) { return (c & ~15) | ((c & 3) << 2) | ((c >> 2) & 3); }
