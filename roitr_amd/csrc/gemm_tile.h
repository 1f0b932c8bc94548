// What the kernels of the GEMM family (gemm.hip, gemm_bf16.hip, gemm_x3.hip) share on the device side: the block tile, the MFMA
// operand and accumulator types and the bf16 packing.  Everything else around the K loops stays written out in each kernel: routed
// through shared __forceinline__ helpers (even the one-line 32 x 32 C/D row map), hipcc allocates the timed kernels' registers
// differently ("GEMM family: what is shared and what is not").
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int BM = 64, BN = 64;   // block rows; columns per accumulator pair of a block (the block tile is 64 x 64 TN)

__device__ __forceinline__ unsigned pack_bf16(float x, float y)   // low half = x; round to nearest even
{
    f32x2 v = {x, y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ unsigned short to_bf16(float x) { return (unsigned short)(pack_bf16(x, 0.f) & 0xffffu); }
