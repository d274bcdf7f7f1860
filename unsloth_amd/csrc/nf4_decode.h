// The NF4 format's device side, shared by every kernel that decodes it (nf4.hip, gemm.hip, decode.hip): the 16 levels, the
// staging of the level tables into LDS and the packed-word decode. One definition of each: the nibble order and the
// rounding point below are the bitsandbytes format (see the head of nf4.hip), and tests/test_checkpoint_format.py pins
// this table -- the only one in the C sources -- to its published construction.
#pragma once
#include "common.h"

// internal linkage: every .hip that includes this header gets its own __constant__ copy
static __constant__ float kNF4[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
    0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f};

// Stage a level table (lut_g, NULL = the NF4 levels) and, for nested statistics, the 256-entry map of the absmax codes
// (code2_g, NULL = none) into LDS. Blocks of 256 threads; the caller's __syncthreads() makes them visible.
__device__ __forceinline__ void nf4_stage_level(float* lut, const float* lut_g, int i) {      // entry i of 16
    lut[i] = lut_g ? lut_g[i] : kNF4[i];
}
__device__ __forceinline__ void nf4_stage_tables(float* lut, const float* lut_g, float* code2, const float* code2_g) {
    if (threadIdx.x < 16) nf4_stage_level(lut, lut_g, threadIdx.x);
    if (code2_g) code2[threadIdx.x] = code2_g[threadIdx.x];
}

// 4 packed bytes -> 8 consecutive elements that share one absmax: HIGH nibble = even element, LOW nibble = odd element,
// lut[code] * absmax in fp32, rounded once to T.
template <typename T>
__device__ __forceinline__ void nf4_decode8(uint32_t w, const float* lut, float absmax, T* o) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t byte = (w >> (8 * b)) & 0xff;
        o[2 * b] = from_f32<T>(lut[byte >> 4] * absmax);
        o[2 * b + 1] = from_f32<T>(lut[byte & 15] * absmax);
    }
}
