// The int8 row arithmetic shared by the embedding index (search.hip) and the token store
// (maxsim_i8.hip): one quantizer for stored rows and for queries, and the score of two
// quantized rows (bert_hip.h, "Storage kinds").
#pragma once

#include "device_common.h"

namespace emb {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// max and integer sum over the 64 lanes of a wave, the result in every lane: four DPP
// steps inside each row of 16 lanes (two quad permutes, the half-row and the row
// mirror), then the four rows' values by readlane.  Both operations are exact, so the
// result does not depend on the order: the bits of an xor butterfly, without its six
// trips through the LDS crossbar.
__device__ __forceinline__ float wave_max_f32(float x)
{
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xb1, 0xf, 0xf, true)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4e, 0xf, 0xf, true)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x141, 0xf, 0xf, true)));
    x = fmaxf(x, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x140, 0xf, 0xf, true)));
    const int b = __float_as_int(x);
    return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(b, 0)), __int_as_float(__builtin_amdgcn_readlane(b, 16))),
                 fmaxf(__int_as_float(__builtin_amdgcn_readlane(b, 32)), __int_as_float(__builtin_amdgcn_readlane(b, 48))));
}

__device__ __forceinline__ int wave_sum_i32(int x)
{
    x += __builtin_amdgcn_mov_dpp(x, 0xb1, 0xf, 0xf, true);
    x += __builtin_amdgcn_mov_dpp(x, 0x4e, 0xf, 0xf, true);
    x += __builtin_amdgcn_mov_dpp(x, 0x141, 0xf, 0xf, true);
    x += __builtin_amdgcn_mov_dpp(x, 0x140, 0xf, 0xf, true);
    return __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
           __builtin_amdgcn_readlane(x, 48);
}

// The int8 quantizer of stored rows and of queries, one wave per row x f32 [d]: lane
// c < d / 16 takes elements 16c .. 16c + 15 and returns their 16 bytes (element 16c + j
// in byte j), the other lanes return zeros; every lane gets the row's scale.
//   amax = max |x_i|;  amax == 0: scale 0, every q 0;  else inv = 127 / amax,
//   q_i = clamp(rint(x_i * inv), -127, 127) (nearest even), scale = amax / 127,
// each operation rounded once to f32.  Non-finite input: the clamp still holds (a NaN
// product becomes -127), the values are unspecified.
// quantize_row_i8 is its three steps in order; a caller that packs several rows at once
// (the MaxSim query prologue) calls the steps itself, so that the rows' loads and
// reductions overlap.  The statements are the same either way.  Against the quantizer as
// search.hip first had it, the maximum over the lanes is taken by wave_max_f32 where an
// xor butterfly of shuffles stood: the same value, max being exact.
__device__ __forceinline__ void load_row_i8(const float *__restrict__ x, int d, int lane, float (&v)[16])
{
    const bool on = lane < (d >> 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float4 a = {0.f, 0.f, 0.f, 0.f};
        if (on) a = *(const float4 *)(x + 16 * lane + 4 * j);
        v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
    }
}

__device__ __forceinline__ float row_amax_i8(const float (&v)[16])
{
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
    return wave_max_f32(amax);
}

__device__ __forceinline__ i32x4 quantize_values_i8(const float (&v)[16], float amax, float &scale)
{
    i32x4 out = {0, 0, 0, 0};
    scale = 0.f;
    if (!(amax > 0.f)) return out;
    const float inv = __fdiv_rn(127.0f, amax);
    scale = __fdiv_rn(amax, 127.0f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float r = fminf(fmaxf(rintf(__fmul_rn(v[i], inv)), -127.0f), 127.0f);
        out[i >> 2] |= ((int)r & 0xff) << (8 * (i & 3));
    }
    return out;
}

__device__ __forceinline__ i32x4 quantize_row_i8(const float *__restrict__ x, int d, int lane, float &scale)
{
    float v[16];
    load_row_i8(x, d, lane, v);
    return quantize_values_i8(v, row_amax_i8(v), scale);
}

// The int8 score: the i32 sum is exact in f32 (|isum| <= 127 * 127 * 1024 < 2^24).
__device__ __forceinline__ float score_i8(int isum, float scale_q, float scale_row)
{
    return __fmul_rn((float)isum, __fmul_rn(scale_q, scale_row));
}

}  // namespace emb
