// The row normalisers of the token store (bert_hip.h "Token store"), shared by the
// scorers (maxsim.hip, maxsim_i8.hip) and the full-scan search (maxsim_search.hip): one
// definition each for stored rows and for query rows, so the kernels cannot drift apart.
#pragma once

#include "device_common.h"
#include "quant_i8.h"

namespace emb {

// One wave normalises row x f32 [w]: lane l takes the 8-element chunks l and l + 64
// (w / 8 <= 128 chunks).  Sum of squares: each lane adds its chunks' squares in element
// order into one f32 (lanes without a chunk hold 0), then the xor butterfly of
// wave_sum; the order depends on w only.  out[j] = chunk l + 64 j as f16, zeros for a
// chunk the row does not have and for a row whose sum of squares is 0.
__device__ __forceinline__ void pack_row_f16(const float *__restrict__ x, int w, int lane, h16x8 (&out)[2])
{
    const int chunks = w >> 3;
    float v[2][8];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (c < chunks) {
            a = *(const float4 *)(x + 8 * c);
            b = *(const float4 *)(x + 8 * c + 4);
        }
        v[j][0] = a.x; v[j][1] = a.y; v[j][2] = a.z; v[j][3] = a.w;
        v[j][4] = b.x; v[j][5] = b.y; v[j][6] = b.z; v[j][7] = b.w;
#pragma unroll
        for (int i = 0; i < 8; ++i) ss = __fadd_rn(ss, __fmul_rn(v[j][i], v[j][i]));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss = __fadd_rn(ss, __shfl_xor(ss, o, 64));
    const float rinv = ss > 0.f ? __fdiv_rn(1.0f, __fsqrt_rn(ss)) : 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) out[j][i] = ss > 0.f ? (h16)__fmul_rn(v[j][i], rinv) : (h16)0.0f;
}

// Where 16-byte chunk c of row `row` sits in an image of KB blocks per group, in 16-byte
// units: the A fragment of a stored row and the B fragment of a query alike.  f16: chunk
// c = elements 8c .. 8c + 7, KB = w / 32; int8: chunk c = bytes 16c .. 16c + 15, KB = w / 64.
__device__ __forceinline__ size_t frag_index(int64_t row, int c, int KB)
{
    return (size_t)((row >> 4) * KB + (c >> 2)) * 64 + 16 * (c & 3) + (int)(row & 15);
}

// u of a quantized row, the lanes' bytes in v.  n2: each lane adds the squares of its 16
// bytes (v_dot4_i32_i8), wave_sum_i32 adds the lanes; integer sums, so the order is
// immaterial.
__device__ __forceinline__ float unit_scale_i8(i32x4 v)
{
    int n2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) n2 = __builtin_amdgcn_sdot4(v[i], v[i], n2, false);   // four signed bytes each
    n2 = wave_sum_i32(n2);
    // sqrtf, not __fsqrt_rn: the intrinsic is the hardware's approximate root in this toolchain
    return n2 > 0 ? __fdiv_rn(1.0f, sqrtf((float)n2)) : 0.f;
}

// One wave packs row x f32 [w]: lane c < w / 16 gets bytes 16c .. 16c + 15 (the other
// lanes zeros), every lane gets u.
__device__ __forceinline__ i32x4 pack_row_i8(const float *__restrict__ x, int w, int lane, float &u)
{
    float scale;
    const i32x4 v = quantize_row_i8(x, w, lane, scale);
    u = unit_scale_i8(v);
    return v;
}

}  // namespace emb
