// The binary row arithmetic shared by the Hamming search (search_bin.hip) and the scorer
// of listed rows (search_rescore.hip): one binarizer for stored rows and for queries, the
// stored layout, and the score of two bit rows (bert_hip.h, "Binary storage").
//
// Stored layout ("bit order"): rows in groups of 64, lane = row of the group, a group's
// NB = ceil(d / 128) blocks consecutive, a block = 64 rows x 128 bits = 1 KiB, lane l of
// a block holds bits 128c .. 128c + 127 of row l as one 16-B chunk: element i of a row is
// bit i % 32 of dword (i % 128) / 32 of chunk i / 128.  One global_load_dwordx4 per wave
// is one contiguous block.  Where d is no multiple of 128 the last chunk's upper 64 bits
// are zeros in rows and in queries alike, so they add nothing to the xor.
#pragma once

#include "device_common.h"

namespace emb {

// x > 0, taken on the bits so that no denormal mode can change it: +0, -0, negative
// values and NaN give false; the smallest subnormal and +inf give true.
__device__ __forceinline__ bool bin_positive(float x)
{
    return (uint32_t)(__float_as_uint(x) - 1u) < 0x7f800000u;
}

__device__ __forceinline__ uint4 bin_pack(unsigned long long lo, unsigned long long hi)
{
    return uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

// Chunk c (128 c < d) of row x f32 [d] by one whole wave, the result in every lane:
// lane l tests elements 128c + l and 128c + 64 + l (zeros past d; d % 64 == 0).
__device__ __forceinline__ uint4 bin_chunk(const float *__restrict__ x, int d, int c, int lane)
{
    const float x0 = x[128 * c + lane];
    const float x1 = 128 * c + 64 < d ? x[128 * c + 64 + lane] : 0.f;
    return bin_pack(__ballot(bin_positive(x0)), __ballot(bin_positive(x1)));
}

// Index, in 16-B chunks, of chunk c of row `row` in an image of NB blocks per group.
__device__ __forceinline__ size_t bin_slot(int64_t row, int NB, int c)
{
    return ((size_t)(row >> 6) * NB + c) * 64 + (size_t)(row & 63);
}

// popcount(x) + acc in one instruction.  Written as __builtin_popcount(x) + acc the compiler
// re-associates four of them into four v_bcnt_u32_b32 with a zero operand and two adds.
__device__ __forceinline__ int bin_count(uint32_t x, int acc)
{
    int out;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(out) : "v"(x), "v"(acc));
    return out;
}

// acc + popcount(a xor b): v_xor_b32 and v_bcnt_u32_b32, four times.
__device__ __forceinline__ int bin_distance(uint4 a, uint4 b, int acc)
{
    acc = bin_count(a.x ^ b.x, acc);
    acc = bin_count(a.y ^ b.y, acc);
    acc = bin_count(a.z ^ b.z, acc);
    acc = bin_count(a.w ^ b.w, acc);
    return acc;
}

// The score: d - 2 hamming, the dot product of the two +-1 vectors, exact in f32.
__device__ __forceinline__ float bin_score(int d, int hamming) { return (float)(d - 2 * hamming); }

}  // namespace emb
