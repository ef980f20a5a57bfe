// Union and fusion of the hybrid dense + sparse search (bert_hip.h "Hybrid search";
// DESIGN.md 9i-6).  Two kernels, one wave per query, grid B, around the two scorers of listed
// ids: hybrid_union_kernel merges the two stages' candidate lists into the ascending list of
// their distinct ids with each id's 1-based position in either list; hybrid_fuse_kernel
// turns the two scores (linear) or the two positions (reciprocal rank) of every id into the
// fused score and writes the k best.
//
// Both are a 128-key bitonic sort across the wave, sort128 below, the one place that can go
// wrong: element p = lane + 64 r lies in register r of the lane; the steps 32 .. 1 apart
// trade keys by __shfl_xor, the step 64 apart is a compare-exchange within the lane.  Keys
// are 64-bit and ascend; an optional 32-bit payload travels with its key.  No LDS, no atomics.
//
// The fused score is built from single f32 operations rounded to nearest, mul_rn / add_rn /
// __fdiv_rn, never contracted into an FMA, so numpy's float32 arithmetic restates it.
#include "device_common.h"
#include "kernels.h"

namespace emb {
namespace {

constexpr uint64_t kLast = ~0ull;   // the key that sorts behind every candidate

template <bool PAY>
__device__ __forceinline__ void exchange(uint64_t &ka, uint32_t &pa, uint64_t kb, uint32_t pb, bool keep_min)
{
    if (keep_min ? kb < ka : ka < kb) {
        ka = kb;
        if constexpr (PAY) pa = pb;
    }
}

// key[r] / pay[r] of lane l = element l + 64 r; on return the 128 keys ascend in that numbering
// (equal keys stay where they are).
template <bool PAY>
__device__ __forceinline__ void sort128(uint64_t (&key)[2], uint32_t (&pay)[2], int lane)
{
#pragma unroll
    for (int k = 2; k <= 128; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            if (j == 64) {   // k = 128, ascending: the smaller key to register 0
                if (key[1] < key[0]) {
                    const uint64_t t = key[0];
                    key[0] = key[1];
                    key[1] = t;
                    if constexpr (PAY) {
                        const uint32_t u = pay[0];
                        pay[0] = pay[1];
                        pay[1] = u;
                    }
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint64_t ok = __shfl_xor((unsigned long long)key[r], j, 64);
                uint32_t op = 0;
                if constexpr (PAY) op = __shfl_xor(pay[r], j, 64);
                const bool up = ((lane + 64 * r) & k) == 0, lower = (lane & j) == 0;
                exchange<PAY>(key[r], pay[r], ok, op, lower == up);
            }
        }
    }
}

// cd / cs int32 [B][n_cand]: the stages' candidates, -1 the fill, the ids of one list distinct.
// U int32 [B][2 n_cand]: the distinct ids >= 0 ascending, then -1; rd / rs int32 [B][2 n_cand]:
// the id's 1-based position in cd / cs, 0 when the list lacks it (and behind the ids).
__global__ __launch_bounds__(64) void hybrid_union_kernel(const int32_t *__restrict__ cd, const int32_t *__restrict__ cs,
                                                          int n_cand, int32_t *__restrict__ U, int32_t *__restrict__ rd,
                                                          int32_t *__restrict__ rs)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    // key = id (unsigned: -1 sorts last) : list : position, so of two equal ids the dense one comes first
    uint64_t key[2] = {kLast, kLast};
    uint32_t none[2] = {0u, 0u};
    if (lane < n_cand) {
        const int32_t d = cd[(size_t)b * n_cand + lane], s = cs[(size_t)b * n_cand + lane];
        if (d >= 0) key[0] = (uint64_t)(uint32_t)d << 32 | (uint32_t)(lane + 1);
        if (s >= 0) key[1] = (uint64_t)(uint32_t)s << 32 | 0x100u | (uint32_t)(lane + 1);
    }
    sort128<false>(key, none, lane);

    // the neighbours of element p = lane + 64 r in the sorted order
    const uint64_t last0 = __shfl((unsigned long long)key[0], 63, 64), first1 = __shfl((unsigned long long)key[1], 0, 64);
    int at = 0;   // distinct ids in front of this register's elements
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint64_t prev = __shfl_up((unsigned long long)key[r], 1, 64), next = __shfl_down((unsigned long long)key[r], 1, 64);
        if (lane == 0) prev = r == 0 ? kLast : last0;
        if (lane == 63) next = r == 0 ? first1 : kLast;
        const uint32_t id = (uint32_t)(key[r] >> 32), lo = (uint32_t)key[r];
        // the first element of an id >= 0 (kLast's id is above every id, in front of element 0 too)
        const bool first = key[r] != kLast && (uint32_t)(prev >> 32) != id;
        const unsigned long long heads = __ballot(first);
        if (first) {
            const bool pair = (uint32_t)(next >> 32) == id;   // the sparse list holds it too
            const bool sparse = (lo & 0x100u) != 0;
            const size_t o = (size_t)b * 2 * n_cand + at + __popcll(heads & ((1ull << lane) - 1ull));
            U[o] = (int32_t)id;
            rd[o] = sparse ? 0 : (int32_t)(lo & 0xffu);
            rs[o] = sparse ? (int32_t)(lo & 0xffu) : pair ? (int32_t)((uint32_t)next & 0xffu) : 0;
        }
        at += __popcll(heads);
    }
    for (int i = at + lane; i < 2 * n_cand; i += 64) {
        const size_t o = (size_t)b * 2 * n_cand + i;
        U[o] = -1;
        rd[o] = rs[o] = 0;
    }
}

// f32 bits -> a key that ascends as the value descends; -0 and +0 share one key, and a NaN (inf - inf,
// 0 * inf: scores outside the contract) takes -inf's, so it sorts behind every number and, by its
// id, in front of the fill
__device__ __forceinline__ uint32_t descending_key(float f)
{
    const uint32_t u = __float_as_uint(f == 0.f ? 0.f : f != f ? -INFINITY : f);
    return ~((u & 0x80000000u) ? ~u : u | 0x80000000u);
}

// U, rd, rs as hybrid_union_kernel leaves them, sd / ss f32 [B][2 n_cand] the two scorers' scores
// of U (read only when !RRF).  out_s / out_i [B][k], k <= 2 n_cand: the k best (f, id), f
// descending, equal f by ascending id, the fill (-inf, -1) last.
template <bool RRF>
__global__ __launch_bounds__(64) void hybrid_fuse_kernel(const int32_t *__restrict__ U, const int32_t *__restrict__ rd,
                                                         const int32_t *__restrict__ rs, const float *__restrict__ sd,
                                                         const float *__restrict__ ss, int n_cand, int k, float a,
                                                         float bw, float *__restrict__ out_s, int32_t *__restrict__ out_i)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    uint64_t key[2];
    uint32_t fbits[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        const size_t o = (size_t)b * 2 * n_cand + i;
        int32_t id = i < 2 * n_cand ? U[o] : -1;
        float f = -INFINITY;
        if (id >= 0) {
            if constexpr (RRF) {
                const int32_t pd = rd[o], ps = rs[o];
                const float fd = pd ? __fdiv_rn(1.f, add_rn(a, (float)pd)) : 0.f;
                const float fs = ps ? __fdiv_rn(1.f, add_rn(a, (float)ps)) : 0.f;
                f = add_rn(fd, fs);
            } else {
                const float d = sd[o], s = ss[o];
                if (d == -INFINITY || s == -INFINITY) id = -1;   // one store lacks the id or has deleted it
                else f = add_rn(mul_rn(a, d), mul_rn(bw, s));
            }
        }
        fbits[r] = __float_as_uint(f);
        key[r] = (uint64_t)descending_key(f) << 32 | (uint32_t)id;
    }
    sort128<true>(key, fbits, lane);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        if (i < k) {
            out_s[(size_t)b * k + i] = __uint_as_float(fbits[r]);
            out_i[(size_t)b * k + i] = (int32_t)(uint32_t)key[r];
        }
    }
}

}  // namespace

int launch_hybrid_union(const int32_t *cd, const int32_t *cs, int B, int n_cand, int32_t *U, int32_t *rd, int32_t *rs,
                        hipStream_t s)
{
    if (!cd || !cs || !U || !rd || !rs || B < 1 || n_cand < 1 || n_cand > 64) return -1;
    hybrid_union_kernel<<<(unsigned)B, 64, 0, s>>>(cd, cs, n_cand, U, rd, rs);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_hybrid_fuse(const int32_t *U, const int32_t *rd, const int32_t *rs, const float *sd, const float *ss, int B,
                       int n_cand, int k, bool rrf, float a, float b, float *d_scores, int32_t *d_ids, hipStream_t s)
{
    if (!U || !rd || !rs || !sd || !ss || !d_scores || !d_ids || B < 1 || n_cand < 1 || n_cand > 64 || k < 1 ||
        k > 2 * n_cand)
        return -1;
    if (rrf) hybrid_fuse_kernel<true><<<(unsigned)B, 64, 0, s>>>(U, rd, rs, sd, ss, n_cand, k, a, b, d_scores, d_ids);
    else hybrid_fuse_kernel<false><<<(unsigned)B, 64, 0, s>>>(U, rd, rs, sd, ss, n_cand, k, a, b, d_scores, d_ids);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
