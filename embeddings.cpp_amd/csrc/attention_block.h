// The K / V image layout of the LDS attention kernels and the dh-64 family's
// per-query block arithmetic (attention.hip, its only includer).
#pragma once

#include "device_common.h"

namespace emb {

// ---------------------------------------------------------------------------
// LDS image of K and V: [key][DH] rows of CH 16-B chunks; chunk j of row r
// lives at chunk j ^ swz(r), swz = row_swz(r).k in the K image and .v in the V
// image.  Every writer and reader of an image goes through this one function.
//   K: the 16 lanes of a ds_read_b128 group read 16 rows ({0-3,12-15,20-27} +
//      32n) at one chunk; XOR with (row >> 1) & 7 (128-B rows) or
//      (row >> 2) & 3 (64-B rows) puts them on 16 distinct 16-B bank slots.
//   V: read with ds_read_b64_tr_b16; 128-B rows swap their 64-B halves on
//      every second row pair, 64-B rows need no swizzle.
// Both depend on row bits 1-4 at most, so the offsets of a 32-row-aligned
// block are lane constants.  (One function returning both, sharing row >> 1:
// as two functions each is simplified on its own before it is inlined, and
// attention_lds3's issue then compiles to other address code, measured 0.8 %
// slower per item on its 7-workgroup form.)
// ---------------------------------------------------------------------------
struct RowSwz { int k, v; };
template <int CH>
__device__ __forceinline__ RowSwz row_swz(int row)
{
    static_assert(CH == 8 || CH == 4, "128-B or 64-B rows");
    const int h = row >> 1;
    if constexpr (CH == 8) return RowSwz{h & 7, (h & 1) << 2};
    else return RowSwz{(row >> 2) & 3, 0};
}

// ---------------------------------------------------------------------------
// AttWave64: the 32 queries of one wave at dh 64 (query on the lane, both
// 32-lane halves hold the same query), fixed-offset softmax:
//  * each query keeps an f16 offset c (the max of its first block) and S - c
//    comes out of the MFMA itself -- one extra MFMA per 32 keys multiplies a
//    ones-column of K by a (-c)-row of Q.  softmax(S) = exp2(S - c) /
//    sum exp2(S - c) for any c, so the result is the function of the
//    running-max form.  No max is taken per block: a block whose 32-key
//    partial row sum exceeds 2^ATT_SUMX (so some P may leave the safe f16
//    range) is recomputed after moving c to the row max and rescaling O and
//    l -- rare, and it keeps every P <= 2^ATT_SUMX.
//  * the row sum stays per 32-lane half (no cross-lane op per block); the
//    halves are combined once, by v_permlane32_swap, in store().
//  * LDS reads at base + immediate offsets (the swizzles of both images are
//    lane constants): six address adds per block.
// attention_lds3, attention_pp and attention_short run their queries through
// this one definition, which is what makes a sentence's bits independent of the
// kernel (and so of the batch) it lands in.  The kernels own the K / V image
// (k_base / v_base: the byte offsets of a 64-key block's K and V rows from
// `lds`), the loads of qf, and every wait and barrier.
// ---------------------------------------------------------------------------
constexpr int ATT_SUMX = 12;   // a block whose half-row sum passes 2^ATT_SUMX moves the offset

struct AttWave64 {
    static constexpr int DH = 64, RB = DH * 2, CH = RB / 16;

    h16x8 qf[DH / 16];        // the query's row: raw from the kernel's loads, then scale_q
    f32x16 o[DH / 32];        // O^T, unnormalised
    f32x16 s[2];              // the block's scores, then P
    float c, l;               // offset (f16-exact), this half's row sum
    h16x8 abias, bbias;       // the bias MFMA's operands: ones-column of K, (-c)-row of Q
    int koff[DH / 16], voff[DH / 32];   // lane-constant offsets into a block's K / V rows
    const char *lds;
    int nk, rows, hi;         // counted keys (the mask), the sentence's rows (the store's bound)

    // lane roles and bias operands; `vo` is added to every V offset
    __device__ __forceinline__ void init(int lane, const char *lds_, int vo)
    {
        lds = lds_;
        hi = lane >> 5;
        const int lq = lane & 31;
#pragma unroll
        for (int st = 0; st < DH / 16; ++st) koff[st] = lq * RB + (((2 * st + hi) ^ row_swz<CH>(lq).k) << 4);
        // tr-read lane roles: group gg = lane >> 4 reads rows r0 + (i >> 2), columns c0 + 4 (i & 3)
        const int gi = lane & 15, gq = gi >> 2, gp = gi & 3, gg = lane >> 4;
        const int vrow = 4 * (gg >> 1) + gq;
#pragma unroll
        for (int t = 0; t < DH / 32; ++t) {
            const int ch = 4 * t + 2 * (gg & 1) + (gp >> 1);
            voff[t] = vrow * RB + ((ch ^ row_swz<CH>(vrow).v) << 4) + 8 * (gp & 1) + vo;
        }
        const h16 one = (h16)1.0f, zero = (h16)0.0f;
        abias = h16x8{hi ? zero : one, zero, zero, zero, zero, zero, zero, zero};
        bbias = h16x8{zero, zero, zero, zero, zero, zero, zero, zero};
        c = 0.f;
        l = 0.f;
        nk = 0;
        rows = 0;
    }
    // a new query: nothing of the block state stays live
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int t = 0; t < DH / 32; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
        c = 0.f;
        l = 0.f;
        bbias[0] = (h16)0.0f;
    }
    // Q pre-scaled by log2(e) / sqrt(dh) in f16, so S comes out in the exp2 domain
    __device__ __forceinline__ void scale_q(float sl2)
    {
        const h16 s16 = (h16)sl2;
        const h16x8 sc = {s16, s16, s16, s16, s16, s16, s16, s16};
#pragma unroll
        for (int st = 0; st < DH / 16; ++st) qf[st] *= sc;
    }
    __device__ __forceinline__ void set_offset(float c_)
    {
        c = c_;
        bbias[0] = hi ? (h16)0.0f : (h16)(-c);
    }

    // S^T = K Q^T (- c with bias) of keys kb .. kb + 63; keys past the counted ones -inf
    __device__ __forceinline__ void qk(int kb, int k_base, bool bias)
    {
        int kbo[DH / 16];
#pragma unroll
        for (int st = 0; st < DH / 16; ++st) {
            kbo[st] = koff[st] + k_base;
            asm volatile("" : "+v"(kbo[st]));
        }
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            if (bias) {
                s[kh] = __builtin_amdgcn_mfma_f32_32x32x16_f16(abias, bbias, f32x16{}, 0, 0, 0);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kh][r] = 0.f;
            }
#pragma unroll
            for (int st = 0; st < DH / 16; ++st) {
                const h16x8 a = *(const h16x8 *)(lds + kbo[st] + kh * 32 * RB);
                s[kh] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[st], s[kh], 0, 0, 0);
            }
        }
        if (kb + 64 > nk) {
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kb + 32 * kh + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key >= nk) s[kh][r] = -INFINITY;
                }
        }
    }
    __device__ __forceinline__ float row_max() const      // over both halves
    {
        float mx = s[0][0];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = (kh ? 0 : 1); r < 16; ++r) mx = fmaxf(mx, s[kh][r]);
        return halves_max(mx);
    }
    __device__ __forceinline__ void shift_by(float sh)    // scores -= sh
    {
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kh][r] -= sh;
    }
    __device__ __forceinline__ float expsum()             // s <- exp2(s); this half's sum
    {
        float rs = 0.f;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[kh][r]);
                s[kh][r] = p;
                rs += p;
            }
        return rs;
    }
    // O^T += V^T P^T, the S accumulator reused as the B operand
    __device__ __forceinline__ void pv(int v_base)
    {
        int vbo[DH / 32];
#pragma unroll
        for (int t = 0; t < DH / 32; ++t) {
            vbo[t] = voff[t] + v_base;
            asm volatile("" : "+v"(vbo[t]));
        }
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                h16x8 bp;
#pragma unroll
                for (int j = 0; j < 8; ++j) bp[j] = (h16)s[kh][8 * s2 + j];
#pragma unroll
                for (int t = 0; t < DH / 32; ++t) {
                    const char *va = lds + vbo[t] + (32 * kh + 16 * s2) * RB;
                    const h16x4 lo = lds_read_tr16(va);
                    const h16x4 up = lds_read_tr16(va + 8 * RB);
                    const h16x8 a = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
                    o[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bp, o[t], 0, 0, 0);
                }
            }
        }
    }

    // keys 0-63: the offset is their row max (f16-rounded)
    __device__ __forceinline__ void block0(int k_base, int v_base)
    {
        qk(0, k_base, false);
        const float m = (float)(h16)row_max();
        shift_by(m);
        set_offset(m);
        l = expsum();
        pv(v_base);
    }
    // keys kb .. kb + 63, kb > 0
    __device__ __forceinline__ void block(int kb, int k_base, int v_base)
    {
        qk(kb, k_base, true);                             // S - c
        float rs = expsum();
        if (__builtin_amdgcn_ballot_w64(rs > (float)(1 << ATT_SUMX))) {
            // rare: move c to the row max, rescale, redo the block
            qk(kb, k_base, true);
            const float m = row_max();
            const float sh = m > 0.f ? (float)(h16)(c + m) - c : 0.f;
            const float alpha = __builtin_amdgcn_exp2f(-sh);
            shift_by(sh);
            set_offset(c + sh);
            l *= alpha;
#pragma unroll
            for (int t = 0; t < DH / 32; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
            rs = expsum();
        }
        l += rs;
        pv(v_base);
    }

    // Row q of the sentence at `start` (the lane's query), head h: O / l as f16.
    // Lane (q, hi) holds dh 8m + 4 hi .. +3 of chunks m = 4t + g; one
    // v_permlane32_swap per dword of the chunk pair (2p, 2p + 1) gives lane
    // (q, 0) dh 16p .. 16p + 7 and lane (q, 1) dh 16p + 8 .. 16p + 15: four
    // 16-B stores per lane instead of eight 8-B ones (the store tail is
    // issue-bound).  Both lanes of a pair hold the same query, so the swaps
    // run on every lane.  The stores are bounds-checked buffer stores with the
    // sentence's rows [start, start + rows) of `out` as the resource: a row
    // q >= rows lies past num_records and its store is dropped.  (rows is the
    // sentence's length whatever its key count: every row is a query.)
    __device__ __forceinline__ void store(h16 *out, int start, int d, int h, int q) const
    {
        static_assert(DH / 16 == 4, "four stores per lane");
        const float inv = 1.0f / halves_sum(l);
        uint32_t pk[DH / 8][2];
#pragma unroll
        for (int m = 0; m < DH / 8; ++m)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int t = m >> 2, g = m & 3;
                const h16x2 v = {(h16)(o[t][4 * g + 2 * k] * inv), (h16)(o[t][4 * g + 2 * k + 1] * inv)};
                pk[m][k] = __builtin_bit_cast(uint32_t, v);
            }
#pragma unroll
        for (int p = 0; p < DH / 16; ++p)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const auto r = __builtin_amdgcn_permlane32_swap(pk[2 * p][k], pk[2 * p + 1][k], false, false);
                pk[2 * p][k] = r[0];
                pk[2 * p + 1][k] = r[1];
            }
        const __amdgpu_buffer_rsrc_t ors =
            __builtin_amdgcn_make_buffer_rsrc((void *)(out + (size_t)start * d), (short)0, rows * d * 2, 0x00020000);
        const int ob = (q * d + h * DH + 8 * hi) * 2;
#pragma unroll
        for (int p = 0; p < DH / 16; ++p) {
            typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
            const u32x4v v = {pk[2 * p][0], pk[2 * p][1], pk[2 * p + 1][0], pk[2 * p + 1][1]};
            __builtin_amdgcn_raw_buffer_store_b128(v, ors, ob + 32 * p, 0, 0);
        }
    }
};

}  // namespace emb
