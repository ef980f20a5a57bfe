// Flash-style self-attention for gfx950 (reference bert.cpp:1018-1036).
#include "attention_block.h"
#include "device_common.h"
#include "diag_att_stamps.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <utility>

namespace emb {

// ---------------------------------------------------------------------------
// The running-max kernels (attention: sentences over 512 tokens; attention_lds:
// dh 32) share their online-softmax step and their row store.  What differs in
// bits stays at their call sites: exp2f against the hardware exp2 (FAST), S
// scaled in f32 against Q pre-scaled in f16, and which blocks are masked.
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// Key counts.  Every kernel here exists twice: KV = false is the plain form, all
// of a sentence's rows its keys; KV = true reads keys[b], 1 <= keys[b] <= len,
// the rows of sentence b that are keys and values (a ColBERT query's rows up to
// [SEP]; the [MASK] rows behind them are queries only).  The count bounds the
// mask, the K / V loads and the block loops; the sentence's length bounds the
// query rows, the Q loads and the stores.  A compile-time variant, so the plain
// form's code is what it was before there were counts (key_count:
// device_common.h, shared with f32.hip).
// ---------------------------------------------------------------------------
// an item (sentence, head) of the persistent kernel; the plain form carries no count
template <bool KV> struct AttItem;
template <> struct AttItem<false> {
    int start, len, h;
    __device__ __forceinline__ int keys() const { return len; }
};
template <> struct AttItem<true> {
    int start, len, h, nk;
    __device__ __forceinline__ int keys() const { return nk; }
};

struct RowMaxSum { float m, l; };   // a query's running max and its row sum under that max
template <bool FAST>
__device__ __forceinline__ float ex2(float x)
{
    if constexpr (FAST) return __builtin_amdgcn_exp2f(x);
    else return exp2f(x);
}
// s (masked, in the exp2 domain; mx the max of this lane's 32) -> P; O and the
// returned m, l moved to the new row max.  (m and l go in and out by value and
// l moves before O: through references, or with l updated last, attention<64>
// takes two more VGPRs than with the step written out.)
template <bool FAST, int NT>
__device__ __forceinline__ RowMaxSum running_max_step(f32x16 (&s)[2], float mx, f32x16 (&o)[NT], RowMaxSum ms)
{
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(ms.m, mx);
    const float alpha = ex2<FAST>(ms.m - m_new);
    float rs = 0.f;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = ex2<FAST>(s[kh][r] - m_new);
            s[kh][r] = p;
            rs += p;
        }
    rs += __shfl_xor(rs, 32, 64);
    ms.l = ms.l * alpha + rs;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
    ms.m = m_new;
    return ms;
}
// O / l as f16 into the query's row (8-B stores: lane (q, hi) holds dh 8m + 4 hi .. +3)
template <int NT>
__device__ __forceinline__ void store_row_h16x4(const f32x16 (&o)[NT], float l_i, h16 *orow, int hi)
{
    const float inv = 1.0f / l_i;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            h16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (h16)(o[t][4 * g + e] * inv);
            *(h16x4 *)(orow + 32 * t + 8 * g + 4 * hi) = v;
        }
}

// ---------------------------------------------------------------------------
// attention: flash-style, one workgroup = 128 queries of one (sentence, head),
// 4 waves x 32 queries.  S^T = K Q^T per 32-key block (query on the lane,
// keys in registers) -> online softmax in registers -> O^T += V^T P^T with
// the S accumulator reused as the B operand (no LDS round trip for P).
// Keys past the sentence end get probability exactly 0, as the reference's
// -1e5 mask does after its fp16 exp (bert.cpp:957-961, 1024-1025).
// ---------------------------------------------------------------------------

template <int DH, bool KV>
__global__ __launch_bounds__(256) void attention_kernel(const h16 *__restrict__ qkv, const int32_t *__restrict__ cu,
                                                        int d, int nqt, int nh, float sl2, h16 *__restrict__ out,
                                                        const int32_t *__restrict__ keys)
{
    constexpr int KT = 64, KSTR = DH + 8, VSTR = KT + 8;
    __shared__ __attribute__((aligned(16))) h16 Ks[KT * KSTR];
    __shared__ __attribute__((aligned(16))) h16 Vt[DH * VSTR];
    // XCD-aware order: the query tiles of one (sentence, head) get consecutive
    // logical ids on ONE XCD, so its K/V tiles are fetched into that XCD's L2
    // once instead of once per XCD (dispatch is round-robin over the 8 XCDs).
    const int t = xcd_block(blockIdx.x, gridDim.x);
    const int qt = t % nqt, h = (t / nqt) % nh, b = t / (nqt * nh);
    const int start = cu[b], len = cu[b + 1] - start;
    const int q0 = qt * ATT_QT;
    if (q0 >= len) return;
    const int nk = key_count<KV>(keys, b, len);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int hi = lane >> 5, lq = lane & 31;
    const int ld = 3 * d;
    const int q = q0 + w * 32 + lq;

    h16x8 qf[DH / 16];
    const h16 *qrow = qkv + (size_t)(start + q) * ld + h * DH;
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) qf[s] = *(const h16x8 *)(qrow + 16 * s + 8 * hi);

    f32x16 o[DH / 32];
#pragma unroll
    for (int t = 0; t < DH / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    RowMaxSum ms = {-INFINITY, 0.f};

    const int nkt = (nk + KT - 1) / KT;
    for (int kt = 0; kt < nkt; ++kt) {
        const int k0 = kt * KT;
        __syncthreads();
        // K tile row-major (coalesced: chunk index fastest)
        for (int c = tid; c < KT * DH / 8; c += 256) {
            const int r = c / (DH / 8), ch = c % (DH / 8);
            uint4 kv = {0u, 0u, 0u, 0u};
            if (k0 + r < nk) kv = *(const uint4 *)(qkv + (size_t)(start + k0 + r) * ld + d + h * DH + ch * 8);
            *(uint4 *)(Ks + r * KSTR + ch * 8) = kv;
        }
        // V tile transposed into Vt[d][key] (key fastest across lanes: conflict-free 2-byte writes)
        for (int c = tid; c < KT * DH / 8; c += 256) {
            const int r = c % KT, ch = c / KT;
            // keys past the counted ones: zeros (their P is exactly 0; 0 * garbage could be NaN)
            h16x8 vv = {};
            if (k0 + r < nk) vv = *(const h16x8 *)(qkv + (size_t)(start + k0 + r) * ld + 2 * d + h * DH + ch * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * VSTR + r] = vv[e];
        }
        __syncthreads();

        f32x16 s[2];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kh][r] = 0.f;
#pragma unroll
            for (int st = 0; st < DH / 16; ++st) {
                const h16x8 a = *(const h16x8 *)(Ks + (kh * 32 + lq) * KSTR + 16 * st + 8 * hi);
                s[kh] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[st], s[kh], 0, 0, 0);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + kh * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const float v = key < nk ? s[kh][r] * sl2 : -INFINITY;
                s[kh][r] = v;
                mx = fmaxf(mx, v);
            }
        ms = running_max_step<false>(s, mx, o, ms);

#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                h16x8 bp;
#pragma unroll
                for (int j = 0; j < 8; ++j) bp[j] = (h16)s[kh][8 * s2 + j];
#pragma unroll
                for (int t = 0; t < DH / 32; ++t) {
                    const h16 *vr = Vt + (32 * t + lq) * VSTR + 32 * kh + 16 * s2 + 4 * hi;
                    const h16x4 lo = *(const h16x4 *)vr;
                    const h16x4 up = *(const h16x4 *)(vr + 8);
                    const h16x8 a = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
                    o[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bp, o[t], 0, 0, 0);
                }
            }
        }
    }

    if (q < len) store_row_h16x4(o, ms.l, out + (size_t)(start + q) * d + h * DH, hi);
}

// ---------------------------------------------------------------------------
// attention_lds: one workgroup per (sentence, head), up to 512 keys.  The
// sentence's whole K and V (<= 512 x DH f16 each) are brought into LDS ONCE by
// LDS-DMA; 16 waves x 32 queries then run with no further global loads and no
// barriers.
//   K image: [key][DH] rows, 16-B chunks XOR-swizzled by row_swz(key).k (via the
//            DMA source address), read as ds_read_b128 A fragments of S^T = K Q^T.
//   V image: [key][DH] rows, chunks XOR-swizzled by row_swz(key).v, read with
//            ds_read_b64_tr_b16 as the transposed A fragments of
//            O^T += V^T P^T -- no transposing copy.
// Q is pre-scaled by log2(e)/sqrt(dh) (f16), so S comes out in the exp2 domain;
// keys past the sentence end are masked (only in the last 64-key block).
// ---------------------------------------------------------------------------
template <int DH, bool KV>
__global__ __launch_bounds__(1024) void attention_lds_kernel(const h16 *__restrict__ qkv,
                                                             const int32_t *__restrict__ cu, int d, int nh,
                                                             float sl2, h16 *__restrict__ out,
                                                             const int32_t *__restrict__ keys)
{
    constexpr int RB = DH * 2, CH = RB / 16, LMAX = ATT_LDS_MAX;
    __shared__ __attribute__((aligned(16))) char smem[2 * LMAX * RB];
    char *Kl = smem, *Vl = smem + LMAX * RB;
    const int h = blockIdx.x % nh, b = blockIdx.x / nh;
    const int start = cu[b], len = cu[b + 1] - start;
    if (len <= 0) return;
    const int nk = key_count<KV>(keys, b, len);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int hi = lane >> 5, lq = lane & 31;
    const int ld = 3 * d;
    const int nrows = (nk + 63) & ~63;                    // the counted keys' 64-row blocks

    // ---- K and V of the sentence -> LDS (64 chunks of 16 B per wave-instruction) ----
    {
        const int ninstr = nrows * CH / 64;
        const h16 *kbase = qkv + (size_t)start * ld + d + h * DH;
        const h16 *vbase = kbase + d;
        for (int i = w; i < ninstr; i += 16) {
            const int g = i * 64 + lane, row = g / CH, pc = g % CH;
            const int srow = min(row, nk - 1);           // rows past the end: finite copies, masked / P = 0
            const RowSwz sw = row_swz<CH>(row);
            glds<16>(kbase + (size_t)srow * ld + (pc ^ sw.k) * 8, Kl + i * 1024);
            glds<16>(vbase + (size_t)srow * ld + (pc ^ sw.v) * 8, Vl + i * 1024);
        }
        wait_vmcnt<0>();
        __syncthreads();
    }

    const int q0 = 32 * w;
    if (q0 >= len) return;                                // no barrier follows
    const int q = q0 + lq;
    h16x8 qf[DH / 16];
    {
        const h16 *qrow = qkv + (size_t)(start + min(q, len - 1)) * ld + h * DH;
        const h16 s16 = (h16)sl2;
        const h16x8 sc = {s16, s16, s16, s16, s16, s16, s16, s16};
#pragma unroll
        for (int s = 0; s < DH / 16; ++s) qf[s] = *(const h16x8 *)(qrow + 16 * s + 8 * hi) * sc;
    }
    f32x16 o[DH / 32];
#pragma unroll
    for (int t = 0; t < DH / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    RowMaxSum ms = {-INFINITY, 0.f};

    // tr-read lane roles: group g = lane >> 4 reads rows r0 + (i >> 2), columns c0 + 4 (i & 3)
    const int gi = lane & 15, gq = gi >> 2, gp = gi & 3, gg = lane >> 4;

    for (int kb = 0; kb < nrows; kb += 64) {
        f32x16 s[2];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kh][r] = 0.f;
            const int row = kb + 32 * kh + lq;
            const char *krow = Kl + row * RB;
#pragma unroll
            for (int st = 0; st < DH / 16; ++st) {
                const h16x8 a = *(const h16x8 *)(krow + (((2 * st + hi) ^ row_swz<CH>(row).k) << 4));
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
        float mx = s[0][0];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kh][r]);
        ms = running_max_step<true>(s, mx, o, ms);

#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                h16x8 bp;
#pragma unroll
                for (int j = 0; j < 8; ++j) bp[j] = (h16)s[kh][8 * s2 + j];
                const int r0 = kb + 32 * kh + 16 * s2 + 4 * (gg >> 1) + gq;
#pragma unroll
                for (int t = 0; t < DH / 32; ++t) {
                    const int c0 = 32 * t + 16 * (gg & 1) + 4 * gp;       // column of this lane's 8 bytes
                    const int ch = c0 >> 3;
                    const int rowa = r0, rowb = r0 + 8;
                    const h16x4 lo = lds_read_tr16(Vl + rowa * RB + ((ch ^ row_swz<CH>(rowa).v) << 4) + (c0 & 7) * 2);
                    const h16x4 up = lds_read_tr16(Vl + rowb * RB + ((ch ^ row_swz<CH>(rowb).v) << 4) + (c0 & 7) * 2);
                    const h16x8 a = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
                    o[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bp, o[t], 0, 0, 0);
                }
            }
        }
    }

    if (q < len) store_row_h16x4(o, ms.l, out + (size_t)(start + q) * d + h * DH, hi);
}

// ---------------------------------------------------------------------------
// The dh-64 kernels for sentences of up to 512 tokens: attention_lds3,
// attention_short and attention_pp.  Each brings K and V into the swizzled LDS
// image its own way and runs its queries through AttWave64
// (attention_block.h), so a sentence has the same bits from all three.
// ---------------------------------------------------------------------------

// the lane id from an asm statement the compiler cannot hoist out of a loop
__device__ __forceinline__ int lane_id_opaque()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// LDS-DMA issued from asm: hipcc's waitcnt pass cannot see it, so it no longer
// puts a vmcnt(0) in front of the first LDS read after each issue (which retired
// the next item's region-A prefetch in the first block after B1).  The kernel's
// own waits in front of B1 and S are the only ones; no compiler-visible global
// load may be in flight across the block loop's back edge (its wait there would
// retire the hidden pieces too), and the compiler's waits for its own loads stay
// conservative (hidden younger loads only make its vmcnt(N) stricter).
__device__ __forceinline__ void glds16_hidden(const void *g, const void *lds)
{
    const uint32_t m = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)lds;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(m) : "memory", "m0");
#pragma clang diagnostic pop
}
// every vector-memory op retired: the builtin for the compiler's own loads, the
// asm copy for the hidden pieces
__device__ __forceinline__ void wait_all_vm()
{
    wait_vmcnt<0>();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---------------------------------------------------------------------------
// attention_lds3 (the bitwise reference and A/B form of attention_pp): the
// attention_lds structure (whole K/V of a (sentence, head) in LDS, 16 waves x
// 32 queries), persistent: one workgroup per CU that walks the items
// (sentence, head) it = blockIdx.x, + gridDim.x, ..., so the K/V DMA of the next
// item runs under the current item's MFMAs instead of in front of them (a
// workgroup per item loads every item in the open: about 16 of 84 us at C3 were
// exposed loads).  The K/V image is two regions of 256 keys (A = key blocks
// 0-3, B = blocks 4-7):
//   B1 (every wave past the item's region-A blocks): the next item's region-A
//      K/V pieces are issued;
//   S  (every wave past its region-B blocks; the next item's Q rows loaded in
//      front of it): the item's rows are stored; the next item's region-B
//      pieces are issued once its Q has arrived (the loop top).
// The waits in front of B1 and S retire pieces issued half an item earlier; only
// a workgroup's first item waits for its loads in the open.  Per-phase cycles:
// ATT_STAMPS build, scripts/att_stamps.py.
// ---------------------------------------------------------------------------
template <bool KV>
__global__ __launch_bounds__(1024) void attention_lds3_kernel(const h16 *__restrict__ qkv,
                                                              const int32_t *__restrict__ cu, int d, int nh,
                                                              int n_items, float sl2, h16 *__restrict__ out,
                                                              const int32_t *__restrict__ keys)
{
    constexpr int DH = AttWave64::DH, RB = AttWave64::RB, CH = AttWave64::CH, LMAX = ATT_LDS_MAX, RH = LMAX / 2;
    constexpr int VB = LMAX * RB;                         // the V image behind the K image
    static_assert(RH == 256, "a region is 32 pieces: two per wave");
    __shared__ __attribute__((aligned(16))) char smem[2 * LMAX * RB];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ld = 3 * d;

    using Item = AttItem<KV>;
    auto item = [&](int i) {
        const int b = i / nh;
        Item r;
        r.h = i - b * nh;
        r.start = cu[b];
        r.len = cu[b + 1] - r.start;
        if constexpr (KV) r.nk = keys[b];
        return r;
    };
    // region r (rows 256 r .. 256 r + 255) of `it`: piece i = rows 8i .. 8i + 7;
    // wave w issues pieces 32 r + w and 32 r + w + 16 when they hold rows of the
    // counted keys' 64-row blocks; rows past the end are finite copies (masked / P = 0).
    auto issue = [&](const Item &it, int r) {
        const int lane = lane_id_opaque();                // recomputed here: hoisted, its
        const int nrows = (it.keys() + 63) & ~63;         // derivatives spill around the block loop
        const h16 *kbase = qkv + (size_t)it.start * ld + d + it.h * DH;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = 32 * r + w + 16 * j;
            if (8 * i < nrows) {
                const int row = 8 * i + (lane >> 3), pc = lane & 7;
                const size_t so = (size_t)min(row, it.keys() - 1) * ld;
                const RowSwz sw = row_swz<CH>(row);
                glds16_hidden(kbase + so + (pc ^ sw.k) * 8, smem + i * 1024);
                glds16_hidden(kbase + d + so + (pc ^ sw.v) * 8, smem + VB + i * 1024);
            }
        }
    };
    AttWave64 a;
    a.init(lane, smem, 0);
    auto load_q = [&](const Item &it) {                   // raw rows; scaled at the item's start
        if (it.len <= 0) return;
        const int lane = lane_id_opaque(), hi = lane >> 5, lq = lane & 31;
        const h16 *qrow = qkv + (size_t)(it.start + min(32 * w + lq, it.len - 1)) * ld + it.h * DH;
#pragma unroll
        for (int s = 0; s < DH / 16; ++s) a.qf[s] = *(const h16x8 *)(qrow + 16 * s + 8 * hi);
    };

    int cur_i = blockIdx.x;
    if (cur_i >= n_items) return;                         // workgroup-uniform
    Item cur = item(cur_i);
    // the first item: Q and region A in the open; region B (issued at the loop
    // top) under region A's blocks, retired by B1's wait as in every later item
    load_q(cur);
    issue(cur, 0);
    wait_all_vm();
    __syncthreads();
    ASTAMP_ITEMS(nit);   // (stamps builds only, diag_att_stamps.h)
    for (;;) {
        ASTAMP(0, __builtin_amdgcn_s_memtime());
        const int nx_i = cur_i + (int)gridDim.x;
        const bool more = nx_i < n_items;                 // workgroup-uniform
        Item nx = {};
        if (more) nx = item(nx_i);
        a.nk = cur.keys();
        a.rows = cur.len;
        const int nrows = (a.nk + 63) & ~63;
        const bool active = 32 * w < a.rows;              // wave-uniform
        a.scale_q(sl2);
        // the item's region B, issued after the first use of Q (the compiler's
        // wait for the Q loads retires every older piece); the empty asm keeps
        // the issue below that wait
        asm volatile("" ::"v"(a.qf[0]), "v"(a.qf[1]), "v"(a.qf[2]), "v"(a.qf[3]));
        issue(cur, 1);
        a.clear();                                        // unconditional: no block state stays live across items
        __builtin_amdgcn_s_setprio(3);                    // block 0: see the block loop
        if (active) a.block0(0, VB);
        ASTAMP(1, __builtin_amdgcn_s_memtime());
        // blocks 1-7 in one loop (one inlined copy of the block code), B1 at the
        // region boundary
#pragma clang loop unroll(disable)
        for (int kb = 64; kb < LMAX; kb += 64) {
            if (kb == RH) {
                ASTAMP(2, __builtin_amdgcn_s_memtime());
                wait_all_vm();                            // this item's region-B pieces
                __syncthreads();                          // B1: region A is free
                ASTAMP(3, __builtin_amdgcn_s_memtime());
                if (more) issue(nx, 0);
            }
            // progress-based priority: the further a wave is past the last
            // barrier, the lower its priority, so the 4 waves of a SIMD reach the
            // next barrier together instead of in age order (the oldest wave of a
            // SIMD ran its 4 blocks 2x faster than the youngest and then waited
            // for it; 69.5 -> 65.8 us at C3, profiles/r02_att_stamps_prio.log)
            switch ((kb >> 6) & 3) {
            case 0: __builtin_amdgcn_s_setprio(3); break;
            case 1: __builtin_amdgcn_s_setprio(2); break;
            case 2: __builtin_amdgcn_s_setprio(1); break;
            default: __builtin_amdgcn_s_setprio(0); break;
            }
            if (active && kb < nrows) a.block(kb, kb * RB, kb * RB + VB);
        }
        ASTAMP(4, __builtin_amdgcn_s_memtime());
        // The item's rows are stored after the S barrier (storing them before S,
        // so a wave that finishes early writes while the slower ones still
        // compute, measured 2 us slower: the early stores queue in front of the
        // next item's region-A pieces, profiles/r03_attention_store_ab.log), on
        // every lane of an active wave.  The wait in front of S is exact: the
        // next item's Q (4 loads) stays in flight, every older piece (the next
        // item's region A) is retired.
        if (more) load_q(nx);
        static_assert(DH / 16 == 4, "four Q loads per wave");
        if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // the 4 Q loads younger
        else wait_all_vm();
        ASTAMP(5, __builtin_amdgcn_s_memtime());
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // no LDS read in flight into the store phase
        __syncthreads();                                  // S: region B is free
        if (active) a.store(out, cur.start, d, cur.h, 32 * w + (lane & 31));
        ASTAMP(6, __builtin_amdgcn_s_memtime());
        ASTAMP_ITEM_END(nit);
        if (!more) break;
        cur = nx;
        cur_i = nx_i;
    }
}

// ---------------------------------------------------------------------------
// Short sentences (max_len <= 64, the serving shape: examples/server.cpp:114 ->
// one text per bert_encode): one 2-wave workgroup per (sentence, head), the
// item's one 64-key block.  attention_lds3 runs such an item on 16 waves of which
// one or two have queries, through its region DMA and its B1 and S barriers;
// here the K/V rows are plain 16-B loads into the same swizzled LDS image and
// the block is AttWave64's block 0, so a sentence gets the same bits from either
// kernel (batch-composition invariance: a short sentence alone takes this
// kernel, inside a longer batch attention_pp).
// ---------------------------------------------------------------------------
template <bool KV>
__global__ __launch_bounds__(128) void attention_short_kernel(const h16 *__restrict__ qkv,
                                                              const int32_t *__restrict__ cu, int d, int nh,
                                                              float sl2, h16 *__restrict__ out,
                                                              const int32_t *__restrict__ keys)
{
    constexpr int DH = AttWave64::DH, RB = AttWave64::RB, CH = AttWave64::CH, NK = 64, VB = NK * RB;
    __shared__ __attribute__((aligned(16))) char smem[2 * NK * RB];
    const int it = blockIdx.x, b = it / nh, h = it - b * nh;
    const int start = cu[b], len = cu[b + 1] - start;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int hi = lane >> 5, lq = lane & 31;
    const int ld = 3 * d;
    if (len <= 0) return;                                 // workgroup-uniform
    const int nk = key_count<KV>(keys, b, len);
    AttWave64 a;
    a.init(lane, smem, 0);
    a.nk = nk;
    a.rows = len;
    // the wave's Q rows first: their loads fly with the K / V loads below
    {
        const h16 *qrow = qkv + (size_t)(start + min(32 * w + lq, len - 1)) * ld + h * DH;
#pragma unroll
        for (int st = 0; st < DH / 16; ++st) a.qf[st] = *(const h16x8 *)(qrow + 16 * st + 8 * hi);
    }
    // K / V rows 0-63 (rows past the end: finite copies of the last row, masked / P = 0)
    const h16 *kbase = qkv + (size_t)start * ld + d + h * DH;
#pragma unroll
    for (int k = 0; k < NK * 8 / 128; ++k) {
        const int c = tid + 128 * k, r = c >> 3, j = c & 7;
        const size_t so = (size_t)min(r, nk - 1) * ld + 8 * j;
        const uint4 kv = *(const uint4 *)(kbase + so);
        const uint4 vv = *(const uint4 *)(kbase + d + so);
        const RowSwz sw = row_swz<CH>(r);
        *(uint4 *)(smem + r * RB + ((j ^ sw.k) << 4)) = kv;
        *(uint4 *)(smem + VB + r * RB + ((j ^ sw.v) << 4)) = vv;
    }
    __syncthreads();
    if (32 * w >= len) return;                            // wave-uniform: no queries
    a.scale_q(sl2);
    a.clear();
    a.block0(0, VB);
    a.store(out, start, d, h, 32 * w + lq);
}

// ---------------------------------------------------------------------------
// attention_pp (production for 64 < L <= 512, dh 64; round 6): lds3's per-query
// arithmetic in two co-resident 8-wave workgroups per CU instead of one 16-wave
// workgroup, so one workgroup's per-unit phases (Q in, block 0, the row stores)
// run beside the other's steady blocks instead of stalling the whole CU.  A unit is
// half an item: 256 queries (8 waves x 32, wave w of half qh = lds3's wave
// 8 qh + w) over all of the sentence's keys; K and V stream through a 4-stage
// LDS ring of 64-key blocks (16 KiB a stage: 64 KiB per workgroup, two per CU),
// each wave issuing one K and one V piece per block, NS - 1 blocks ahead; a
// barrier per block publishes block j and frees block j - 1's stage.  The two
// halves of an item are consecutive units on one XCD, so the second reads K/V
// from that L2.  Every query runs AttWave64's block sequence on lds3's wave
// composition, so the output has lds3's bits (the kernel tests compare them).
// (Round 6 also measured, all bitwise equal and slower: four 4-wave workgroups
// per CU with a 2-stage ring, a barrier per block pair, and a persistent form
// whose ring runs on across units; profiles/r06_attention_pp_ab.log.  A priority
// split between the co-resident workgroups: no effect, r06_attention_pp_prio_ab.log.)
template <bool KV>
__global__ __launch_bounds__(512, 4) void attention_pp_kernel(const h16 *__restrict__ qkv,
                                                              const int32_t *__restrict__ cu, int d, int nh,
                                                              float sl2, h16 *__restrict__ out,
                                                              const int32_t *__restrict__ keys)
{
    constexpr int NW = 8, NS = 4, DH = AttWave64::DH, RB = AttWave64::RB, CH = AttWave64::CH;
    constexpr int SB = 2 * 64 * RB, VO = 64 * RB;         // a stage: 64 K rows, then 64 V rows
    constexpr int UPI = 16 / NW, PW = 16 / NW;            // units per item, pieces per wave and block
    __shared__ __attribute__((aligned(16))) char smem[NS * SB];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, lq = lane & 31;
    const int ld = 3 * d;
    // XCD-aware remap: each XCD a contiguous run of units, so an item's two
    // halves share its L2
    const int u = xcd_block(blockIdx.x, gridDim.x);
    const int it = u / UPI, q0 = 32 * NW * (u - it * UPI);
    const int b = it / nh, h = it - b * nh;
    const int start = cu[b], len = cu[b + 1] - start;
    if (q0 >= len) return;                                // workgroup-uniform: no queries
    const int nk = key_count<KV>(keys, b, len);
    const int nblk = (nk + 63) >> 6;                      // the ring runs over the counted keys' blocks
    const bool active = q0 + 32 * w < len;                // wave-uniform
    const h16 *kbase = qkv + (size_t)start * ld + d + h * DH;
    PST_DECL;   // (stamps builds only, diag_att_stamps.h)
    PST_SET(0, PST_NOW());

    // block j's K and V rows into stage j % NS: piece i < 8 is K rows 8i .. 8i + 7
    // of the block, 8 + i the same V rows (the row's swizzle within the block
    // being its swizzle in the sentence); wave w issues pieces w, w + NW, ...;
    // rows past the end are finite copies (masked / P = 0)
    auto issue = [&](int j) {
        const int ln = lane_id_opaque();
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            const int i = w + NW * k, r8 = i & 7;
            const int row = 64 * j + 8 * r8 + (ln >> 3), pc = ln & 7;
            const size_t so = (size_t)min(row, nk - 1) * ld;
            char *dst = smem + (j % NS) * SB + i * 1024;
            const RowSwz sw = row_swz<CH>(row);
            if (i < 8) glds16_hidden(kbase + so + (pc ^ sw.k) * 8, dst);
            else glds16_hidden(kbase + d + so + (pc ^ sw.v) * 8, dst);
        }
    };
    // the wave's Q rows by asm loads (hipcc's waitcnt pass does not see them, so it
    // puts no vmcnt(0) at their first use, which would retire every prologue
    // piece); then blocks 0-2 (always three: a block past the sentence is a
    // clamped copy into a stage no block reads), so block 0's wait below has one
    // constant count and is one asm tied to the Q registers (a wait per branch
    // let hipcc copy the registers in front of it, before the loads landed)
    AttWave64 a;
    {
        const h16 *qrow = qkv + (size_t)(start + min(q0 + 32 * w + lq, len - 1)) * ld + h * DH;
#pragma unroll
        for (int st = 0; st < DH / 16; ++st)
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(a.qf[st]) : "v"(qrow + 16 * st + 8 * hi) : "memory");
    }
#pragma unroll
    for (int j = 0; j < NS - 1; ++j) issue(j);

    a.init(lane, smem, VO);                               // k_base = v_base = the block's stage
    a.nk = nk;
    a.rows = len;
    a.clear();
    // block j: this wave's pieces of it retired (blocks j + 1 .. j + NS - 2 may
    // fly), then the barrier publishes every wave's and frees block j - 1's stage,
    // then block j + NS - 1 is issued into that stage
    auto enter = [&](int j) {
        const int younger = min(NS - 2, nblk - 1 - j);   // blocks in flight behind block j
        if (j == 0) {   // the Q loads and block 0 (the oldest); blocks 1 .. NS - 2 may fly
            asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a.qf[0]), "+v"(a.qf[1]), "+v"(a.qf[2]), "+v"(a.qf[3])
                         : "i"(PW * (NS - 2)) : "memory");
        } else if (younger >= 2) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PW * 2) : "memory");
        } else if (younger == 1) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PW) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if (j + NS - 1 < nblk) issue(j + NS - 1);
    };
    enter(0);
    PST_SET(1, PST_NOW());
    a.scale_q(sl2);
    if (active) a.block0(0, 0);
    PST_SET(2, PST_NOW());
#pragma clang loop unroll(disable)
    for (int j = 1; j < nblk; ++j) {
        PST_MARK();
        enter(j);
        PST_ADDW();
        PST_MARK();
        if (active) {
            const int sbase = (j % NS) * SB;
            a.block(64 * j, sbase, sbase);
        }
        PST_ADDC();
    }
    PST_SUMS();
    PST_SET(5, PST_NOW());
    // (short sentences: the clamped prologue copies may still fly; none may land
    // after the workgroup is gone)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!active) return;
    // (the lane's query from lane_id_opaque: lq kept live across the block loop
    // for this alone spills at the 128-VGPR boundary, as in lds3's issue)
    a.store(out, start, d, h, q0 + 32 * w + (lane_id_opaque() & 31));
    PST_SET(6, PST_NOW());
    PST_HWID();
}

thread_local int g_att_variant = 0;   // benches only (bertx_bench_attention), per calling thread
thread_local int g_att_ran = -1;      // the AttKernel of the calling thread's last launch_attention

// an A/B switch of the environment: on unless set to a value starting with 0
static bool env_on(const char *name)
{
    const char *e = std::getenv(name);
    return !(e && *e == '0');
}

// The kernel of a launch.  Up to ATT_LDS_MAX tokens at dh 64: variant 0 is
// production -- attention_short for max_len <= 64 (one 2-wave workgroup per
// item), else attention_pp (two 8-wave workgroups per CU, half an item each:
// 66.2-67.1 vs lds3 67.5-68.2 us at C3, profiles/r06_attention_pp_ab.log);
// variants 7 and 8 run attention_lds3 (tests, A/B; 7 on at most 7 workgroups:
// many ragged items each), as BERT_ATT_PP=0 does; BERT_ATT_SHORT=0 takes short
// batches off attention_short.  All three give the same bits.
enum class AttKernel { Short, PP, LDS3, LDS_DH32, Streaming };
static AttKernel choose_attention(int dh, int max_len, int variant)
{
    if (max_len > ATT_LDS_MAX || (dh != 64 && dh != 32)) return AttKernel::Streaming;
    if (dh == 32) return AttKernel::LDS_DH32;
    if (variant == 7 || variant == 8) return AttKernel::LDS3;
    if (max_len <= 64) {
        static const bool short_env = env_on("BERT_ATT_SHORT");
        if (short_env) return AttKernel::Short;
    }
    static const bool pp_env = env_on("BERT_ATT_PP");
    return pp_env ? AttKernel::PP : AttKernel::LDS3;
}

// One launch, plain (KV = false, keys unused) or with key counts
template <bool KV>
static void launch_attention_as(AttKernel kernel, const h16 *qkv, const int32_t *cu, const int32_t *keys, int n_items,
                                int max_len, int n_head, int d, int dh, float sl2, h16 *out, hipStream_t s)
{
    switch (kernel) {
    case AttKernel::Short:
        if (n_items > 0) attention_short_kernel<KV><<<n_items, 128, 0, s>>>(qkv, cu, d, n_head, sl2, out, keys);
        break;
    case AttKernel::PP:
        if (n_items > 0) attention_pp_kernel<KV><<<2 * n_items, 512, 0, s>>>(qkv, cu, d, n_head, sl2, out, keys);
        break;
    case AttKernel::LDS3: {   // persistent: one workgroup per CU
        const int grid = std::min(n_items, g_att_variant == 7 ? 7 : device_cu_count());
        if (grid > 0) attention_lds3_kernel<KV><<<grid, 1024, 0, s>>>(qkv, cu, d, n_head, n_items, sl2, out, keys);
        break;
    }
    case AttKernel::LDS_DH32:
        attention_lds_kernel<32, KV><<<n_items, 1024, 0, s>>>(qkv, cu, d, n_head, sl2, out, keys);
        break;
    case AttKernel::Streaming: {
        const int nqt = (max_len + ATT_QT - 1) / ATT_QT;
        const int grid = nqt * n_items;
        if (dh == 64) attention_kernel<64, KV><<<grid, 256, 0, s>>>(qkv, cu, d, nqt, n_head, sl2, out, keys);
        else attention_kernel<32, KV><<<grid, 256, 0, s>>>(qkv, cu, d, nqt, n_head, sl2, out, keys);
        break;
    }
    }
}

void launch_attention(const uint16_t *qkv_, const int32_t *cu, int32_t n_seqs, int32_t max_len, int32_t n_head,
                      int32_t d, uint16_t *out_, hipStream_t s, const int32_t *keys)
{
    const int dh = d / n_head, n_items = n_seqs * n_head;
    const float sl2 = (1.0f / sqrtf((float)dh)) * 1.4426950408889634f;
    const h16 *qkv = (const h16 *)qkv_;
    h16 *out = (h16 *)out_;
    // (the kernel is chosen by the sentences' lengths, with or without counts)
    const AttKernel kernel = choose_attention(dh, max_len, g_att_variant);
    g_att_ran = (int)kernel;
    if (keys) launch_attention_as<true>(kernel, qkv, cu, keys, n_items, max_len, n_head, d, dh, sl2, out, s);
    else launch_attention_as<false>(kernel, qkv, cu, nullptr, n_items, max_len, n_head, d, dh, sl2, out, s);
}

}  // namespace emb
