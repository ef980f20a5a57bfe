// Fused top-k search over a device-resident f16 embedding index (bertx_index_*,
// bert_hip.h).  One streaming pass over the stored rows:
// the scores of up to 64 queries are taken on v_mfma_f32_16x16x32_f16 straight from
// the rows' HBM image (fragment order, below) and the k best of a workgroup's row
// range are kept in LDS, so no [B][N] score matrix ever exists.  A second small
// kernel merges the workgroups' lists.
//
// Stored layout ("fragment order", the A operand of the MFMA as it sits in HBM):
// rows in groups of 16, a group's d / 32 blocks consecutive, a block = 16 rows x
// 32 k = 1 KiB; lane 16g + f of a block holds row f, elements 8g .. 8g + 7 (16 B).
// One global_load_dwordx4 per wave is one contiguous block and goes to the MFMA
// without touching LDS.
//
// Arithmetic of one (query, row) score: both operands f16 (round to nearest even),
// the d / 32 MFMAs of the row's group in ascending k into an f32 accumulator that
// starts at 0.  Every tile of every launch runs that same sequence, so a score
// depends on neither the row's position, the row count nor the other queries.
//
// int8 storage (BERTX_INDEX_I8) is the same kernel over another Store:
// "i8 fragment order" is the A operand of v_mfma_i32_16x16x64_i8, a block = 16 rows x
// 64 k = 1 KiB, lane 16g + f = row f, bytes 16g .. 16g + 15, a group's d / 64 blocks
// consecutive, and one f32 scale per row in a second buffer.  quantize_row_i8 is the
// one quantizer of stored rows and queries; a score is the exact i32 sum of the byte
// products times the two scales (score_i8), so it is order-free as well.
#include "device_common.h"
#include "kernels.h"
#include "quant_i8.h"
#include "topk_list.h"

#include <algorithm>

namespace emb {
namespace {

constexpr int kThreads = 256;          // 4 waves: each streams its own contiguous run of 16-row groups
constexpr int kUnitsAhead = 8;         // prefetch ring: 8 units of 2 blocks = 16 KiB in flight per wave
constexpr int kRingBlocks = 2 * kUnitsAhead;   // int8: 16 units of 1 block
constexpr int kLdsBudget = 160 * 1024; // LDS of one CU (a single workgroup may use all of it)

// What differs between the storage kinds: the 16-B lane fragment of a 1-KiB block, the
// k a block covers, the accumulator, the blocks of one ring unit (a group's block count
// is a multiple of it: d / 32 is even, d / 64 may be odd and may be 1) and the bytes a
// query takes in LDS.
template <int ST> struct Store;
template <> struct Store<SEARCH_F16> {
    typedef h16x8 Block;
    typedef f32x4 Acc;
    static constexpr int kShift = 5, kUnit = 2;
    __host__ __device__ static constexpr size_t query_bytes(int d) { return (size_t)d * 2; }
};
template <> struct Store<SEARCH_I8> {
    typedef i32x4 Block;
    typedef i32x4 Acc;
    static constexpr int kShift = 6, kUnit = 1;
    __host__ __device__ static constexpr size_t query_bytes(int d) { return (size_t)d + 4; }   // bytes + the scale
};

__device__ __forceinline__ f32x4 mma(h16x8 a, h16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ i32x4 mma(i32x4 a, i32x4 b, i32x4 c)
{
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}

// LDS of the search kernel for QT query tiles (16 queries each): the queries' B
// fragments, the running lists, the score tile of one step, the step's group ids.
template <int ST>
__host__ __device__ inline size_t search_lds_bytes(int QT, int d, int k)
{
    return (size_t)QT * 16 * (Store<ST>::query_bytes(d) + (size_t)k * 8 + 64 * 4) + 16;
}
inline size_t search_lds_bytes(int storage, int QT, int d, int k)
{
    return storage == SEARCH_I8 ? search_lds_bytes<SEARCH_I8>(QT, d, k) : search_lds_bytes<SEARCH_F16>(QT, d, k);
}

// Workgroup b walks the 16-row groups [b * per, (b + 1) * per), per % 4 == 0: wave w
// streams the contiguous quarter w of them, one group per step.  After a group's
// d / 32 blocks the wave's 16 x (16 QT) scores go to the LDS score tile; then wave w
// offers the step's 64 rows to the lists of queries w, w + 4, ... (one lane per row).
// Rows >= n_rows (the unfilled part of the last group, and the groups a range has
// past the end) are never offered.  partial: [query][P][k].
// int8: row_scale f32 [rows]; a row's scale is read only for rows < n_rows, one group
// ahead of its use, and the group's i32 sums become scores (score_i8) on their way to
// the score tile.  f16: row_scale is not used.
// Mask: nothing, the unmasked kernel, whose arguments end at row_scale; or one SearchMask,
// the masked kernel, which offers a row only when its tombstone is 0 and its
// bit in the query's filter is 1.  The tombstones and a shared filter are wave-uniform words:
// like the int8 scales they come through the scalar cache a group ahead of their use and
// stay out of the counter that paces the ring.  Per-query filters are one vector load per
// lane and step: lane 16h + i holds the word of query w + 4i for the rows of quarter h.
// Every word index is clamped to the words that cover rows < n_rows.
template <int QT, int ST, class... Mask>
__global__ __launch_bounds__(kThreads) void search_kernel(const typename Store<ST>::Block *__restrict__ corpus,
                                                          const float *__restrict__ queries, int nq, int d,
                                                          int n_rows, int k, int per, Hit *__restrict__ partial,
                                                          const float *__restrict__ row_scale, Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    typedef Store<ST> S;
    typedef typename S::Block Block;
    typedef typename S::Acc Acc;
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int KB = d >> S::kShift, nq16 = QT * 16;
    Block *qf = (Block *)smem;                                  // [QT][KB][64]
    Hit *lists = (Hit *)(qf + (size_t)QT * KB * 64);            // [nq16][k]
    float *tile = (float *)(lists + (size_t)nq16 * k);          // [nq16][64]
    int *gb = (int *)(tile + nq16 * 64);                        // [4]
    float *qscale = (float *)(gb + 4);                          // int8: [nq16]

    if constexpr (ST == SEARCH_F16) {
        // the queries as f16 B fragments: lane 16g + c of block (t, kb) holds query
        // 16t + c, elements 32kb + 8g .. + 7; queries past nq are zeros
        const int chunks = d >> 3;
        for (int i = tid; i < nq16 * chunks; i += kThreads) {
            const int q = i / chunks, c = i - q * chunks;
            h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (q < nq) {
                const float4 a = *(const float4 *)(queries + (size_t)q * d + 8 * c);
                const float4 b = *(const float4 *)(queries + (size_t)q * d + 8 * c + 4);
                v = h16x8{(h16)a.x, (h16)a.y, (h16)a.z, (h16)a.w, (h16)b.x, (h16)b.y, (h16)b.z, (h16)b.w};
            }
            qf[((size_t)(q >> 4) * KB + (c >> 2)) * 64 + 16 * (c & 3) + (q & 15)] = v;
        }
    } else {
        // the queries quantized as the rows are, one wave per query: lane 16g + c of
        // block (t, kb) holds query 16t + c, bytes 64kb + 16g .. + 15, the same byte -> k
        // map as a stored block; queries past nq are zeros with scale 0
        for (int q = w; q < nq16; q += 4) {
            float sc = 0.f;
            i32x4 v = {0, 0, 0, 0};
            if (q < nq) v = quantize_row_i8(queries + (size_t)q * d, d, lane, sc);
            if (lane < (d >> 4)) qf[((size_t)(q >> 4) * KB + (lane >> 2)) * 64 + 16 * (lane & 3) + (q & 15)] = v;
            if (lane == 0) qscale[q] = sc;
        }
    }
    for (int i = tid; i < nq16 * k; i += kThreads) lists[i] = Hit{-INFINITY, -1};
    lds_barrier();

    // wave-uniform stream position in scalar registers: block index -> one base
    // address per load, the lane's 16 B at base + 16 lane
    const int ws = __builtin_amdgcn_readfirstlane(w);
    const int steps = per >> 2;
    const int g0 = blockIdx.x * per + ws * steps;                 // this wave's first group
    const int last_blk = max((n_rows + 15) >> 4, 1) * KB - 1;     // loads stay inside the filled groups
    const int blk0 = g0 * KB;
    constexpr int UB = S::kUnit, NU = kRingBlocks / UB;           // blocks per unit, units in the ring
    const int U = steps * (UB == 2 ? KB >> 1 : KB);               // units; the same for all waves
    auto load = [&](int blk) { return (corpus + (size_t)min(blk, last_blk) * 64)[lane]; };
    // int8: the scales of group grp's 16 rows, zeros for rows >= n_rows.  The address is
    // wave-uniform and the scales do not change during a search, so they come through
    // the scalar cache (constant address space) and never enter the vector-memory
    // counter that paces the ring.
    typedef const __attribute__((address_space(4))) float *ScalePtr;
    const ScalePtr scale_c = (ScalePtr)(uintptr_t)row_scale;
    auto load_scales = [&](int grp, float (&o)[16]) {
        const int64_t r0 = (int64_t)grp * 16;
        if (r0 + 16 <= n_rows) {
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] = scale_c[r0 + i];
        } else {
            // the index's last, partly filled group (once per launch) and the groups
            // past it: one lane per row, then broadcast
            float v = 0.f;
            if (r0 + (lane & 15) < n_rows) v = row_scale[r0 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
        }
    };
    // masked: the admissible words (tombstone 0 and shared filter 1) of the 32 rows around the
    // four groups of the step in which this wave streams group grp: wave h is (h - w) * steps
    // groups away, the waves walk in step.  Wave-uniform addresses, as the scales.
    typedef const __attribute__((address_space(4))) uint32_t *WordPtr;
    const int last_word = max((n_rows + 31) >> 5, 1) - 1;
    const bool per_query = MK && m.filt && m.stride != 0;
    auto load_admissible = [&](int grp, uint32_t (&o)[4]) {
        const WordPtr tomb_c = (WordPtr)(uintptr_t)m.tomb, filt_c = (WordPtr)(uintptr_t)m.filt;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int word = min((grp + (h - ws) * steps) >> 1, last_word);
            o[h] = ~tomb_c[word];
            if (m.filt && !per_query) o[h] &= filt_c[word];
        }
    };

    // the ring is filled and refilled in the order it is consumed (the scheduling
    // barriers keep the compiler from reordering the loads), so a unit's loads
    // are always the oldest ones outstanding
    Block ring[NU][UB];
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        ring[j][0] = load(blk0 + UB * j);
        if constexpr (UB == 2) ring[j][1] = load(blk0 + UB * j + 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    int hmask[4];                                                 // int8: all ones where lane >> 4 == h
#pragma unroll
    for (int h = 0; h < 4; ++h) hmask[h] = -(int)((lane >> 4) == h);
    float rs[16] = {};                                            // int8: the scales of group g, loaded a group ahead
    if constexpr (ST == SEARCH_I8) {
        if (U > 0) load_scales(g0, rs);
    }
    uint32_t adm[4] = {};                                         // masked: the admissible words of this step's groups
    if constexpr (MK) {
        if (U > 0) load_admissible(g0, adm);
    }
    Acc acc[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) acc[t] = Acc{0, 0, 0, 0};
    int kb = 0, g = g0;
    const int nqv = min(nq, nq16);
    for (int u0 = 0; u0 < U; u0 += NU) {
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int u = u0 + j;
            if (u >= U) goto done;   // uniform over the workgroup; no path re-enters the ring out of order
            {
                const Block a0 = ring[j][0], a1 = ring[j][UB - 1];
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    const Block b0 = qf[((size_t)t * KB + kb) * 64 + lane];
                    if constexpr (UB == 2) {
                        const Block b1 = qf[((size_t)t * KB + kb + 1) * 64 + lane];
                        acc[t] = mma(a0, b0, acc[t]);
                        acc[t] = mma(a1, b1, acc[t]);
                    } else {
                        acc[t] = mma(a0, b0, acc[t]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                ring[j][0] = load(blk0 + UB * (u + NU));
                if constexpr (UB == 2) ring[j][1] = load(blk0 + UB * (u + NU) + 1);
                __builtin_amdgcn_sched_barrier(0);
                kb += UB;
                if (kb == KB) {
                    // accumulator register r of lane l: row 4 (l >> 4) + r of the group, query l & 15 of tile t.
                    // int8: this lane's four row scales out of the group's 16 uniform ones, by bit
                    // masks (selects here compiled to exec-mask branches)
                    float rrow[4] = {};
                    if constexpr (ST == SEARCH_I8) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            int b = 0;
#pragma unroll
                            for (int h = 0; h < 4; ++h) b |= __float_as_int(rs[4 * h + r]) & hmask[h];
                            rrow[r] = __int_as_float(b);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        f32x4 sc;
                        if constexpr (ST == SEARCH_F16) {
                            sc = acc[t];
                        } else {
                            const float qs = qscale[16 * t + (lane & 15)];
#pragma unroll
                            for (int r = 0; r < 4; ++r) sc[r] = score_i8(acc[t][r], qs, rrow[r]);
                        }
                        *(f32x4 *)&tile[(16 * t + (lane & 15)) * 64 + 16 * w + 4 * (lane >> 4)] = sc;
                        acc[t] = Acc{0, 0, 0, 0};
                    }
                    if constexpr (ST == SEARCH_I8) load_scales(g + 1, rs);
                    if (lane == 0) gb[w] = g;
                    lds_barrier();
                    const int64_t row = (int64_t)gb[lane >> 4] * 16 + (lane & 15);
                    bool valid = row < n_rows;
                    if constexpr (!MK) {
                        for (int q = w; q < nqv; q += 4)
                            list_offer(lists + (size_t)q * k, k, tile[q * 64 + lane], (int32_t)row, valid, lane);
                    } else {
                        // this lane's quarter's word, by bit masks as the scales above
                        uint32_t word = 0;
#pragma unroll
                        for (int h = 0; h < 4; ++h) word |= adm[h] & (uint32_t)hmask[h];
                        valid = valid && ((word >> (row & 31)) & 1u);
                        load_admissible(g + 1, adm);
                        uint32_t fq = 0;                          // per-query filters: query w + 4 (lane & 15)'s word of this lane's quarter
                        if (per_query && w + 4 * (lane & 15) < nqv)
                            fq = m.filt[(size_t)(w + 4 * (lane & 15)) * m.stride + min((int)(row >> 5), last_word)];
                        if (!per_query) {   // uniform: the loop without the shuffle is the unmasked kernel's
                            for (int q = w; q < nqv; q += 4)
                                list_offer(lists + (size_t)q * k, k, tile[q * 64 + lane], (int32_t)row, valid, lane);
                        } else {
                            for (int q = w, i = 0; q < nqv; q += 4, ++i) {
                                // (the shuffle by every lane, before any lane-dependent condition)
                                const uint32_t fw = (uint32_t)__shfl((int)fq, (lane & 48) | i, 64);
                                const bool ok = valid & (bool)((fw >> (row & 31)) & 1u);
                                list_offer(lists + (size_t)q * k, k, tile[q * 64 + lane], (int32_t)row, ok, lane);
                            }
                        }
                    }
                    lds_barrier();
                    kb = 0;
                    ++g;
                }
            }
        }
    }
done:
    const int P = gridDim.x;
    for (int i = tid; i < nqv * k; i += kThreads) {
        const int q = i / k, j = i - q * k;
        partial[((size_t)q * P + blockIdx.x) * k + j] = lists[i];
    }
}

// One workgroup per query: wave w folds the partial lists w, w + 4, ... into its own
// LDS list (the next list's entries are loaded while the current one is offered),
// wave 0 then folds the other three waves' lists into its own and writes the result.
__global__ __launch_bounds__(kThreads) void search_merge_kernel(const Hit *__restrict__ partial, int P, int k,
                                                                float *__restrict__ scores,
                                                                int32_t *__restrict__ ids)
{
    __shared__ Hit lists[4][128];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = blockIdx.x;
    Hit *mine = lists[w];
    for (int j = lane; j < 128; j += 64) mine[j] = Hit{-INFINITY, -1};
    const Hit *src = partial + (size_t)q * P * k;
    const Hit none{-INFINITY, -1};
    Hit n0 = none, n1 = none;
    if (w < P) {
        if (lane < k) n0 = src[(size_t)w * k + lane];
        if (lane + 64 < k) n1 = src[(size_t)w * k + lane + 64];
    }
    for (int p = w; p < P; p += 4) {
        const Hit e0 = n0, e1 = n1;
        n0 = none; n1 = none;
        if (p + 4 < P) {
            if (lane < k) n0 = src[(size_t)(p + 4) * k + lane];
            if (lane + 64 < k) n1 = src[(size_t)(p + 4) * k + lane + 64];
        }
        list_offer(mine, k, e0.s, e0.id, lane < k && e0.id >= 0, lane);
        list_offer(mine, k, e1.s, e1.id, lane + 64 < k && e1.id >= 0, lane);
    }
    lds_barrier();
    if (w == 0) {
        for (int o = 1; o < 4; ++o) {
            const Hit e0 = lists[o][lane], e1 = lists[o][lane + 64];
            list_offer(mine, k, e0.s, e0.id, lane < k && e0.id >= 0, lane);
            list_offer(mine, k, e1.s, e1.id, lane + 64 < k && e1.id >= 0, lane);
        }
        for (int j = lane; j < k; j += 64) {
            const Hit e = mine[j];
            scores[(size_t)q * k + j] = e.s;
            ids[(size_t)q * k + j] = e.id;
        }
    }
}

// rows f32 [n][d] -> f16 (round to nearest even) into fragment order at rows
// first .. first + n - 1; one thread per 8 elements (one 16-B store).
__global__ __launch_bounds__(kThreads) void index_add_kernel(const float *__restrict__ rows, int64_t n, int d,
                                                             int64_t first, h16x8 *__restrict__ corpus)
{
    const int chunks = d >> 3, KB = d >> 5;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n * chunks) return;
    const int64_t r = i / chunks;
    const int c = (int)(i - r * chunks);
    const float4 a = *(const float4 *)(rows + r * d + 8 * c);
    const float4 b = *(const float4 *)(rows + r * d + 8 * c + 4);
    const int64_t row = first + r;
    corpus[((row >> 4) * KB + (c >> 2)) * 64 + 16 * (c & 3) + (row & 15)] =
        h16x8{(h16)a.x, (h16)a.y, (h16)a.z, (h16)a.w, (h16)b.x, (h16)b.y, (h16)b.z, (h16)b.w};
}

// rows f32 [n][d] -> int8 (quantize_row_i8) into i8 fragment order at rows first ..
// first + n - 1 with their scales; one wave per row, one 16-B store per 16 elements.
// A row touches only its own 16 B of each block and its own scale, so rows may
// start and end inside a group.
__global__ __launch_bounds__(kThreads) void index_add_i8_kernel(const float *__restrict__ rows, int64_t n, int d,
                                                                int64_t first, i32x4 *__restrict__ corpus,
                                                                float *__restrict__ scales)
{
    const int lane = threadIdx.x & 63, KB = d >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float sc;
    const i32x4 v = quantize_row_i8(rows + r * d, d, lane, sc);
    const int64_t row = first + r;
    if (lane < (d >> 4)) corpus[((row >> 4) * KB + (lane >> 2)) * 64 + 16 * (lane & 3) + (row & 15)] = v;
    if (lane == 0) scales[row] = sc;
}

// Benchmark data: row r of out [n][d] = a unit vector of hashed values in [-1, 1); one wave per row.
__global__ __launch_bounds__(kThreads) void unit_rows_kernel(float *__restrict__ out, int64_t n, int d, uint32_t seed)
{
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & 63;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) {
        uint32_t h = (uint32_t)(r * d + c) * 2654435761u + seed;
        h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
        const float v = (float)(h >> 8) * (1.0f / 8388608.0f) - 1.0f;
        out[r * d + c] = v;
        ss += v * v;
    }
    const float inv = 1.0f / sqrtf(wave_sum(ss));
    for (int c = lane; c < d; c += 64) out[r * d + c] *= inv;
}

template <int QT, int ST, class... Mask>
hipError_t allow_lds()
{
    return hipFuncSetAttribute((const void *)search_kernel<QT, ST, Mask...>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               kLdsBudget);
}

template <int ST, class... Mask>
hipError_t allow_lds_all()
{
    hipError_t e = allow_lds<1, ST, Mask...>();
    if (e == hipSuccess) e = allow_lds<2, ST, Mask...>();
    if (e == hipSuccess) e = allow_lds<3, ST, Mask...>();
    if (e == hipSuccess) e = allow_lds<4, ST, Mask...>();
    return e;
}

// One group of nq <= 64 queries: the streaming kernel over P row ranges, then the merge.
// mask: none (the unmasked kernel) or the group's SearchMask.
template <int ST, class... Mask>
int launch_group(const void *corpus, const float *row_scale, const float *Q, int nq, int d, int n_rows, int k,
                 int per, int P, Hit *part, float *d_scores, int32_t *d_ids, hipStream_t s, Mask... mask)
{
    typedef typename Store<ST>::Block Block;
    const int QT = (nq + 15) / 16;
    const size_t lds = search_lds_bytes<ST>(QT, d, k);
    const Block *C = (const Block *)corpus;
    switch (QT) {
    case 1: search_kernel<1, ST, Mask...><<<(unsigned)P, kThreads, lds, s>>>(C, Q, nq, d, n_rows, k, per, part, row_scale, mask...); break;
    case 2: search_kernel<2, ST, Mask...><<<(unsigned)P, kThreads, lds, s>>>(C, Q, nq, d, n_rows, k, per, part, row_scale, mask...); break;
    case 3: search_kernel<3, ST, Mask...><<<(unsigned)P, kThreads, lds, s>>>(C, Q, nq, d, n_rows, k, per, part, row_scale, mask...); break;
    default: search_kernel<4, ST, Mask...><<<(unsigned)P, kThreads, lds, s>>>(C, Q, nq, d, n_rows, k, per, part, row_scale, mask...); break;
    }
    if (hipGetLastError() != hipSuccess) return -3;
    search_merge_kernel<<<nq, kThreads, 0, s>>>(part, P, k, d_scores, d_ids);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int search_prepare_device()
{
    hipError_t e = allow_lds_all<SEARCH_F16>();
    if (e == hipSuccess) e = allow_lds_all<SEARCH_I8>();
    if (e == hipSuccess) e = allow_lds_all<SEARCH_F16, SearchMask>();
    if (e == hipSuccess) e = allow_lds_all<SEARCH_I8, SearchMask>();
    return e == hipSuccess ? 0 : -1;
}

int search_group_queries(int d, int k, int storage)
{
    int QT = 4;
    while (QT > 1 && search_lds_bytes(storage, QT, d, k) > (size_t)kLdsBudget) --QT;
    return 16 * QT;
}

int64_t search_max_workgroups(int64_t capacity_rows)
{
    const int64_t groups = (capacity_rows + 15) / 16;
    return std::max<int64_t>(1, std::min<int64_t>(2 * (int64_t)device_cu_count(), (groups + 3) / 4));
}

int launch_index_add(const float *d_rows, int64_t n, int d, int64_t first, int storage, void *corpus, float *scales,
                     hipStream_t s)
{
    if (n <= 0 || d % 64 || d < 64 || d > 1024) return -1;
    if (storage == SEARCH_I8) {
        if (!scales) return -1;
        index_add_i8_kernel<<<(unsigned)((n + 3) / 4), kThreads, 0, s>>>(d_rows, n, d, first, (i32x4 *)corpus, scales);
        return hipGetLastError() == hipSuccess ? 0 : -3;
    }
    if (storage != SEARCH_F16) return -1;
    const int64_t blocks = (n * (d / 8) + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return -1;
    index_add_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(d_rows, n, d, first, (h16x8 *)corpus);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_search(const void *corpus, const float *scales, int storage, int64_t n_rows, int d, const float *d_queries,
                  int B, int k, void *scratch, float *d_scores, int32_t *d_ids, hipStream_t s, const SearchMask *mask)
{
    if (B < 1 || k < 1 || k > 128 || d % 64 || d < 64 || d > 1024 || n_rows < 0 || n_rows > 0x7ffffff0) return -1;
    if ((storage != SEARCH_F16 && storage != SEARCH_I8) || (storage == SEARCH_I8 && !scales)) return -1;
    if (mask && !mask->tomb) return -1;
    const int QG = search_group_queries(d, k, storage);
    if (search_lds_bytes(storage, 1, d, k) > (size_t)kLdsBudget) return -1;
    // the row ranges: P workgroups of `per` groups each, per % 4 == 0 (one group per wave and step)
    const int64_t groups = std::max<int64_t>(1, (n_rows + 15) / 16);
    const int cus = device_cu_count();
    // block indices are 32-bit in the kernel, the ranges' overhang and the prefetch included
    // (counted in f16 blocks, d / 32 per group; int8 has half as many)
    if ((groups + 8 * (int64_t)cus + 8) * (d / 32) + 4 * kUnitsAhead > 0x7fffffffll) return -1;
    for (int b0 = 0; b0 < B; b0 += QG) {
        const int nq = std::min(QG, B - b0), QT = (nq + 15) / 16;
        const size_t lds = search_lds_bytes(storage, QT, d, k);
        const int64_t wg_per_cu = std::min<int64_t>(2, (int64_t)kLdsBudget / (int64_t)lds);
        int64_t P = std::max<int64_t>(1, std::min<int64_t>(wg_per_cu * cus, (groups + 3) / 4));
        const int64_t per = ((groups + P - 1) / P + 3) / 4 * 4;
        P = (groups + per - 1) / per;
        const float *Q = d_queries + (size_t)b0 * d;
        float *S = d_scores + (size_t)b0 * k;
        int32_t *I = d_ids + (size_t)b0 * k;
        int rc;
        if (mask) {
            // this group's filters; an empty index has no row to admit and its filters may have no word
            SearchMask gm = *mask;
            if (n_rows == 0) gm.filt = nullptr;
            if (gm.filt) gm.filt += (size_t)b0 * (size_t)gm.stride;
            rc = storage == SEARCH_I8 ? launch_group<SEARCH_I8>(corpus, scales, Q, nq, d, (int)n_rows, k, (int)per, (int)P,
                                                                (Hit *)scratch, S, I, s, gm)
                                      : launch_group<SEARCH_F16>(corpus, nullptr, Q, nq, d, (int)n_rows, k, (int)per, (int)P,
                                                                 (Hit *)scratch, S, I, s, gm);
        } else {
            rc = storage == SEARCH_I8 ? launch_group<SEARCH_I8>(corpus, scales, Q, nq, d, (int)n_rows, k, (int)per, (int)P,
                                                                (Hit *)scratch, S, I, s)
                                      : launch_group<SEARCH_F16>(corpus, nullptr, Q, nq, d, (int)n_rows, k, (int)per, (int)P,
                                                                 (Hit *)scratch, S, I, s);
        }
        if (rc != 0) return rc;
    }
    return 0;
}

int launch_search_merge(const void *partial, int nq, int P, int k, float *d_scores, int32_t *d_ids, hipStream_t s)
{
    if (!partial || nq < 1 || P < 1 || k < 1 || k > 128) return -1;
    search_merge_kernel<<<(unsigned)nq, kThreads, 0, s>>>((const Hit *)partial, P, k, d_scores, d_ids);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_unit_rows(float *d_out, int64_t n, int d, uint32_t seed, hipStream_t s)
{
    if (n <= 0 || d <= 0) return -1;
    unit_rows_kernel<<<(unsigned)((n + 3) / 4), kThreads, 0, s>>>(d_out, n, d, seed);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
