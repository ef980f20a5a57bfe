// Inverted-file lists and the probed search of the embedding index (bert_hip.h "Lists and
// probed search"): the rows of an f16 or int8 index clustered by their nearest
// centroid, and a search that reads only the lists a query probes.
//
// The clustered image.  A single stored row is 16-B pieces at a 256-B stride (search.hip's
// fragment order), so a list keeps its own contiguous copy of its rows, in the same fragment
// order and padded to whole 16-row groups: list l is groups goff[l] .. goff[l + 1] - 1 of the
// image, slot_id[16 g + f] is the row id whose copy sits in lane-fragment f of group g, -1 in the
// padding, and an int8 image has scale[16 g + f] beside it.  Padding holds zeros.  The order of
// the rows inside a list is whatever the atomics gave: no result bit depends on it.
//
// The search.  The centroids are an f16 image of their own, searched by launch_search for the
// n_probe lists of every query.  One workgroup sorts the pass's (list, query) pairs by list and
// cuts every run into items of one list and up to 16 of its queries; the scan kernel gives
// one workgroup to an item: the 16 query columns of the MFMA are the queries that probe the
// list, so the list is read once for all of them.  A score is search.hip's: the same B
// fragments, the d / 32 (d / 64) MFMAs of the row's group in ascending k from a zero accumulator,
// score_i8 for int8.  It depends on its own row and its own query only, so it has the bits the
// flat search gives that pair.  The per-(query, probe) lists go to launch_search_merge.
#include "device_common.h"
#include "kernels.h"
#include "quant_i8.h"
#include "topk_list.h"

#include <algorithm>

namespace emb {
namespace {

constexpr int kThreads = 256;
constexpr int kRing = 16;               // prefetch ring of the scan: 16 blocks of 1 KiB in flight per wave
constexpr int kPairBits = 13;           // a pass holds at most 64 x 128 = 2^13 (query, probe) pairs
constexpr int kMaxPairs = 1 << kPairBits;
constexpr uint32_t kNoList = 0x10000u;  // the list of a -1 probe: behind every real list (C <= 65,536)

template <int ST> struct Frag;
template <> struct Frag<SEARCH_F16> {
    typedef h16x8 Block;
    typedef f32x4 Acc;
    static constexpr int kShift = 5;
};
template <> struct Frag<SEARCH_I8> {
    typedef i32x4 Block;
    typedef i32x4 Acc;
    static constexpr int kShift = 6;
};

__device__ __forceinline__ f32x4 mma(h16x8 a, h16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ i32x4 mma(i32x4 a, i32x4 b, i32x4 c)
{
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}

// The 16-B piece c of row r in an image whose rows have `pieces` of them (d / 8 for f16,
// d / 16 for int8; a block holds 4 pieces of each of its 16 rows).
__device__ __forceinline__ size_t piece_at(int64_t r, int c, int pieces)
{
    return ((size_t)(r >> 4) * (size_t)(pieces >> 2) + (size_t)(c >> 2)) * 64 + 16 * (c & 3) + (int)(r & 15);
}

// Rows first .. first + n - 1 of the flat image widened to f32 [n][d]: the f16 values, or
// (float)q * scale in one f32 multiply (bertx_index_rows' values).  One thread per piece.
template <int ST>
__global__ __launch_bounds__(kThreads) void widen_kernel(const uint4 *__restrict__ corpus, const float *__restrict__ scales,
                                                         int64_t first, int n, int d, float *__restrict__ out)
{
    const int pieces = ST == SEARCH_I8 ? d >> 4 : d >> 3;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)n * pieces) return;
    const int r = (int)(i / pieces), c = (int)(i - (int64_t)r * pieces);
    const uint4 v = corpus[piece_at(first + r, c, pieces)];
    if constexpr (ST == SEARCH_F16) {
        const h16x8 h = __builtin_bit_cast(h16x8, v);
        float *o = out + (size_t)r * d + 8 * c;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (float)h[j];
    } else {
        const float sc = scales[first + r];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        float *o = out + (size_t)r * d + 16 * c;
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = __fmul_rn((float)(int8_t)(w[j >> 2] >> (8 * (j & 3))), sc);
    }
}

// count[l] += the rows of [0, n_rows) whose list is l; a row without a list (-1: its scores
// were not numbers) is in no list.
__global__ __launch_bounds__(kThreads) void lists_count_kernel(const int32_t *__restrict__ row_list, int n_rows, int C,
                                                               uint32_t *__restrict__ count)
{
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t l = (uint32_t)row_list[r];
    if (l < (uint32_t)C) atomicAdd(count + l, 1u);
}

// goff[l] = the 16-row groups of lists 0 .. l - 1, every list padded up; goff[C] the total.
// One workgroup: thread t sums lists [t per, (t + 1) per), the 256 sums are scanned in LDS,
// then every thread writes its lists' offsets.  count is left zeroed: it is the fill cursor next.
__global__ __launch_bounds__(kThreads) void lists_offsets_kernel(uint32_t *__restrict__ count, int C, uint32_t *__restrict__ goff)
{
    __shared__ uint32_t part[kThreads];
    const int tid = threadIdx.x, per = (C + kThreads - 1) / kThreads;
    const int l0 = min(tid * per, C), l1 = min(l0 + per, C);
    uint32_t sum = 0;
    for (int l = l0; l < l1; ++l) sum += (count[l] + 15u) >> 4;
    part[tid] = sum;
    lds_barrier();
    if (tid == 0) {
        uint32_t run = 0;
        for (int t = 0; t < kThreads; ++t) {
            const uint32_t v = part[t];
            part[t] = run;
            run += v;
        }
        goff[C] = run;
    }
    lds_barrier();
    uint32_t off = part[tid];
    for (int l = l0; l < l1; ++l) {
        goff[l] = off;
        off += (count[l] + 15u) >> 4;
        count[l] = 0;
    }
}

// One wave per row: lane 0 takes the row's slot in its list (an atomic on the list's cursor),
// the wave copies the row's pieces from the flat image to that slot of the clustered one and
// writes the slot's id (and scale).  A slot past the image (never, while count and fill read
// the same lists) is dropped.
template <int ST>
__global__ __launch_bounds__(kThreads) void lists_fill_kernel(const uint4 *__restrict__ corpus, const float *__restrict__ scales,
                                                              const int32_t *__restrict__ row_list, int n_rows, int C, int d,
                                                              const uint32_t *__restrict__ goff, uint32_t *__restrict__ cursor,
                                                              int64_t cap_slots, uint4 *__restrict__ image,
                                                              float *__restrict__ img_scales, int32_t *__restrict__ slot_id)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const uint32_t l = (uint32_t)row_list[r];
    if (l >= (uint32_t)C) return;
    uint32_t pos = 0;
    if (lane == 0) pos = atomicAdd(cursor + l, 1u);
    pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);
    const int64_t slot = (int64_t)goff[l] * 16 + pos;
    if (slot >= cap_slots || slot >= (int64_t)goff[l + 1] * 16) return;
    const int pieces = ST == SEARCH_I8 ? d >> 4 : d >> 3;
    for (int c = lane; c < pieces; c += 64) image[piece_at(slot, c, pieces)] = corpus[piece_at(r, c, pieces)];
    if (lane == 0) {
        slot_id[slot] = (int32_t)r;
        if constexpr (ST == SEARCH_I8) img_scales[slot] = scales[r];
    }
}

// The pass's pairs sorted by list.  probe_ids int32 [nq][n_probe]; pair i = b n_probe + p has
// the key list << 13 | i, so equal lists come in ascending (query, probe) order.  A bitonic
// sort in LDS over the next power of two (the padding keys sort last).  Then position i of
// the sorted run starts an item when it is the first, 17th, ... pair of its list: item_n[i] =
// the item's pairs (1 .. 16), 0 everywhere else.  A -1 probe (or one >= C) is in no item: its
// (query, probe) list is written here, as fill.
__global__ __launch_bounds__(kThreads) void pair_sort_kernel(const int32_t *__restrict__ probe_ids, int pairs, int C, int k,
                                                             uint32_t *__restrict__ sorted, int32_t *__restrict__ item_n,
                                                             Hit *__restrict__ partial)
{
    __shared__ uint32_t key[kMaxPairs];
    const int tid = threadIdx.x;
    int n2 = kThreads;
    while (n2 < pairs) n2 <<= 1;
    for (int i = tid; i < n2; i += kThreads) {
        uint32_t v = 0xffffffffu;
        if (i < pairs) {
            const uint32_t l = (uint32_t)probe_ids[i];
            v = ((l < (uint32_t)C ? l : kNoList) << kPairBits) | (uint32_t)i;
        }
        key[i] = v;
    }
    lds_barrier();
    for (int k2 = 2; k2 <= n2; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += kThreads) {
                const int o = i ^ j;
                if (o > i) {
                    const uint32_t a = key[i], b = key[o];
                    if ((a > b) == ((i & k2) == 0)) {
                        key[i] = b;
                        key[o] = a;
                    }
                }
            }
            lds_barrier();
        }
    for (int i = tid; i < pairs; i += kThreads) {
        const uint32_t v = key[i], l = v >> kPairBits;
        int n = 0;
        if (l == kNoList) {
            Hit *o = partial + (size_t)(v & (kMaxPairs - 1)) * k;
            for (int t = 0; t < k; ++t) o[t] = Hit{-INFINITY, -1};
        } else {
            int j = i;   // the run's first pair: at most 63 back, a list is probed once per query
            while (j > 0 && (key[j - 1] >> kPairBits) == l) --j;
            if (((i - j) & 15) == 0) {
                n = 1;
                while (n < 16 && i + n < pairs && (key[i + n] >> kPairBits) == l) ++n;
            }
        }
        sorted[i] = v;
        item_n[i] = n;
    }
}

// The scan of one item: workgroup i of the grid of `pairs` runs when item_n[i] != 0.
// LDS: the item's n <= 16 queries as the B fragments of one query tile (search_kernel's
// prologue; the columns past n are zeros and are never offered), their running lists, the
// score tile of one step.  A step is four consecutive groups of the list, wave w takes group
// 4 s + w of it: its d / 32 (d / 64) blocks come straight from HBM through a ring of kRing
// loads that runs ahead over the wave's later groups (a group past the list's end reloads the
// last one and is never offered).  After a step's scores are in the tile, wave w offers the 64
// rows to the lists of columns w, w + 4, ...: lane 16 h + f has row f of wave h's group, whose id
// it loaded at the start of the step.  A row is offered when its id is >= 0 and, in the masked
// instantiation, its tombstone is clear and its bit in the column's query's filter is set: the
// words are looked up by id, one vector load per lane (and per column for per-query filters).
// partial: [query][probe][k].
template <int ST, class... Mask>
__global__ __launch_bounds__(kThreads) void probe_scan_kernel(const typename Frag<ST>::Block *__restrict__ image,
                                                              const float *__restrict__ img_scales,
                                                              const int32_t *__restrict__ slot_id,
                                                              const uint32_t *__restrict__ goff,
                                                              const uint32_t *__restrict__ sorted,
                                                              const int32_t *__restrict__ item_n,
                                                              const float *__restrict__ queries, int d, int k, int n_probe,
                                                              Hit *__restrict__ partial, Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    typedef typename Frag<ST>::Block Block;
    typedef typename Frag<ST>::Acc Acc;
    const int n = item_n[blockIdx.x];
    if (n == 0) return;   // uniform over the workgroup
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int KB = d >> Frag<ST>::kShift;
    Block *qf = (Block *)smem;                          // [KB][64]
    Hit *lists = (Hit *)(qf + (size_t)KB * 64);         // [16][k]
    float *tile = (float *)(lists + (size_t)16 * k);    // [16][64]
    int *pq = (int *)(tile + 16 * 64);                  // [16]: the column's pair b n_probe + p, -1 past n
    float *qscale = (float *)(pq + 16);                 // int8: [16]

    if (tid < 16) pq[tid] = tid < n ? (int)(sorted[blockIdx.x + tid] & (kMaxPairs - 1)) : -1;
    const int l = (int)(sorted[blockIdx.x] >> kPairBits);
    lds_barrier();
    if constexpr (ST == SEARCH_F16) {
        const int chunks = d >> 3;
        for (int i = tid; i < 16 * chunks; i += kThreads) {
            const int j = i / chunks, c = i - j * chunks;
            h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (pq[j] >= 0) {
                const float *q = queries + (size_t)(pq[j] / n_probe) * d + 8 * c;
                const float4 a = *(const float4 *)q;
                const float4 b = *(const float4 *)(q + 4);
                v = h16x8{(h16)a.x, (h16)a.y, (h16)a.z, (h16)a.w, (h16)b.x, (h16)b.y, (h16)b.z, (h16)b.w};
            }
            qf[(size_t)(c >> 2) * 64 + 16 * (c & 3) + j] = v;
        }
    } else {
        for (int j = w; j < 16; j += 4) {
            float sc = 0.f;
            i32x4 v = {0, 0, 0, 0};
            if (pq[j] >= 0) v = quantize_row_i8(queries + (size_t)(pq[j] / n_probe) * d, d, lane, sc);
            if (lane < (d >> 4)) qf[(size_t)(lane >> 2) * 64 + 16 * (lane & 3) + j] = v;
            if (lane == 0) qscale[j] = sc;
        }
    }
    for (int i = tid; i < 16 * k; i += kThreads) lists[i] = Hit{-INFINITY, -1};
    lds_barrier();

    const int ws = __builtin_amdgcn_readfirstlane(w);
    const int gb = (int)goff[l], ge = (int)goff[l + 1];
    const int steps = (ge - gb + 3) >> 2;   // 0: an empty list, nothing is loaded
    const int g_last = ge - 1, U = steps * KB;
    const bool per_query = MK && m.filt && m.stride != 0;
    // the load position runs kRing blocks ahead of the MFMAs: (ls, lkb) = (step, block)
    int ls = 0, lkb = 0;
    auto load_next = [&]() {
        const int g = min(gb + 4 * ls + ws, g_last);
        const Block v = (image + ((size_t)g * KB + lkb) * 64)[lane];
        if (++lkb == KB) {
            lkb = 0;
            ++ls;
        }
        return v;
    };
    // what a step needs beside the blocks: the id of this lane's row of the step's 64 and,
    // int8, the scales of the four rows this lane's accumulator holds
    int32_t id = -1;
    f32x4 rsc = {0.f, 0.f, 0.f, 0.f};
    auto load_meta = [&](int s) {
        const int gh = gb + 4 * s + (lane >> 4);
        id = gh < ge ? slot_id[(size_t)gh * 16 + (lane & 15)] : -1;
        if constexpr (ST == SEARCH_I8)
            rsc = *(const f32x4 *)(img_scales + (size_t)min(gb + 4 * s + ws, g_last) * 16 + 4 * (lane >> 4));
    };
    Block ring[kRing];
    if (steps > 0) {
#pragma unroll
        for (int j = 0; j < kRing; ++j) {
            ring[j] = load_next();
            __builtin_amdgcn_sched_barrier(0);
        }
        load_meta(0);
    }
    Acc acc = {0, 0, 0, 0};
    int kb = 0, s = 0;
    for (int u0 = 0; u0 < U; u0 += kRing) {
#pragma unroll
        for (int j = 0; j < kRing; ++j) {
            if (u0 + j >= U) goto done;   // uniform over the workgroup; no path re-enters the ring out of order
            {
                acc = mma(ring[j], qf[(size_t)kb * 64 + lane], acc);
                __builtin_amdgcn_sched_barrier(0);
                ring[j] = load_next();
                __builtin_amdgcn_sched_barrier(0);
                if (++kb == KB) {
                    // accumulator register r of lane l: row 4 (l >> 4) + r of the wave's group, column l & 15
                    f32x4 sc;
                    if constexpr (ST == SEARCH_F16) {
                        sc = acc;
                    } else {
                        const float qs = qscale[lane & 15];
#pragma unroll
                        for (int r = 0; r < 4; ++r) sc[r] = score_i8(acc[r], qs, rsc[r]);
                    }
                    *(f32x4 *)&tile[(lane & 15) * 64 + 16 * w + 4 * (lane >> 4)] = sc;
                    acc = Acc{0, 0, 0, 0};
                    bool ok = id >= 0;
                    if constexpr (MK) {
                        if (ok) {
                            uint32_t word = ~m.tomb[id >> 5];
                            if (m.filt && !per_query) word &= m.filt[id >> 5];
                            ok = (word >> (id & 31)) & 1u;
                        }
                    }
                    lds_barrier();
                    for (int c = w; c < n; c += 4) {
                        bool okc = ok;
                        if constexpr (MK) {
                            if (per_query && ok)
                                okc = (m.filt[(size_t)(pq[c] / n_probe) * (size_t)m.stride + (size_t)(id >> 5)] >> (id & 31)) & 1u;
                        }
                        list_offer(lists + (size_t)c * k, k, tile[c * 64 + lane], id, okc, lane);
                    }
                    lds_barrier();
                    kb = 0;
                    ++s;
                    if (s < steps) load_meta(s);
                }
            }
        }
    }
done:
    for (int i = tid; i < n * k; i += kThreads) {
        const int j = i / k, t = i - j * k;
        partial[(size_t)pq[j] * k + t] = lists[i];
    }
}

// out[r][c] = rows[r][c] + cent[(r * step + shift) % C][c]: a benchmark row planted near a centroid.
__global__ __launch_bounds__(kThreads) void plant_rows_kernel(float *__restrict__ rows, int64_t n, int d,
                                                              const float *__restrict__ cent, int C, int64_t step,
                                                              int64_t shift, float noise)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n * d) return;
    const int64_t r = i / d;
    const int c = (int)(i - r * d);
    rows[i] = rows[i] * noise + cent[(size_t)((r * step + shift) % C) * d + c];
}

size_t scan_lds_bytes(int storage, int d, int k)
{
    return (size_t)16 * (storage == SEARCH_I8 ? d : 2 * d) + (size_t)16 * k * 8 + 16 * 64 * 4 + 16 * 4 + 16 * 4;
}

template <int ST, class... Mask>
int launch_scan(const void *image, const float *img_scales, const int32_t *slot_id, const uint32_t *goff,
                const uint32_t *sorted, const int32_t *item_n, const float *Q, int d, int k, int n_probe, int pairs,
                Hit *partial, hipStream_t s, Mask... mask)
{
    typedef typename Frag<ST>::Block Block;
    probe_scan_kernel<ST, Mask...><<<(unsigned)pairs, kThreads, scan_lds_bytes(ST, d, k), s>>>(
        (const Block *)image, img_scales, slot_id, goff, sorted, item_n, Q, d, k, n_probe, partial, mask...);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

bool shape_ok(int storage, int d) { return (storage == SEARCH_F16 || storage == SEARCH_I8) && d % 64 == 0 && d >= 64 && d <= 1024; }

}  // namespace

int launch_index_widen(const void *corpus, const float *scales, int storage, int64_t first, int n, int d, float *d_out,
                       hipStream_t s)
{
    if (!corpus || !d_out || first < 0 || n < 1 || !shape_ok(storage, d) || (storage == SEARCH_I8 && !scales)) return -1;
    const int pieces = storage == SEARCH_I8 ? d / 16 : d / 8;
    const unsigned blocks = (unsigned)(((int64_t)n * pieces + kThreads - 1) / kThreads);
    if (storage == SEARCH_I8)
        widen_kernel<SEARCH_I8><<<blocks, kThreads, 0, s>>>((const uint4 *)corpus, scales, first, n, d, d_out);
    else
        widen_kernel<SEARCH_F16><<<blocks, kThreads, 0, s>>>((const uint4 *)corpus, scales, first, n, d, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int64_t lists_max_groups(int64_t n_rows, int C) { return n_rows / 16 + C; }

size_t probed_partial_bytes(int C) { return (size_t)64 * (size_t)std::min(C, 128) * 128 * sizeof(Hit); }

int launch_lists_layout(const void *corpus, const float *scales, int storage, int64_t n_rows, int d,
                        const int32_t *row_list, int C, uint32_t *count, uint32_t *goff, void *image, float *img_scales,
                        int32_t *slot_id, int64_t cap_groups, hipStream_t s)
{
    if (!corpus || !row_list || !count || !goff || !image || !slot_id || !shape_ok(storage, d) || C < 1 || C > 65536 ||
        n_rows < 0 || n_rows > 0x7ffffff0 || cap_groups < lists_max_groups(n_rows, C) ||
        (storage == SEARCH_I8 && (!scales || !img_scales)))
        return -1;
    const size_t esz = storage == SEARCH_I8 ? 1 : 2;
    // the padding: zero rows, zero scales, id -1
    if (hipMemsetAsync(image, 0, (size_t)cap_groups * 16 * d * esz, s) != hipSuccess ||
        hipMemsetAsync(slot_id, 0xff, (size_t)cap_groups * 16 * 4, s) != hipSuccess ||
        hipMemsetAsync(count, 0, (size_t)C * 4, s) != hipSuccess ||
        (storage == SEARCH_I8 && hipMemsetAsync(img_scales, 0, (size_t)cap_groups * 16 * 4, s) != hipSuccess))
        return -3;
    if (n_rows > 0) lists_count_kernel<<<(unsigned)((n_rows + kThreads - 1) / kThreads), kThreads, 0, s>>>(row_list, (int)n_rows, C, count);
    lists_offsets_kernel<<<1, kThreads, 0, s>>>(count, C, goff);
    if (n_rows > 0) {
        const unsigned blocks = (unsigned)((n_rows + 3) / 4);
        if (storage == SEARCH_I8)
            lists_fill_kernel<SEARCH_I8><<<blocks, kThreads, 0, s>>>((const uint4 *)corpus, scales, row_list, (int)n_rows, C, d, goff,
                                                                     count, cap_groups * 16, (uint4 *)image, img_scales, slot_id);
        else
            lists_fill_kernel<SEARCH_F16><<<blocks, kThreads, 0, s>>>((const uint4 *)corpus, scales, row_list, (int)n_rows, C, d, goff,
                                                                      count, cap_groups * 16, (uint4 *)image, img_scales, slot_id);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_search_probed(const void *image, const float *img_scales, const int32_t *slot_id, const uint32_t *goff,
                         int storage, int C, int d, const float *d_queries, int nq, int k, int n_probe,
                         const int32_t *probe_ids, uint32_t *sorted, int32_t *item_n, void *partial, float *d_scores,
                         int32_t *d_ids, hipStream_t s, const SearchMask *mask)
{
    if (!image || !slot_id || !goff || !d_queries || !probe_ids || !sorted || !item_n || !partial || !shape_ok(storage, d) ||
        nq < 1 || nq > 64 || k < 1 || k > 128 || C < 1 || C > 65536 || n_probe < 1 || n_probe > std::min(C, 128) ||
        (storage == SEARCH_I8 && !img_scales) || (mask && !mask->tomb))
        return -1;
    const int pairs = nq * n_probe;
    pair_sort_kernel<<<1, kThreads, 0, s>>>(probe_ids, pairs, C, k, sorted, item_n, (Hit *)partial);
    if (hipGetLastError() != hipSuccess) return -3;
    int rc;
    if (mask)
        rc = storage == SEARCH_I8 ? launch_scan<SEARCH_I8>(image, img_scales, slot_id, goff, sorted, item_n, d_queries, d, k, n_probe,
                                                           pairs, (Hit *)partial, s, *mask)
                                  : launch_scan<SEARCH_F16>(image, img_scales, slot_id, goff, sorted, item_n, d_queries, d, k, n_probe,
                                                            pairs, (Hit *)partial, s, *mask);
    else
        rc = storage == SEARCH_I8 ? launch_scan<SEARCH_I8>(image, img_scales, slot_id, goff, sorted, item_n, d_queries, d, k, n_probe,
                                                           pairs, (Hit *)partial, s)
                                  : launch_scan<SEARCH_F16>(image, img_scales, slot_id, goff, sorted, item_n, d_queries, d, k, n_probe,
                                                            pairs, (Hit *)partial, s);
    if (rc != 0) return rc;
    return launch_search_merge(partial, nq, n_probe, k, d_scores, d_ids, s);
}

int launch_plant_rows(float *d_rows, int64_t n, int d, const float *d_cent, int C, int64_t step, int64_t shift, float noise,
                      hipStream_t s)
{
    if (!d_rows || !d_cent || n < 1 || d < 1 || C < 1 || step < 0 || shift < 0) return -1;
    const int64_t blocks = (n * d + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return -1;
    plant_rows_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(d_rows, n, d, d_cent, C, step, shift, noise);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
