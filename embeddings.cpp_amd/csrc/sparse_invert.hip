// Block-local inverted lists of the sparse index and the term-major search over them
// (bert_hip.h "Sparse index", "Inverted lists").
//
// A block is inv_block consecutive documents.  Its inverted image is an offset row uint32
// [V + 1] (row[t] .. row[t + 1]: the list of term t, counted from the block's first posting)
// and the block's postings regrouped by term, one uint32 each: the document's id within the
// block in the low 16 bits, the stored f16 weight bits in the high 16.  The lists of block b
// start where the forward store's document b * inv_block starts (table[b * inv_block].x * 16
// postings into the inverted area, which is as large as the forward store): a block's lists
// hold its postings without the padding, so they never reach the next block's.  The order
// within a list is whatever the fill's atomic cursors gave; no score bit depends on it,
// because a document occurs at most once in a list.
//
// Build (launch_sparse_invert), for the blocks that hold documents d0 .. d1 - 1, d0 a block's
// first document: zero the rows; count (a wave per document, one integer atomicAdd per posting
// into row[term + 1]); an exclusive prefix sum per row in place (one workgroup per block, 1,024
// entries a round, shuffle scan plus wave totals plus a carry); fill (the count's walk again,
// the rows' entries as cursors: atomicAdd returns the posting's place and leaves row[term + 1]
// at the list's end, which is the next list's start).
//
// Search (sparse_inv_search_kernel): workgroup (x, query) of 16 waves walks the blocks x,
// x + P, ...  Per block it
//   1. zeroes an f32 accumulator per document in LDS,
//   2. fetches the query's offset pairs, one slot per thread in one round of loads, and turns
//      the list lengths into an exclusive prefix sum over the slots (cum): the query's lists
//      laid end to end in slot order are one virtual array of cum[q_top] postings,
//   3. stages that array into LDS kStagePost postings at a time: thread t takes elements t,
//      t + 1,024, t + 2,048 of the chunk, finds each one's slot by a binary search of cum (LDS
//      only) and issues its loads together, so a chunk is one global round trip whatever the
//      number of lists in it, and a list longer than the staging area spans chunks,
//   4. applies the staged lists slot by slot: acc[id] = fmaf(f16(weight), w, acc[id]), the
//      threads of the workgroup side by side over a list (its ids are distinct: no two
//      threads meet on an accumulator, no atomics), a barrier between two slots, so every
//      accumulator receives its additions in the query's slot order,
//   5. offers the accumulators to the waves' top-k lists, wave w the documents 64 w .. 64 w +
//      63 of every 1,024, by list_offer.
// After the last block wave 0 folds the other waves' lists into its own and writes the
// workgroup's list; launch_search_merge merges the P lists of each query.
//
// Mask: nothing, the unmasked kernel, whose arguments end at partial; or one SearchMask over
// documents, the masked kernel.  Per (block, query), before step 1, the
// workgroup loads the block's inv_block / 32 admit words into LDS (~tombstones & the query's
// filter, the bits at and above n_docs cleared; a block starts on a multiple of 64 documents, so
// its words are whole) and ORs them over the workgroup through one flag per wave.  A block with
// no admissible document is skipped there: no offset row, no staging, no accumulation, no offers.
// Otherwise step 5 offers a document only when its bit is set; a wave's 64 documents are two words.
#include "device_common.h"
#include "kernels.h"
#include "maxsim_common.h"
#include "topk_list.h"

namespace emb {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kPerThread = 3;                        // staged postings per thread and chunk
constexpr int kStagePost = kPerThread * kThreads;    // postings of the staging area (12 KiB)
constexpr int kBuildThreads = 256;

// LDS words in front of the lists: acc [inv_block] | stage [kStagePost] | cum [q_top + 1] |
// start [q_top] | qw [q_top] | the scan's wave totals [kWaves] | masked: the block's admit words
// [inv_block / 32] and the waves' "some document is admissible" flags [kWaves] |, rounded to the
// lists' 8 bytes.  (No static LDS: the kernel's dynamic limit is the whole 160 KiB.)
__host__ __device__ inline int inv_admit_word(int inv_block, int q_top) { return inv_block + kStagePost + 3 * q_top + kWaves + 1; }
__host__ __device__ inline int inv_lists_word(int inv_block, int q_top, bool masked)
{
    return (inv_admit_word(inv_block, q_top) + (masked ? inv_block / 32 + kWaves : 0) + 1) & ~1;
}
inline size_t inv_lds_bytes(int inv_block, int q_top, int k, bool masked)
{
    return (size_t)inv_lists_word(inv_block, q_top, masked) * 4 + (size_t)kWaves * k * sizeof(Hit);
}

__global__ __launch_bounds__(kBuildThreads) void inv_zero_kernel(uint32_t *__restrict__ p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * kBuildThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kBuildThreads) p[i] = 0u;
}

// A wave per document d0 .. d1 - 1: !FILL counts posting (term, w) into row[term + 1] of the
// document's block; FILL takes its place from that cursor and writes (local id, w) there.
template <bool FILL>
__global__ __launch_bounds__(kBuildThreads) void inv_walk_kernel(const uint32_t *__restrict__ store,
                                                                 const int2 *__restrict__ table, int d0, int d1,
                                                                 int inv_block, int V, uint32_t *__restrict__ rows,
                                                                 uint32_t *__restrict__ inv)
{
    const int lane = threadIdx.x & 63, nw = (int)gridDim.x * (kBuildThreads / 64);
    for (int64_t doc = d0 + (int64_t)blockIdx.x * (kBuildThreads / 64) + (threadIdx.x >> 6); doc < d1; doc += nw) {
        const int2 e = table[doc];
        const int blk = (int)(doc / inv_block), local = (int)(doc - (int64_t)blk * inv_block);
        uint32_t *row = rows + (size_t)blk * (size_t)(V + 1);
        uint32_t *dst = nullptr;
        if constexpr (FILL) dst = inv + (size_t)table[(int64_t)blk * inv_block].x * 16;
        for (int j = lane; j < e.y; j += 64) {
            const uint32_t p = store[(size_t)e.x * 16 + j], t = p & 0xffffu;
            if (t >= (uint32_t)V) continue;
            const uint32_t at = atomicAdd(&row[t + 1], 1u);
            if constexpr (FILL) dst[at] = (uint32_t)local | (p & 0xffff0000u);
        }
    }
}

// The inclusive scan of x over the workgroup's 1,024 threads: returns this thread's inclusive
// value and the workgroup's total.  Two barriers: wave_tot is free again on return.
__device__ __forceinline__ uint32_t scan_1024(uint32_t x, uint32_t *wave_tot, int lane, int wv, uint32_t *total)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wave_tot[wv] = x;
    lds_barrier();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t t = wave_tot[w];
        if (w < wv) before += t;
        tot += t;
    }
    lds_barrier();
    *total = tot;
    return before + x;
}

// Block first + blockIdx.x: row[1 .. V] (the counts) -> their exclusive prefix sum, row[0] = 0.
__global__ __launch_bounds__(kThreads) void inv_prefix_kernel(uint32_t *__restrict__ rows, int first, int V)
{
    __shared__ uint32_t wave_tot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t *row = rows + (size_t)(first + (int)blockIdx.x) * (size_t)(V + 1);
    uint32_t carry = 0;
    for (int base = 0; base < V; base += kThreads) {
        const int i = base + tid;
        const uint32_t c = i < V ? row[1 + i] : 0u;
        uint32_t tot;
        const uint32_t inc = scan_1024(c, wave_tot, lane, wv, &tot);
        if (i < V) row[1 + i] = carry + inc - c;
        carry += tot;
    }
    if (tid == 0) row[0] = 0u;
}

// Workgroup (x, query): blocks x, x + gridDim.x, ...  partial: [B][gridDim.x][k].
template <class... Mask>
__global__ __launch_bounds__(kThreads) void sparse_inv_search_kernel(const uint32_t *__restrict__ inv,
                                                                     const uint32_t *__restrict__ rows,
                                                                     const int2 *__restrict__ table, int n_docs, int V,
                                                                     int inv_block, const int32_t *__restrict__ terms,
                                                                     const float *__restrict__ weights, int q_top, int k,
                                                                     Hit *__restrict__ partial, Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = blockIdx.y, P = gridDim.x;
    float *acc = (float *)smem;                              // [inv_block]
    uint32_t *stage = (uint32_t *)smem + inv_block;          // [kStagePost]
    uint32_t *cum = stage + kStagePost;                      // [q_top + 1]
    uint32_t *start = cum + q_top + 1;                       // [q_top]
    float *qw = (float *)(start + q_top);                    // [q_top]
    uint32_t *wave_tot = (uint32_t *)(qw + q_top);           // [kWaves]
    uint32_t *adm = (uint32_t *)smem + inv_admit_word(inv_block, q_top);   // masked: [inv_block / 32]
    uint32_t *wave_any = adm + (inv_block >> 5);                           // masked: [kWaves]
    Hit *lists = (Hit *)((uint32_t *)smem + inv_lists_word(inv_block, q_top, MK));   // [kWaves][k]
    Hit *mine = lists + (size_t)wv * k;

    // this thread's slot of the query: a term outside 0 .. V - 1 is an empty slot
    int32_t term = -1;
    if (tid < q_top) {
        term = terms[(size_t)q * q_top + tid];
        qw[tid] = (float)(h16)weights[(size_t)q * q_top + tid];
        if (term >= V) term = -1;
    }
    for (int i = tid; i < kWaves * k; i += kThreads) lists[i] = Hit{-INFINITY, -1};

    const int n_blocks = (n_docs + inv_block - 1) / inv_block;
    for (int b = blockIdx.x; b < n_blocks; b += P) {
        const int doc0 = b * inv_block, nb = min(inv_block, n_docs - doc0);
        if constexpr (MK) {
            // the block's admit words, and whether any document of the block is admissible
            const uint32_t *tomb = m.tomb + (doc0 >> 5);
            const uint32_t *filt = m.filt ? m.filt + (int64_t)q * m.stride + (doc0 >> 5) : nullptr;
            uint32_t some = 0u;
            for (int i = tid; i < inv_block >> 5; i += kThreads) {
                const int left = nb - 32 * i;   // the block's documents from this word on
                uint32_t a = 0u;
                if (left > 0) {
                    a = filt ? ~tomb[i] & filt[i] : ~tomb[i];
                    if (left < 32) a &= (1u << left) - 1u;
                }
                adm[i] = a;
                some |= a;
            }
            if (lane == 0) wave_any[wv] = 0u;   // (a wave's own flag: in order with the write below)
            if (__ballot(some != 0u) && lane == 0) wave_any[wv] = 1u;
            lds_barrier();
            const bool skip = __ballot(wave_any[lane & (kWaves - 1)] != 0u) == 0;
            if (skip) {
                lds_barrier();   // every wave has read the flags before the next block's are written
                continue;
            }
        }
        for (int i = tid; i < (nb + 3) >> 2; i += kThreads) ((float4 *)acc)[i] = float4{0.f, 0.f, 0.f, 0.f};
        const uint32_t *row = rows + (size_t)b * (size_t)(V + 1);
        uint32_t s0 = 0, len = 0;
        if (term >= 0) {
            s0 = row[term];
            len = row[term + 1] - s0;
        }
        const uint32_t *list0 = inv + (size_t)table[doc0].x * 16;
        uint32_t total;
        const uint32_t inc = scan_1024(len, wave_tot, lane, wv, &total);
        if (tid < q_top) {
            cum[tid] = inc - len;
            start[tid] = s0;
        }
        if (tid == 0) cum[q_top] = total;
        lds_barrier();   // the accumulators are zero, the slots' tables stand

        int slot = 0;    // the first slot that may reach into the chunk; the same in every thread
        for (uint32_t c0 = 0; c0 < total; c0 += kStagePost) {
            const uint32_t c1 = min(c0 + (uint32_t)kStagePost, total);
            uint32_t v[kPerThread];
#pragma unroll
            for (int j = 0; j < kPerThread; ++j) {
                const uint32_t e = c0 + (uint32_t)(tid + j * kThreads);
                v[j] = 0u;
                if (e < c1) {
                    int lo = 0, hi = q_top;   // the last slot whose cum is at most e
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (cum[mid] <= e) lo = mid;
                        else hi = mid;
                    }
                    v[j] = list0[start[lo] + (e - cum[lo])];
                }
            }
#pragma unroll
            for (int j = 0; j < kPerThread; ++j)
                if (c0 + (uint32_t)(tid + j * kThreads) < c1) stage[tid + j * kThreads] = v[j];
            lds_barrier();
            while (__builtin_amdgcn_readfirstlane(cum[slot + 1]) <= c0) ++slot;   // cum[q_top] = total > c0 ends it
            for (int i = slot; i < q_top; ++i) {
                const uint32_t a = __builtin_amdgcn_readfirstlane(cum[i]), z = __builtin_amdgcn_readfirstlane(cum[i + 1]);
                if (a >= c1) break;
                const uint32_t lo = max(a, c0), hi = min(z, c1);
                if (hi <= lo) continue;
                const float w = qw[i];
                for (uint32_t e = lo + tid; e < hi; e += kThreads) {
                    const uint32_t p = stage[e - c0], id = p & 0xffffu;
                    if (id < (uint32_t)nb) acc[id] = fmaf(w, (float)as_h((uint16_t)(p >> 16)), acc[id]);
                }
                lds_barrier();   // the next slot, or the next chunk's staging, follows this list
            }
        }

        for (int i0 = wv * 64; i0 < nb; i0 += kThreads) {
            const int i = i0 + lane;
            bool valid = i < nb;
            if constexpr (MK) valid = valid && ((adm[i >> 5] >> (i & 31)) & 1u);
            list_offer(mine, k, i < nb ? acc[i] : 0.f, doc0 + i, valid, lane);
        }
        lds_barrier();   // the next block's zeros and tables follow the offers
    }

    lds_barrier();
    if (wv == 0) {
        for (int o = 1; o < kWaves; ++o) {
            const Hit *src = lists + (size_t)o * k;
            Hit e0{-INFINITY, -1}, e1{-INFINITY, -1};
            if (lane < k) e0 = src[lane];
            if (lane + 64 < k) e1 = src[lane + 64];
            list_offer(lists, k, e0.s, e0.id, lane < k && e0.id >= 0, lane);
            list_offer(lists, k, e1.s, e1.id, lane + 64 < k && e1.id >= 0, lane);
        }
        for (int j = lane; j < k; j += 64) partial[((size_t)q * P + blockIdx.x) * k + j] = lists[j];
    }
}

// Benches: documents' rows get the heavy terms (sparse_bench_heavy_term) at a weight above every
// hashed value, heavy term j in a share 1/2 (3/4)^j of the rows by a hash of (row, j); queries'
// rows (all_of > 0) get the first all_of heavy terms in every row.
__global__ __launch_bounds__(kBuildThreads) void skew_rows_kernel(float *__restrict__ rows, int n, int V, uint32_t seed,
                                                                  int all_of)
{
    const int i = blockIdx.x * kBuildThreads + threadIdx.x;
    if (i >= n * kSparseHeavyTerms) return;
    const int r = i / kSparseHeavyTerms, j = i % kSparseHeavyTerms;
    uint32_t h = ((uint32_t)r * 0x9e3779b1u) ^ ((uint32_t)j * 0x85ebca6bu) ^ seed;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    float share = 0.5f;
    for (int o = 0; o < j; ++o) share *= 0.75f;
    const bool on = all_of > 0 ? j < all_of : (float)(h >> 8) * (1.f / 16777216.f) < share;
    if (on) rows[(size_t)r * V + sparse_bench_heavy_term(j, V)] = 2.f + 0.125f * (float)j;
}

}  // namespace

int sparse_inv_prepare_device()
{
    hipError_t e = allow_lds((const void *)sparse_inv_search_kernel<>);
    if (e == hipSuccess) e = allow_lds((const void *)sparse_inv_search_kernel<SearchMask>);
    return e == hipSuccess ? 0 : -1;
}

size_t sparse_inv_rows_bytes(int64_t cap_docs, int V, int inv_block)
{
    return (size_t)((cap_docs + inv_block - 1) / inv_block) * (size_t)(V + 1) * 4;
}

// A workgroup per (block, query) while the device has room for them: as many workgroups as
// its LDS holds, shared among the B queries, never more per query than blocks.
int sparse_inv_grid(int n_docs, int inv_block, int B, int q_top, int k, int max_wg, int *ran_wg, size_t *lds, bool masked)
{
    *lds = inv_lds_bytes(inv_block, q_top, k, masked);
    const int64_t blocks = ((int64_t)n_docs + inv_block - 1) / inv_block;
    const int64_t room = std::max<int64_t>(1, wg_per_cu(*lds) * device_cu_count() / B);
    return capped_grid(std::min(blocks, room), max_wg, ran_wg);
}

// B lists of the rule's most workgroups per query.
size_t sparse_inv_partial_bytes()
{
    return (size_t)std::max(kMaxWgPerCu * device_cu_count(), 64) * 128 * sizeof(Hit);
}

int launch_sparse_invert(const uint32_t *store, const void *d_table, int d0, int d1, int V, int inv_block, uint32_t *rows,
                         uint32_t *inv, hipStream_t s)
{
    if (!store || !d_table || !rows || !inv || V < 1 || V > 65536 || inv_block < 64 || inv_block > 65536 ||
        inv_block % 64 != 0 || d0 < 0 || d0 % inv_block != 0 || d1 < d0)
        return -1;
    if (d1 == d0) return 0;
    const int first = d0 / inv_block, blocks = (int)(((int64_t)d1 + inv_block - 1) / inv_block) - first;
    const size_t words = (size_t)blocks * (size_t)(V + 1);
    uint32_t *r0 = rows + (size_t)first * (size_t)(V + 1);
    const unsigned walk = (unsigned)std::min<int64_t>(((int64_t)(d1 - d0) + 3) / 4, 64 * (int64_t)device_cu_count());
    inv_zero_kernel<<<(unsigned)std::min<size_t>((words + kBuildThreads - 1) / kBuildThreads, 4096), kBuildThreads, 0, s>>>(r0, words);
    if (hipGetLastError() != hipSuccess) return -3;
    inv_walk_kernel<false><<<walk, kBuildThreads, 0, s>>>(store, (const int2 *)d_table, d0, d1, inv_block, V, rows, inv);
    if (hipGetLastError() != hipSuccess) return -3;
    inv_prefix_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(rows, first, V);
    if (hipGetLastError() != hipSuccess) return -3;
    inv_walk_kernel<true><<<walk, kBuildThreads, 0, s>>>(store, (const int2 *)d_table, d0, d1, inv_block, V, rows, inv);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_sparse_inv_search(const uint32_t *inv, const uint32_t *rows, const void *d_table, int n_docs, int V,
                             int inv_block, const int32_t *d_terms, const float *d_weights, int B, int q_top, int k,
                             void *partial, float *d_scores, int32_t *d_ids, hipStream_t s, int max_wg, int *ran_wg,
                             const SearchMask *mask)
{
    if (!inv || !rows || !d_table || !d_terms || !d_weights || !partial || !d_scores || !d_ids || n_docs < 0 || V < 1 ||
        V > 65536 || inv_block < 64 || inv_block > 65536 || inv_block % 64 != 0 || B < 1 || B > 64 || q_top < 1 ||
        q_top > 1024 || k < 1 || k > 128)
        return -1;
    size_t lds = 0;
    const int P = sparse_inv_grid(n_docs, inv_block, B, q_top, k, max_wg, ran_wg, &lds, mask != nullptr);
    if (lds > (size_t)kLdsBudget || (size_t)B * P * 128 * sizeof(Hit) > sparse_inv_partial_bytes()) return -1;
    if (mask)
        sparse_inv_search_kernel<SearchMask><<<dim3((unsigned)P, (unsigned)B), kThreads, lds, s>>>(
            inv, rows, (const int2 *)d_table, n_docs, V, inv_block, d_terms, d_weights, q_top, k, (Hit *)partial, *mask);
    else
        sparse_inv_search_kernel<><<<dim3((unsigned)P, (unsigned)B), kThreads, lds, s>>>(
            inv, rows, (const int2 *)d_table, n_docs, V, inv_block, d_terms, d_weights, q_top, k, (Hit *)partial);
    if (hipGetLastError() != hipSuccess) return -3;
    return launch_search_merge(partial, B, P, k, d_scores, d_ids, s);
}

int launch_sparse_skew_rows(float *d_rows, int n, int V, uint32_t seed, int all_of, hipStream_t s)
{
    if (!d_rows || n < 1 || V < 4 * kSparseHeavyTerms) return -1;
    skew_rows_kernel<<<(unsigned)((n * kSparseHeavyTerms + kBuildThreads - 1) / kBuildThreads), kBuildThreads, 0, s>>>(
        d_rows, n, V, seed, all_of);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
