// Batched scan of the sparse index with sparse queries (bert_hip.h "Sparse index"; DESIGN.md
// 9i-3): one streaming pass over the stored postings scores every document against the NQ
// = 32, 16, 8 or 4 queries of the pass, where sparse_scan.hip's dense lookup tables hold two.
//
// Queries arrive as int32 terms [B][q_top] and f32 weights [B][q_top], term -1 an empty slot
// (launch_sparse_select's output).  The score is the contract of sparse_scan.hip: posting j
// adds qh[term_j] * w_j to sub-sum j mod 16 by fmaf, from +0, in ascending j, and the 16
// sub-sums fold 8, 4, 2, 1 apart.  A posting whose term is in no query of the pass would add
// +-0 to a sub-sum that is never -0, so leaving it out changes no bit: this kernel adds only
// the postings that hit, in the same lane, the same order and the same fold, and returns the
// bits of the dense-query search of the densified queries.
//
// Query image of a pass (sparse_image_kernel, one workgroup per pass, once per search):
//   header  uint32 U, the terms that occur in any query of the pass
//   dict    uint2 {bits, base} per 32 terms: bits marks those terms, base counts the marked
//           terms of earlier words; a term's slot is base + popcount(bits below it)
//   W       f16 [U][NQ]: row = slot, column i = f16(weight) of query i, +0 where it lacks the term
// The scan copies dict and the U rows of W into LDS.  A posting costs one ds_read_b64 of its
// dictionary word and a bit test; only a hit reads its NQ-wide row and runs NQ fmafs.
//
// Work split as sparse_scan_kernel: persistent workgroups of 16 waves, a contiguous range of
// documents per workgroup and per quarter-wave, lane l of a quarter takes posting l of each
// 64-byte unit, the next unit's load in flight under the current one.  At a document's end
// the 16 lanes fold by a halving exchange: partners l and l ^ 8 trade half of their queries
// and add, then l ^ 4 a quarter, and so on; every step adds the same two values the plain
// fold adds (f32 addition commutes), and lane l ends with the finished scores of NQ / 16
// queries (NQ < 16: the last steps are plain shuffles).
//
// Top-k: one list per (workgroup, query) in LDS.  A closing quarter stages (id, scores[NQ])
// into its wave's kDepth slots of a tile; a wave scans until fewer than four slots are free
// or its range is done; after a barrier wave w offers the staged entries, 64 per list_offer,
// to the lists of queries w, w + 16, ...; a second barrier carries every wave's "documents
// left" flag, and the loop ends when none has.  (A workgroup OR by flags in the dynamic LDS:
// the library reduction's static words would not fit beside a full 160 KiB.)
//
// Mask: nothing, the unmasked kernel, whose arguments end at partial; or one SearchMask over
// documents (filt at the pass's first filter), the masked kernel.  The part of
// the mask the pass's queries share, the tombstones and a filter given once for all queries, is
// tested where a quarter closes a document, from a word the quarter keeps for the 32 documents
// around its current one: a document it rejects takes no staging slot, writes nothing and is
// never offered, and the slots count the admitted documents only.  Filters given per query
// cannot be tested there, since a staged document serves every query; wave w, offering for
// query i, gathers the word of each staged id from query i's filter and gates its offer.
#include "device_common.h"
#include "kernels.h"
#include "maxsim_common.h"
#include "topk_list.h"

namespace emb {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kQuarters = 4 * kWaves;
constexpr int kDepth = 16;                     // staging slots per wave
constexpr int kSlots = kWaves * kDepth;        // staging slots per workgroup
constexpr int kHeader = 16;                    // bytes in front of an image's dictionary

inline size_t round16(size_t b) { return (b + 15) / 16 * 16; }
inline size_t dict_bytes(int V) { return round16((size_t)((V + 31) / 32) * 8); }
// rows of W in the worst case: every slot of every query another term
inline int max_rows(int V, int q_top, int NQ) { return std::min(NQ * q_top, V); }
inline size_t w_bytes(int V, int q_top, int NQ) { return round16((size_t)max_rows(V, q_top, NQ) * NQ * 2); }
inline size_t image_bytes(int V, int q_top, int NQ) { return kHeader + dict_bytes(V) + w_bytes(V, q_top, NQ); }
// dict | W | lists [NQ][k] | staged scores [NQ][kSlots] | staged ids [kSlots] | counts, flags [2][kWaves]
inline size_t batch_lds_bytes(int V, int q_top, int k, int NQ)
{
    return dict_bytes(V) + w_bytes(V, q_top, NQ) + (size_t)NQ * k * sizeof(Hit) + (size_t)NQ * kSlots * 4 + kSlots * 4 +
           2 * kWaves * 4;
}

// Pass p's image of its nq = min(NQ, B - NQ p) queries.  V <= 65,536 is at most 2,048
// dictionary words, two per thread.  A term outside 0 .. V - 1 is an empty slot.  Of a term
// repeated within a query the highest slot wins: a wave owns a query, walks its slots 64 at
// a time in ascending order and silences a lane whose term a higher lane repeats.
__global__ __launch_bounds__(kThreads) void sparse_image_kernel(const int32_t *__restrict__ terms,
                                                                const float *__restrict__ weights, int B, int q_top,
                                                                int V, int NQ, size_t img_bytes, char *__restrict__ images)
{
    __shared__ uint32_t bits[2 * kThreads];
    __shared__ int base[2 * kThreads], wave_tot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, p = blockIdx.x;
    const int nq = min(NQ, B - p * NQ), words = (V + 31) >> 5;
    const int32_t *tp = terms + (size_t)p * NQ * q_top;
    const float *wp = weights + (size_t)p * NQ * q_top;
    char *img = images + (size_t)p * img_bytes;

    bits[2 * tid] = bits[2 * tid + 1] = 0u;
    lds_barrier();
    for (int i = tid; i < nq * q_top; i += kThreads) {
        const int32_t t = tp[i];
        if (t >= 0 && t < V) atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
    lds_barrier();

    // exclusive prefix sum of the words' popcounts
    const int c0 = __popc(bits[2 * tid]), c1 = __popc(bits[2 * tid + 1]);
    int inc = c0 + c1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_tot[wv] = inc;
    lds_barrier();
    int before = 0, U = 0;
    for (int o = 0; o < kWaves; ++o) {
        const int t = wave_tot[o];
        if (o < wv) before += t;
        U += t;
    }
    base[2 * tid] = before + inc - c0 - c1;
    base[2 * tid + 1] = before + inc - c1;
    lds_barrier();

    if (tid == 0) *(uint32_t *)img = (uint32_t)U;
    uint2 *dict = (uint2 *)(img + kHeader);
    for (int i = tid; i < words; i += kThreads) dict[i] = uint2{bits[i], (uint32_t)base[i]};
    h16 *W = (h16 *)(img + kHeader + (((size_t)words * 8 + 15) & ~(size_t)15));
    uint32_t *W32 = (uint32_t *)W;
    for (int i = tid; i < U * NQ / 2; i += kThreads) W32[i] = 0u;
    __threadfence();
    __syncthreads();   // the zeros are out before a weight lands on one

    for (int q = wv; q < nq; q += kWaves) {
        for (int j0 = 0; j0 < q_top; j0 += 64) {
            const int j = j0 + lane;
            const int32_t t = j < q_top ? tp[(size_t)q * q_top + j] : -1;
            const float w = j < q_top ? wp[(size_t)q * q_top + j] : 0.f;
            bool live = t >= 0 && t < V;
#pragma unroll
            for (int l = 1; l < 64; ++l)
                if (__builtin_amdgcn_readlane(t, l) == t && lane < l) live = false;
            if (live) {
                const uint32_t b = bits[t >> 5], below = b & ((1u << (t & 31)) - 1u);
                W[(size_t)(base[t >> 5] + __popc(below)) * NQ + q] = (h16)w;
            }
            __threadfence();   // a later step's store to the same entry follows this one
        }
    }
}

// The 16 sub-sums of a quarter folded 8, 4, 2, 1 apart by a halving exchange.  On return
// a[0 .. max(NQ / 16, 1) - 1] of lane l16 are finished scores of queries first, first + 1, ...
// (NQ < 16: 16 / NQ neighbouring lanes hold the same query).
template <int NQ, int N, int O>
__device__ __forceinline__ void fold_step(float (&a)[NQ], int l16, int &first)
{
    if constexpr (N > 1) {
        constexpr int H = N / 2;
        const bool up = (l16 & O) != 0;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float lo = a[j], hi = a[j + H];
            const float keep = up ? hi : lo, send = up ? lo : hi;
            a[j] = __fadd_rn(keep, __shfl_xor(send, O, 64));
        }
        if (up) first += H;
    } else {
        a[0] = __fadd_rn(a[0], __shfl_xor(a[0], O, 64));
    }
    if constexpr (O > 1) fold_step<NQ, (N > 1 ? N / 2 : 1), O / 2>(a, l16, first);
}
template <int NQ>
__device__ __forceinline__ int fold_halving(float (&a)[NQ], int l16)
{
    int first = 0;
    fold_step<NQ, NQ, 8>(a, l16, first);
    return first;
}

// nq <= NQ: the queries of this pass that exist.  partial: [nq][gridDim.x][k].
template <int NQ, class... Mask>
__global__ __launch_bounds__(kThreads) void sparse_scan_batch_kernel(const uint32_t *__restrict__ store,
                                                                     const int2 *__restrict__ table,
                                                                     const int32_t *__restrict__ d_used, int n_docs,
                                                                     const char *__restrict__ image, int dict16,
                                                                     int w16, int nq, int k, Hit *__restrict__ partial,
                                                                     Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    // the filter every query of the pass shares (tested with the tombstones where a document
    // closes), and whether each query has its own (tested at the offer)
    const uint32_t *shared_filt = m.stride == 0 ? m.filt : nullptr;
    const bool own_filt = m.filt && m.stride != 0;
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & 15;
    const uint2 *dict = (const uint2 *)smem;
    const h16 *W = (const h16 *)(smem + dict16);
    Hit *lists = (Hit *)(smem + dict16 + w16);                 // [NQ][k]
    float *st_s = (float *)(lists + (size_t)NQ * k);           // [NQ][kSlots]
    int32_t *st_id = (int32_t *)(st_s + NQ * kSlots);          // [kSlots]
    int32_t *st_cnt = st_id + kSlots, *st_more = st_cnt + kWaves;   // [kWaves] each

    {
        const uint4 *src = (const uint4 *)(image + kHeader);
        const int rows16 = min(w16, (int)((*(const uint32_t *)image * (uint32_t)(NQ * 2) + 15u) >> 4));
        for (int i = tid; i < dict16; i += kThreads) smem[i] = src[i];
        for (int i = tid; i < rows16; i += kThreads) smem[dict16 + i] = src[dict16 + i];
        for (int i = tid; i < NQ * k; i += kThreads) lists[i] = Hit{-INFINITY, -1};
    }
    lds_barrier();

    // this workgroup's documents, this quarter's of them
    const int per_wg = (n_docs + (int)gridDim.x - 1) / (int)gridDim.x;
    const int w0 = min((int)blockIdx.x * per_wg, n_docs), w1 = min(w0 + per_wg, n_docs);
    const int per_q = (w1 - w0 + kQuarters - 1) / kQuarters, qi = 4 * wv + (lane >> 4);
    int doc = min(w0 + qi * per_q, w1);
    const int dend = min(doc + per_q, w1);
    const int last_unit = d_used[0] - 1;             // loads stay inside the used units

    int u = 0, rem = 0, nxt = 0;
    uint32_t cur = 0;
    if (doc < dend) {
        const int2 e = table[doc];
        u = e.x;
        rem = (e.y + 15) >> 4;
        nxt = table[min(doc + 1, n_docs - 1)].y;
        if (last_unit >= 0) cur = store[(size_t)min(u, last_unit) * 16 + l16];
    }
    float acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = 0.f;
    // masked: the shared admit word of documents 32 (doc / 32) .. + 31, reloaded when doc crosses
    // a multiple of 32
    auto shared_admit = [&](int d) {
        const uint32_t live = ~m.tomb[d >> 5];
        return shared_filt ? live & shared_filt[d >> 5] : live;
    };
    uint32_t adm = 0u;
    if constexpr (MK)
        if (doc < dend) adm = shared_admit(doc);

    bool any = true;
    while (any) {
        int cnt = 0;   // staged by this wave in this round
        while (cnt <= kDepth - 4 && __ballot(doc < dend)) {
            const bool active = doc < dend, has = active && rem > 0;
            const uint32_t p = cur;
            if (has) {
                cur = store[(size_t)min(u + 1, last_unit) * 16 + l16];   // in flight under this unit's arithmetic
                const uint32_t term = p & 0xffffu, b = term & 31u;
                const uint2 wd = dict[term >> 5];
                if ((wd.x >> b) & 1u) {
                    const float w = (float)as_h((uint16_t)(p >> 16));
                    const h16 *row = W + (size_t)(wd.y + __popc(wd.x & ((1u << b) - 1u))) * NQ;
                    if constexpr (NQ == 4) {
                        const h16x4 r = *(const h16x4 *)row;
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] = fmaf((float)r[i], w, acc[i]);
                    } else {
#pragma unroll
                        for (int c = 0; c < NQ / 8; ++c) {
                            const h16x8 r = ((const h16x8 *)row)[c];
#pragma unroll
                            for (int i = 0; i < 8; ++i) acc[8 * c + i] = fmaf((float)r[i], w, acc[8 * c + i]);
                        }
                    }
                }
                ++u;
                --rem;
            }
            const bool fin = active && rem == 0;
            // take: the quarter closes a document that is staged (masked: an admitted one)
            bool take = fin;
            if constexpr (MK) take = fin && ((adm >> (doc & 31)) & 1u);
            const unsigned long long closing = __ballot(take && l16 == 0);
            unsigned long long ending = closing;   // the quarters that close a document, staged or not
            if constexpr (MK) ending = __ballot(fin);
            if (ending) {
                if (closing) {
                    float s[NQ];
#pragma unroll
                    for (int i = 0; i < NQ; ++i) s[i] = acc[i];
                    const int first = fold_halving<NQ>(s, l16);
                    if (take) {
                        const int slot = wv * kDepth + cnt + __popcll(closing & ((1ull << (lane & 48)) - 1ull));
                        if constexpr (NQ >= 16) {
#pragma unroll
                            for (int j = 0; j < NQ / 16; ++j) st_s[(first + j) * kSlots + slot] = s[j];
                        } else {
                            if ((l16 & (16 / NQ - 1)) == 0) st_s[first * kSlots + slot] = s[0];
                        }
                        if (l16 == 0) st_id[slot] = doc;
                    }
                }
                if (fin) {
                    ++doc;
                    rem = (nxt + 15) >> 4;
                    nxt = table[min(doc + 1, n_docs - 1)].y;
#pragma unroll
                    for (int i = 0; i < NQ; ++i) acc[i] = 0.f;
                    if constexpr (MK)
                        if ((doc & 31) == 0 && doc < dend) adm = shared_admit(doc);
                }
                cnt += __popcll(closing);
            }
        }
        if (lane == 0) st_cnt[wv] = cnt;
        lds_barrier();
        for (int i = wv; i < nq; i += kWaves) {
#pragma unroll
            for (int g = 0; g < kSlots / 64; ++g) {
                const int slot = 64 * g + lane;
                bool valid = (slot & (kDepth - 1)) < st_cnt[slot / kDepth];
                if constexpr (MK) {
                    if (own_filt && valid) {   // query i's own filter: the word of the staged id
                        const int32_t id = st_id[slot];
                        valid = (m.filt[(int64_t)i * m.stride + (id >> 5)] >> (id & 31)) & 1u;
                    }
                }
                if (__ballot(valid)) list_offer(lists + (size_t)i * k, k, st_s[i * kSlots + slot], st_id[slot], valid, lane);
            }
        }
        // the workgroup's "any wave has work", its second barrier of the round
        const bool more = __ballot(doc < dend) != 0;
        if (lane == 0) st_more[wv] = more;
        lds_barrier();
        any = __ballot(st_more[lane & (kWaves - 1)] != 0) != 0;
    }

    for (int i = wv; i < nq; i += kWaves)
        for (int j = lane; j < k; j += 64) partial[((size_t)i * gridDim.x + blockIdx.x) * k + j] = lists[(size_t)i * k + j];
}

// mask: none (the unmasked kernel) or the pass's SearchMask
template <int NQ, class... Mask>
void launch_pass(int P, size_t lds, hipStream_t s, const uint32_t *store, const void *d_table, const int32_t *d_used,
                 int n_docs, const char *image, int V, int q_top, int nq, int k, void *partial, Mask... mask)
{
    sparse_scan_batch_kernel<NQ, Mask...><<<(unsigned)P, kThreads, lds, s>>>(
        store, (const int2 *)d_table, d_used, n_docs, image, (int)(dict_bytes(V) / 16),
        (int)(w_bytes(V, q_top, NQ) / 16), nq, k, (Hit *)partial, mask...);
}

template <class... Mask>
void launch_pass_of(int NQ, int P, size_t lds, hipStream_t s, const uint32_t *store, const void *d_table,
                    const int32_t *d_used, int n_docs, const char *image, int V, int q_top, int nq, int k, void *partial,
                    Mask... mask)
{
    switch (NQ) {
    case 32: launch_pass<32>(P, lds, s, store, d_table, d_used, n_docs, image, V, q_top, nq, k, partial, mask...); break;
    case 16: launch_pass<16>(P, lds, s, store, d_table, d_used, n_docs, image, V, q_top, nq, k, partial, mask...); break;
    case 8: launch_pass<8>(P, lds, s, store, d_table, d_used, n_docs, image, V, q_top, nq, k, partial, mask...); break;
    default: launch_pass<4>(P, lds, s, store, d_table, d_used, n_docs, image, V, q_top, nq, k, partial, mask...); break;
    }
}

template <class... Mask>
hipError_t allow_lds_all()
{
    hipError_t e = allow_lds((const void *)sparse_scan_batch_kernel<32, Mask...>);
    if (e == hipSuccess) e = allow_lds((const void *)sparse_scan_batch_kernel<16, Mask...>);
    if (e == hipSuccess) e = allow_lds((const void *)sparse_scan_batch_kernel<8, Mask...>);
    if (e == hipSuccess) e = allow_lds((const void *)sparse_scan_batch_kernel<4, Mask...>);
    return e;
}

}  // namespace

int sparse_batch_prepare_device()
{
    hipError_t e = allow_lds_all<>();
    if (e == hipSuccess) e = allow_lds_all<SearchMask>();
    return e == hipSuccess ? 0 : -1;
}

int sparse_batch_queries(int V, int q_top, int k)
{
    if (V < 1 || V > 65536 || q_top < 1 || q_top > 1024 || k < 1 || k > 128) return 0;
    for (int NQ = 32; NQ >= 4; NQ >>= 1)
        if (batch_lds_bytes(V, q_top, k, NQ) <= (size_t)kLdsBudget) return NQ;
    return 0;
}

// An image is smaller than the LDS that holds it, and a search has at most 64 / 4 passes.
size_t sparse_batch_image_bytes() { return (size_t)16 * (kLdsBudget + kHeader); }

// One workgroup per CU, up to 32 lists each.
size_t sparse_batch_partial_bytes() { return (size_t)32 * device_cu_count() * 128 * sizeof(Hit); }

int launch_sparse_batch_image(const int32_t *d_terms, const float *d_weights, int B, int q_top, int V, int k, void *images,
                              hipStream_t s)
{
    const int NQ = sparse_batch_queries(V, q_top, k);
    if (!d_terms || !d_weights || !images || B < 1 || B > 64 || NQ == 0) return -1;
    sparse_image_kernel<<<(unsigned)((B + NQ - 1) / NQ), kThreads, 0, s>>>(d_terms, d_weights, B, q_top, V, NQ,
                                                                          image_bytes(V, q_top, NQ), (char *)images);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_sparse_scan_batch(const uint32_t *store, const void *d_table, const int32_t *d_used, int n_docs, int V,
                             const int32_t *d_terms, const float *d_weights, int B, int q_top, int k, void *images,
                             void *partial, float *d_scores, int32_t *d_ids, hipStream_t s, int max_wg, int *ran_wg,
                             const SearchMask *mask)
{
    if (!store || !d_table || !d_used || !partial || !d_scores || !d_ids || n_docs < 0) return -1;
    const int NQ = sparse_batch_queries(V, q_top, k);
    if (const int rc = launch_sparse_batch_image(d_terms, d_weights, B, q_top, V, k, images, s)) return rc;
    const size_t lds = batch_lds_bytes(V, q_top, k, NQ), ib = image_bytes(V, q_top, NQ);
    // a wave has four documents in flight: never more quarter-waves than documents; one
    // workgroup per CU (the budget as the LDS figure), which is what `partial` is sized for
    const int P = scan_grid((size_t)kLdsBudget, (n_docs + 3) / 4, kWaves, max_wg, ran_wg);
    for (int p = 0; p * NQ < B; ++p) {
        const int nq = std::min(NQ, B - p * NQ);
        const char *img = (const char *)images + (size_t)p * ib;
        if (mask)
            launch_pass_of(NQ, P, lds, s, store, d_table, d_used, n_docs, img, V, q_top, nq, k, partial,
                           pass_mask(*mask, (int64_t)p * NQ));
        else
            launch_pass_of(NQ, P, lds, s, store, d_table, d_used, n_docs, img, V, q_top, nq, k, partial);
        if (hipGetLastError() != hipSuccess) return -3;
        const int rc = launch_search_merge(partial, nq, P, k, d_scores + (size_t)p * NQ * k, d_ids + (size_t)p * NQ * k, s);
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace emb
