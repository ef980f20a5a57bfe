// Fused top-k scan of the sparse index (bert_hip.h "Sparse index"): one
// streaming pass over the stored postings scores every document against the one or two
// queries of the pass and keeps the k best in LDS, so no [B][docs] score array exists.
//
// Store: a document is a run of postings, uint32 = term | f16(weight) << 16, ascending
// term, padded with (term 0, +0) to whole units of 16 postings (64 B); documents lie
// contiguous in id order; table int2 [docs] = (first unit, postings).
//
// Score of (query, document), the contract: qh[v] = f16(q[v]); posting j adds
// qh[term_j] * w_j to sub-sum j mod 16 by fmaf (the product is exact in f32, so the fma
// rounds once, as a multiply and an add would), each sub-sum from +0 in ascending j; the
// 16 sub-sums then fold 8, 4, 2, 1 apart (s_l + s_(l ^ 8), ...).  A padding posting adds
// qh[0] * +0 = +-0 to a sub-sum that is never -0: no bit changes.  The order depends on
// the document's posting count alone.
//
// Query table: the pass's queries as an LDS lookup table indexed by term, two queries
// interleaved as half2 [V] (one ds_read_b32 serves both) where two tables fit beside the
// lists, else one query as half [V] (sparse_scan_pair).  sparse_qtable_kernel writes the
// passes' tables once per search; a workgroup's prologue is a 16-byte copy.
//
// Work split: persistent workgroups of 16 waves, each workgroup a contiguous range of
// documents, each quarter-wave (16 lanes) a contiguous sub-range, so a quarter streams
// contiguous units and a document's end is bookkeeping: lane l of the quarter loads
// posting l of the unit (one dword, the wave four 64-B lines), the next unit's load is
// issued before the current one is used.  The step loop is wave-uniform; the quarters
// that close a document in a step fold their sub-sums by shuffles and lane 0 of each
// offers (score, id) to the wave's own list of the query (list_offer is a whole-wave
// operation).  At the end wave 0 folds the other waves' lists into its own and writes
// the workgroup's list; launch_search_merge merges the workgroups' lists.
//
// Mask: nothing, the unmasked kernel, whose arguments end at partial; or one SearchMask over
// documents (filt at the pass's first filter), the masked kernel.  A quarter
// keeps the admit words of the 32 documents around its current one in registers, ~tombstones &
// filter: one word when the pass's queries share a filter or have none, one per query when the
// filters are per query.  The words are loaded at the quarter's first document and again only
// when the document crosses a multiple of 32; a document's bit gates the `valid` of its offer,
// per query.  The postings are streamed and the scores computed as ever.
#include "device_common.h"
#include "kernels.h"
#include "maxsim_common.h"
#include "topk_list.h"

namespace emb {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kQuarters = 4 * kWaves;

// entries of one pass's table, a multiple of 16 bytes
inline size_t table_bytes(int V, int NQ) { return ((size_t)V * 2 * NQ + 15) / 16 * 16; }
inline size_t scan_lds_bytes(int V, int k, int NQ) { return table_bytes(V, NQ) + (size_t)kWaves * NQ * k * sizeof(Hit); }

// Pass p's table: entry v = f16(q[NQ p + i][v]) for its queries i < NQ, +0 for a query past
// B and for the entries that pad the table to 16 bytes.
template <int NQ>
__global__ __launch_bounds__(256) void sparse_qtable_kernel(const float *__restrict__ q, int B, int V, int entries,
                                                            h16 *__restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (v >= entries) return;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int b = NQ * p + i;
        out[((size_t)p * entries + v) * NQ + i] = v < V && b < B ? (h16)q[(size_t)b * V + v] : (h16)0.f;
    }
}

// The admit words of the 32 documents around `doc` (< n_docs) for the queries i < nq of the pass:
// a query that does not exist reads no filter, queries that share a filter read it once.
template <int NQ>
__device__ __forceinline__ void load_admit(const SearchMask &m, int nq, int doc, uint32_t (&adm)[NQ])
{
    const uint32_t live = ~m.tomb[doc >> 5];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        adm[i] = live;
        if (!m.filt || i >= nq) continue;
        if (i == 0 || m.stride != 0) adm[i] = live & m.filt[(int64_t)i * m.stride + (doc >> 5)];
        else adm[i] = adm[0];
    }
}

// nq <= NQ: the queries of this pass that exist.  partial: [nq][gridDim.x][k].
template <int NQ, class... Mask>
__global__ __launch_bounds__(kThreads) void sparse_scan_kernel(const uint32_t *__restrict__ store,
                                                               const int2 *__restrict__ table,
                                                               const int32_t *__restrict__ d_used, int n_docs,
                                                               const uint4 *__restrict__ qtab, int tab16, int nq, int k,
                                                               Hit *__restrict__ partial, Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & 15;
    Hit *lists = (Hit *)(smem + tab16);              // [wave][NQ][k]
    Hit *mine = lists + (size_t)wv * NQ * k;
    for (int i = tid; i < tab16; i += kThreads) smem[i] = qtab[i];
    for (int i = tid; i < kWaves * NQ * k; i += kThreads) lists[i] = Hit{-INFINITY, -1};
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
    uint32_t adm[NQ];   // masked: the admit words of documents 32 (doc / 32) .. + 31
#pragma unroll
    for (int i = 0; i < NQ; ++i) adm[i] = 0u;
    if constexpr (MK)
        if (doc < dend) load_admit<NQ>(m, nq, doc, adm);

    while (__ballot(doc < dend)) {
        const bool active = doc < dend, has = active && rem > 0;
        const uint32_t p = cur;
        if (has) {
            cur = store[(size_t)min(u + 1, last_unit) * 16 + l16];   // in flight under this unit's arithmetic
            const float w = (float)as_h((uint16_t)(p >> 16));
            const uint32_t term = p & 0xffffu;
            if constexpr (NQ == 2) {
                const h16x2 t = as_h2(((const uint32_t *)smem)[term]);
                acc[0] = fmaf((float)t.x, w, acc[0]);
                acc[1] = fmaf((float)t.y, w, acc[1]);
            } else {
                acc[0] = fmaf((float)((const h16 *)smem)[term], w, acc[0]);
            }
            ++u;
            --rem;
        }
        const bool fin = active && rem == 0;
        if (__ballot(fin)) {
            float s[NQ];
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                s[i] = acc[i];
#pragma unroll
                for (int o = 8; o >= 1; o >>= 1) s[i] = __fadd_rn(s[i], __shfl_xor(s[i], o, 64));
            }
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                bool ok = fin && l16 == 0;
                if constexpr (MK) ok = ok && ((adm[i] >> (doc & 31)) & 1u);
                if (i < nq) list_offer(mine + (size_t)i * k, k, s[i], doc, ok, lane);
            }
            if (fin) {
                ++doc;
                rem = (nxt + 15) >> 4;
                nxt = table[min(doc + 1, n_docs - 1)].y;
                if constexpr (MK)
                    if ((doc & 31) == 0 && doc < dend) load_admit<NQ>(m, nq, doc, adm);
#pragma unroll
                for (int i = 0; i < NQ; ++i) acc[i] = 0.f;
            }
        }
    }

    lds_barrier();
    if (wv == 0) {
        for (int i = 0; i < nq; ++i) {
            Hit *dst = lists + (size_t)i * k;
            for (int o = 1; o < kWaves; ++o) {
                const Hit *src = lists + ((size_t)o * NQ + i) * k;
                Hit e0{-INFINITY, -1}, e1{-INFINITY, -1};
                if (lane < k) e0 = src[lane];
                if (lane + 64 < k) e1 = src[lane + 64];
                list_offer(dst, k, e0.s, e0.id, lane < k && e0.id >= 0, lane);
                list_offer(dst, k, e1.s, e1.id, lane + 64 < k && e1.id >= 0, lane);
            }
            for (int j = lane; j < k; j += 64) partial[((size_t)i * gridDim.x + blockIdx.x) * k + j] = dst[j];
        }
    }
}

}  // namespace

int sparse_scan_prepare_device()
{
    hipError_t e = allow_lds((const void *)sparse_scan_kernel<1>);
    if (e == hipSuccess) e = allow_lds((const void *)sparse_scan_kernel<2>);
    if (e == hipSuccess) e = allow_lds((const void *)sparse_scan_kernel<1, SearchMask>);
    if (e == hipSuccess) e = allow_lds((const void *)sparse_scan_kernel<2, SearchMask>);
    return e == hipSuccess ? 0 : -1;
}

int sparse_scan_pair(int V, int k) { return scan_lds_bytes(V, k, 2) <= (size_t)kLdsBudget ? 2 : 1; }

size_t sparse_scan_table_bytes(int V) { return std::max(32 * table_bytes(V, 2), 64 * table_bytes(V, 1)); }

size_t sparse_scan_partial_bytes() { return (size_t)2 * scan_max_lists() * 128 * sizeof(Hit); }

int launch_sparse_scan(const uint32_t *store, const void *d_table, const int32_t *d_used, int n_docs, int V,
                       const float *d_queries, int B, int k, void *qtab, void *partial, float *d_scores, int32_t *d_ids,
                       hipStream_t s, int max_wg, int *ran_wg, const SearchMask *mask)
{
    if (!store || !d_table || !d_used || !d_queries || !qtab || !partial || !d_scores || !d_ids || n_docs < 0 || V < 1 ||
        V > 65536 || B < 1 || B > 64 || k < 1 || k > 128)
        return -1;
    const int NQ = sparse_scan_pair(V, k), passes = (B + NQ - 1) / NQ;
    const size_t tb = table_bytes(V, NQ), lds = scan_lds_bytes(V, k, NQ);
    if (lds > (size_t)kLdsBudget) return -1;
    const int entries = (int)(tb / (2 * NQ));
    const dim3 tg((unsigned)((entries + 255) / 256), (unsigned)passes);
    if (NQ == 2) sparse_qtable_kernel<2><<<tg, 256, 0, s>>>(d_queries, B, V, entries, (h16 *)qtab);
    else sparse_qtable_kernel<1><<<tg, 256, 0, s>>>(d_queries, B, V, entries, (h16 *)qtab);
    if (hipGetLastError() != hipSuccess) return -3;
    // a wave has four documents in flight: never more quarter-waves than documents
    const int P = scan_grid(lds, (n_docs + 3) / 4, kWaves, max_wg, ran_wg);
    for (int p = 0; p < passes; ++p) {
        const int nq = std::min(NQ, B - p * NQ);
        const uint4 *tab = (const uint4 *)((const char *)qtab + (size_t)p * tb);
        if (mask) {
            const SearchMask pm = pass_mask(*mask, (int64_t)p * NQ);
            if (NQ == 2)
                sparse_scan_kernel<2, SearchMask><<<(unsigned)P, kThreads, lds, s>>>(
                    store, (const int2 *)d_table, d_used, n_docs, tab, (int)(tb / 16), nq, k, (Hit *)partial, pm);
            else
                sparse_scan_kernel<1, SearchMask><<<(unsigned)P, kThreads, lds, s>>>(
                    store, (const int2 *)d_table, d_used, n_docs, tab, (int)(tb / 16), nq, k, (Hit *)partial, pm);
        } else if (NQ == 2)
            sparse_scan_kernel<2><<<(unsigned)P, kThreads, lds, s>>>(store, (const int2 *)d_table, d_used, n_docs, tab,
                                                                     (int)(tb / 16), nq, k, (Hit *)partial);
        else
            sparse_scan_kernel<1><<<(unsigned)P, kThreads, lds, s>>>(store, (const int2 *)d_table, d_used, n_docs, tab,
                                                                     (int)(tb / 16), nq, k, (Hit *)partial);
        if (hipGetLastError() != hipSuccess) return -3;
        const int rc = launch_search_merge(partial, nq, P, k, d_scores + (size_t)p * NQ * k, d_ids + (size_t)p * NQ * k, s);
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace emb
