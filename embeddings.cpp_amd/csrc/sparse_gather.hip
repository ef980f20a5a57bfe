// Scores of listed documents of the sparse index (bert_hip.h "Sparse index", "Listed
// documents"): d_scores [B][n] = the score of (sparse query b, document
// d_ids[b][j]) with the bits of the document-major scans, -inf for an id the store does not
// hold or has deleted.
//
// The score is the contract of sparse_scan.hip: posting j adds qh[term_j] * w_j to sub-sum
// j mod 16 by fmaf, from +0, in ascending j, and the 16 sub-sums fold 8, 4, 2, 1 apart.  One
// quarter-wave (16 lanes) owns one listed document and lane l takes posting l of every
// 64-byte unit, as the scans' quarters do: the lane, the order of the additions and the fold
// are the scans', so the bits are theirs.  As in sparse_batch.hip only the postings that hit
// are added: a miss would add +-0 to a sub-sum that is never -0.
//
// Grid (ceil(n / 16), B), 256 threads: 16 quarters, 16 listed documents of one query.
//
// Query image, built by every workgroup in LDS (sparse_batch.hip's rank dictionary for one
// query): dict uint2 {bits, base} per 32 terms (all 2,048 words: 16 KiB), weight f16 [q_top]
// in rank order.  Zero the bits; one LDS atomicOr per slot; a prefix sum of the popcounts,
// 8 words per thread; then "the highest slot of a repeated term wins" as an LDS atomicMax of
// the slot number per rank, and the slot that won writes f16(weight) at its rank.  A term
// outside 0 .. V - 1 is an empty slot.
//
// A posting costs one ds_read_b64 of its dictionary word and a bit test; a hit reads its
// weight and runs one fmaf.  A listed document is a cold gather: the quarter reads its
// (first unit, postings) entry and issues the loads of up to four units (one dword per lane
// each) before it consumes any, so up to four 64-byte lines per document are in flight; a
// longer document continues four units at a time.  An id outside [0, n_docs) or (MK: the
// instantiation a store with removals launches) one whose tombstone is set loads nothing.
#include "device_common.h"
#include "kernels.h"

namespace emb {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kQuarters = kThreads / 16;
constexpr int kWords = 2048;     // dictionary words of the largest vocabulary, 65,536 terms
constexpr int kMaxTop = 1024;    // slots of a query
constexpr int kRound = 4;        // units whose loads are issued together

template <bool MK>
__global__ __launch_bounds__(kThreads) void sparse_gather_kernel(const uint32_t *__restrict__ store,
                                                                 const int2 *__restrict__ table, int n_docs, int V,
                                                                 const int32_t *__restrict__ terms,
                                                                 const float *__restrict__ weights, int q_top,
                                                                 const int32_t *__restrict__ ids, int n,
                                                                 const uint32_t *__restrict__ tomb,
                                                                 float *__restrict__ scores)
{
    __shared__ uint2 dict[kWords];
    __shared__ int win[kMaxTop];
    __shared__ h16 wt[kMaxTop];
    __shared__ int wave_tot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = tid & 15, b = blockIdx.y;
    const int32_t *tp = terms + (size_t)b * q_top;
    const float *wp = weights + (size_t)b * q_top;

    // this quarter's document: its table entry is in flight under the image's build
    const int j = (int)blockIdx.x * kQuarters + (tid >> 4);
    const int32_t id = j < n ? ids[(size_t)b * n + j] : -1;
    bool ok = id >= 0 && id < n_docs;
    if constexpr (MK)
        if (ok) ok = !((tomb[id >> 5] >> (id & 31)) & 1u);
    int2 e = int2{0, 0};
    if (ok) e = table[id];

    for (int i = tid; i < kWords; i += kThreads) dict[i].x = 0u;
    for (int i = tid; i < q_top; i += kThreads) win[i] = -1;
    lds_barrier();
    for (int i = tid; i < q_top; i += kThreads) {
        const int32_t t = tp[i];
        if (t >= 0 && t < V) atomicOr(&dict[t >> 5].x, 1u << (t & 31));
    }
    lds_barrier();

    // exclusive prefix sum of the words' popcounts, 8 consecutive words per thread
    int c[8], inc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) inc += c[i] = __popc(dict[8 * tid + i].x);
    const int own = inc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_tot[wv] = inc;
    lds_barrier();
    int base = inc - own;
    for (int o = 0; o < wv; ++o) base += wave_tot[o];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        dict[8 * tid + i].y = (uint32_t)base;
        base += c[i];
    }
    lds_barrier();

    // rank of slot i's term: at most q_top distinct terms, so a rank is below q_top
    auto rank_of = [&](int32_t t) {
        const uint2 wd = dict[t >> 5];
        return (int)(wd.y + __popc(wd.x & ((1u << (t & 31)) - 1u)));
    };
    for (int i = tid; i < q_top; i += kThreads) {
        const int32_t t = tp[i];
        if (t >= 0 && t < V) atomicMax(&win[rank_of(t)], i);
    }
    lds_barrier();
    for (int i = tid; i < q_top; i += kThreads) {
        const int32_t t = tp[i];
        if (t >= 0 && t < V) {
            const int r = rank_of(t);
            if (win[r] == i) wt[r] = (h16)wp[i];
        }
    }
    lds_barrier();

    float acc = 0.f;
    const int units = (e.y + 15) >> 4;   // 0 for a masked id
    for (int u0 = 0; u0 < units; u0 += kRound) {
        uint32_t p[kRound];
#pragma unroll
        for (int i = 0; i < kRound; ++i) p[i] = u0 + i < units ? store[(size_t)(e.x + u0 + i) * 16 + l16] : 0u;
#pragma unroll
        for (int i = 0; i < kRound; ++i) {
            if (u0 + i >= units) break;
            const uint32_t term = p[i] & 0xffffu, bit = term & 31u;
            const uint2 wd = dict[term >> 5];
            if ((wd.x >> bit) & 1u) {
                const float w = (float)as_h((uint16_t)(p[i] >> 16));
                acc = fmaf((float)wt[wd.y + __popc(wd.x & ((1u << bit) - 1u))], w, acc);
            }
        }
    }
    float s = acc;
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
    if (l16 == 0 && j < n) scores[(size_t)b * n + j] = ok ? s : -INFINITY;
}

}  // namespace

int launch_sparse_score_ids(const uint32_t *store, const void *d_table, int n_docs, int V, const int32_t *d_terms,
                            const float *d_weights, int B, int q_top, const int32_t *d_ids, int n, float *d_scores,
                            hipStream_t s, const uint32_t *tomb)
{
    if (!store || !d_table || !d_terms || !d_weights || !d_ids || !d_scores || n_docs < 0 || V < 1 || V > 32 * kWords ||
        B < 1 || B > 64 || q_top < 1 || q_top > kMaxTop || n < 1 || n > 128)
        return -1;
    const dim3 grid((unsigned)((n + kQuarters - 1) / kQuarters), (unsigned)B);
    if (tomb)
        sparse_gather_kernel<true><<<grid, kThreads, 0, s>>>(store, (const int2 *)d_table, n_docs, V, d_terms, d_weights,
                                                             q_top, d_ids, n, tomb, d_scores);
    else
        sparse_gather_kernel<false><<<grid, kThreads, 0, s>>>(store, (const int2 *)d_table, n_docs, V, d_terms, d_weights,
                                                              q_top, d_ids, n, nullptr, d_scores);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
