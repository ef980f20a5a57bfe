// Binary storage of the embedding index (BERTX_INDEX_BIN, bert_hip.h "Binary storage";
// DESIGN.md 9e-3): a row is its d sign bits, a search is a Hamming scan with the top-k
// fused in.  The layout, the binarizer and the score are bin_bits.h's.
//
// The scan: a lane is one row.  Workgroup b walks the 64-row groups [b * per, (b + 1) *
// per); a group's NB = ceil(d / 128) blocks are NB global_load_dwordx4 of 1 KiB each,
// straight into registers, through a ring that keeps about 16 KiB in flight.  The bits
// of up to 64 queries are made once per workgroup and lie in LDS; they are wave-uniform,
// so every read of them is a broadcast.  The four waves of a workgroup divide the
// queries, not the rows: wave w owns queries w, w + 4, ... and their running lists
// (topk_list.h) and walks every group of the range for them (the three repeats of a
// group's loads come out of the caches; a wave without a query ends at once).  Per query
// and group a lane takes d / 32 xor + popcount-accumulate steps, holds the integer score
// of its own row, and offers it to the query's list: one LDS read of the list's k-th
// entry and a ballot, and only the lanes that beat it are inserted.  No score tile and
// no barrier inside the loop: a list has one owner.  The workgroups' lists go to the
// index's scratch as [query][P][k] and the f16 kernel's merge (launch_search_merge) folds
// them.
#include "bin_bits.h"
#include "kernels.h"
#include "topk_list.h"

#include <algorithm>

namespace emb {
namespace {

constexpr int kThreads = 256;          // 4 waves: each owns a quarter of the queries
constexpr int kLdsBudget = 160 * 1024;
constexpr int kGroupQueries = 64;      // queries of one launch
constexpr int kQueriesAhead = 4;       // prologue: queries of one wave whose loads are in flight together

__host__ __device__ inline size_t search_bin_lds_bytes(int nq, int NB, int k)
{
    return (size_t)nq * ((size_t)NB * 16 + (size_t)k * 8);
}

// Groups in flight per wave, R NB KiB: about 16 KiB, two to eight groups (with sixteen
// one-block groups the register allocator reused a slot in flight and the wait for it
// emptied the ring).
constexpr int ring_groups(int NB) { return 16 / NB > 8 ? 8 : 16 / NB > 2 ? 16 / NB : 2; }

// partial: [query][P][k].  Rows >= n_rows (the rest of the last group, stale rows after a
// clear, the groups a range has past the end) are never offered; loads past the last
// filled group are redirected to it, so they stay inside the allocation.
// Mask: nothing, the unmasked kernel; or one SearchMask, the masked kernel.
// A group's 64 tombstones and its 64 bits of a shared filter are one word pair each, wave-
// uniform, read through the scalar cache a group ahead; a group none of whose rows is
// admissible is left at once, before any Hamming distance.  Per-query filters are one
// vector load per group: lane 16h + i < 32 holds half h of query w + 4i's pair.  Word
// indices are clamped to the words that cover rows < n_rows (tombstones: to the last group).
template <int NB, class... Mask>
__global__ __launch_bounds__(kThreads) void search_bin_kernel(const uint4 *__restrict__ corpus,
                                                              const float *__restrict__ queries, int nq, int d,
                                                              int n_rows, int k, int per, Hit *__restrict__ partial,
                                                              Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    extern __shared__ uint4 smem[];
    constexpr int R = ring_groups(NB);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint4 *qb = smem;                                   // [nq][NB]
    Hit *lists = (Hit *)(qb + (size_t)nq * NB);         // [nq][k]

    // the bits of this wave's queries, kQueriesAhead queries' loads at a time
    for (int q0 = w; q0 < nq; q0 += 4 * kQueriesAhead) {
        float x0[kQueriesAhead][NB], x1[kQueriesAhead][NB];
#pragma unroll
        for (int i = 0; i < kQueriesAhead; ++i) {
            const float *x = queries + (size_t)min(q0 + 4 * i, nq - 1) * d;
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                x0[i][c] = x[128 * c + lane];
                x1[i][c] = 128 * c + 64 < d ? x[128 * c + 64 + lane] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < kQueriesAhead; ++i) {
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const uint4 v = bin_pack(__ballot(bin_positive(x0[i][c])), __ballot(bin_positive(x1[i][c])));
                if (lane == 0 && q0 + 4 * i < nq) qb[(size_t)(q0 + 4 * i) * NB + c] = v;
            }
        }
    }
    for (int i = tid; i < nq * k; i += kThreads) lists[i] = Hit{-INFINITY, -1};
    lds_barrier();
    if (w >= nq) return;   // (no barrier follows)

    const int G = (n_rows + 63) >> 6;
    const int g0 = blockIdx.x * per, g1 = min(g0 + per, G);
    const int last = max(G, 1) - 1;
    auto load = [&](int g, uint4 (&o)[NB]) {
        const uint4 *p = corpus + (size_t)min(g, last) * NB * 64 + lane;
#pragma unroll
        for (int c = 0; c < NB; ++c) o[c] = p[c * 64];
    };
    // masked: bit l = row 64 g + l is admissible as far as the tombstones and a shared filter say
    typedef const __attribute__((address_space(4))) uint32_t *WordPtr;
    const int last_word = max((n_rows + 31) >> 5, 1) - 1;
    const bool per_query = MK && m.filt && m.stride != 0;
    auto load_admissible = [&](int g) {
        const WordPtr tomb_c = (WordPtr)(uintptr_t)m.tomb, filt_c = (WordPtr)(uintptr_t)m.filt;
        const int w0 = 2 * min(g, last);
        uint64_t a = ~((uint64_t)tomb_c[w0] | (uint64_t)tomb_c[w0 + 1] << 32);
        if (m.filt && !per_query) a &= (uint64_t)filt_c[min(w0, last_word)] | (uint64_t)filt_c[min(w0 + 1, last_word)] << 32;
        return a;
    };
    uint64_t adm = 0;
    if constexpr (MK) adm = load_admissible(g0);
    // the ring is filled and refilled in the order it is consumed, so a group's loads are
    // always the oldest ones outstanding
    uint4 ring[R][NB];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        load(g0 + j, ring[j]);
        __builtin_amdgcn_sched_barrier(0);
    }
    for (int base = g0; base < g1; base += R) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int g = base + j;
            if (g >= g1) goto done;   // uniform; no path re-enters the ring out of order
            uint4 r[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) r[c] = ring[j][c];
            __builtin_amdgcn_sched_barrier(0);
            load(g + R, ring[j]);
            __builtin_amdgcn_sched_barrier(0);
            const int64_t row = (int64_t)g * 64 + lane;
            bool valid = row < n_rows;
            if constexpr (!MK) {
                for (int q = w; q < nq; q += 4) {
                    int ham = 0;
#pragma unroll
                    for (int c = 0; c < NB; ++c) ham = bin_distance(r[c], qb[(size_t)q * NB + c], ham);
                    list_offer(lists + (size_t)q * k, k, bin_score(d, ham), (int32_t)row, valid, lane);
                }
            } else {
                valid = valid && ((adm >> lane) & 1);
                adm = load_admissible(g + 1);
                if (__ballot(valid) == 0) continue;   // uniform: no row of the group for any of this wave's queries
                uint32_t fq = 0;                      // per-query filters: half lane >> 4 of query w + 4 (lane & 15)'s pair
                if (per_query && lane < 32 && w + 4 * (lane & 15) < nq)
                    fq = m.filt[(size_t)(w + 4 * (lane & 15)) * m.stride + min(2 * g + (lane >> 4), last_word)];
                for (int q = w, i = 0; q < nq; q += 4, ++i) {
                    int ham = 0;
#pragma unroll
                    for (int c = 0; c < NB; ++c) ham = bin_distance(r[c], qb[(size_t)q * NB + c], ham);
                    // (the shuffle by every lane, before any lane-dependent condition)
                    uint32_t fw = ~0u;
                    if (per_query) fw = (uint32_t)__shfl((int)fq, ((lane >> 5) << 4) | i, 64);   // (a uniform branch)
                    const bool ok = valid & (bool)((fw >> (lane & 31)) & 1u);
                    list_offer(lists + (size_t)q * k, k, bin_score(d, ham), (int32_t)row, ok, lane);
                }
            }
        }
    }
done:
    const int P = gridDim.x;
    for (int q = w; q < nq; q += 4)
        for (int j = lane; j < k; j += 64) partial[((size_t)q * P + blockIdx.x) * k + j] = lists[(size_t)q * k + j];
}

// rows f32 [n][d] -> bits at rows first .. first + n - 1; one wave per row, lane 0 stores
// the row's own 16 B of each block, so rows may start and end inside a group.
__global__ __launch_bounds__(256) void index_add_bin_kernel(const float *__restrict__ rows, int64_t n, int d,
                                                            int64_t first, uint4 *__restrict__ corpus)
{
    const int lane = threadIdx.x & 63, NB = (d + 127) >> 7;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c < NB) {
            const uint4 v = bin_chunk(rows + r * d, d, c, lane);
            if (lane == 0) corpus[bin_slot(first + r, NB, c)] = v;
        }
    }
}

// mask: none (the unmasked kernel) or the launch's SearchMask
template <int NB, class... Mask>
int launch_scan(const void *corpus, const float *Q, int nq, int d, int n_rows, int k, int per, int P, Hit *part,
                hipStream_t s, Mask... mask)
{
    search_bin_kernel<NB, Mask...><<<(unsigned)P, kThreads, search_bin_lds_bytes(nq, NB, k), s>>>(
        (const uint4 *)corpus, Q, nq, d, n_rows, k, per, part, mask...);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <class... Mask>
int launch_scan_of(int NB, const void *corpus, const float *Q, int nq, int d, int n_rows, int k, int per, int P, Hit *part,
                   hipStream_t s, Mask... mask)
{
    switch (NB) {
    case 1: return launch_scan<1>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    case 2: return launch_scan<2>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    case 3: return launch_scan<3>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    case 4: return launch_scan<4>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    case 5: return launch_scan<5>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    case 6: return launch_scan<6>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    case 7: return launch_scan<7>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    default: return launch_scan<8>(corpus, Q, nq, d, n_rows, k, per, P, part, s, mask...);
    }
}

template <int NB>
hipError_t allow_lds()
{
    hipError_t e = hipFuncSetAttribute((const void *)search_bin_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLdsBudget);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)search_bin_kernel<NB, SearchMask>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                kLdsBudget);
    return e;
}

}  // namespace

int search_bin_prepare_device()
{
    hipError_t e = allow_lds<1>();
    if (e == hipSuccess) e = allow_lds<2>();
    if (e == hipSuccess) e = allow_lds<3>();
    if (e == hipSuccess) e = allow_lds<4>();
    if (e == hipSuccess) e = allow_lds<5>();
    if (e == hipSuccess) e = allow_lds<6>();
    if (e == hipSuccess) e = allow_lds<7>();
    if (e == hipSuccess) e = allow_lds<8>();
    return e == hipSuccess ? 0 : -1;
}

size_t search_bin_image_bytes(int64_t capacity_rows, int d)
{
    return (size_t)((capacity_rows + 63) / 64) * (size_t)((d + 127) / 128) * 1024;
}

int64_t search_bin_max_workgroups(int64_t capacity_rows)
{
    const int64_t groups = (capacity_rows + 63) / 64;
    return std::max<int64_t>(1, std::min<int64_t>(2 * (int64_t)device_cu_count(), groups));
}

int launch_index_add_bin(const float *d_rows, int64_t n, int d, int64_t first, void *corpus, hipStream_t s)
{
    if (n <= 0 || d % 64 || d < 64 || d > 1024 || first < 0 || (n + 3) / 4 > 0x7fffffffll) return -1;
    index_add_bin_kernel<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(d_rows, n, d, first, (uint4 *)corpus);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_search_bin(const void *corpus, int64_t n_rows, int d, const float *d_queries, int B, int k, void *scratch,
                      float *d_scores, int32_t *d_ids, hipStream_t s, const SearchMask *mask)
{
    if (B < 1 || k < 1 || k > 128 || d % 64 || d < 64 || d > 1024 || n_rows < 0 || n_rows > 0x7ffffff0) return -1;
    if (mask && !mask->tomb) return -1;
    const int NB = (d + 127) / 128;
    const int64_t groups = std::max<int64_t>(1, (n_rows + 63) / 64);
    const int cus = device_cu_count();
    for (int b0 = 0; b0 < B; b0 += kGroupQueries) {
        const int nq = std::min(kGroupQueries, B - b0);
        const size_t lds = search_bin_lds_bytes(nq, NB, k);
        const int64_t per_cu = std::min<int64_t>(2, (int64_t)kLdsBudget / (int64_t)lds);
        int64_t P = std::max<int64_t>(1, std::min<int64_t>(per_cu * cus, groups));
        const int64_t per = (groups + P - 1) / P;
        P = (groups + per - 1) / per;
        const float *Q = d_queries + (size_t)b0 * d;
        int rc;
        if (mask) {
            // this launch's filters; an empty index has no row to admit and its filters may have no word
            SearchMask gm = *mask;
            if (n_rows == 0) gm.filt = nullptr;
            if (gm.filt) gm.filt += (size_t)b0 * (size_t)gm.stride;
            rc = launch_scan_of(NB, corpus, Q, nq, d, (int)n_rows, k, (int)per, (int)P, (Hit *)scratch, s, gm);
        } else {
            rc = launch_scan_of(NB, corpus, Q, nq, d, (int)n_rows, k, (int)per, (int)P, (Hit *)scratch, s);
        }
        if (rc != 0) return rc;
        rc = launch_search_merge(scratch, nq, (int)P, k, d_scores + (size_t)b0 * k, d_ids + (size_t)b0 * k, s);
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace emb
