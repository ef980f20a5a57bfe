// One definition of the token store's MaxSim arithmetic and launch rule,
// shared by the scorers (maxsim.hip, maxsim_i8.hip, maxsim_res.hip), the scans
// (maxsim_search.hip, maxsim_approx.hip) and the coder (maxsim_codes.hip).  Every scan
// promises the scorers' score bit for bit; the pieces of a score that do not depend on how a
// kernel streams its rows live here, so that the promise rests on one text: the storage
// kinds and their MFMA, the sim of an accumulator, the query prologue, the document
// epilogue, the quad fetch of the rows' u, the table access of the scans and the pack
// kernels' row lookup; and for the host the LDS budget, the grid rules and the QT dispatch.
// The row normalisers stay in maxsim_pack.h, which this header builds on: they are the
// store's number format and know nothing of tiles, lanes' roles or launches.
#pragma once

#include "device_common.h"
#include "kernels.h"
#include "maxsim_pack.h"

#include <algorithm>
#include <type_traits>

namespace emb {

// What differs between the storage kinds (search.hip Store): the 16-B lane fragment of a
// 1-KiB block, the accumulator, the k a block covers (w >> kShift blocks per group) and the
// bytes of a row.
template <int ST> struct Kind;
template <> struct Kind<SEARCH_F16> {
    typedef h16x8 Block;
    typedef f32x4 Acc;
    static constexpr int kShift = 5;
    __host__ __device__ static constexpr size_t row_bytes(int w) { return (size_t)w * 2; }
};
template <> struct Kind<SEARCH_I8> {
    typedef i32x4 Block;
    typedef i32x4 Acc;
    static constexpr int kShift = 6;
    __host__ __device__ static constexpr size_t row_bytes(int w) { return (size_t)w; }
};

// One block of 16 stored rows (a) against one block of 16 query rows (b): accumulator
// register r of lane 16g + c is (row 4g + r, query c).
__device__ __forceinline__ f32x4 mma(h16x8 a, h16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ i32x4 mma(i32x4 a, i32x4 b, i32x4 c)
{
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}

// sim of one accumulator element after a group's last block: the f32 accumulator itself
// (f16), score_i8 of the exact int32 sum with the query's and the row's u (int8).
__device__ __forceinline__ float sim(float acc, float, float) { return acc; }
__device__ __forceinline__ float sim(int acc, float uq, float urow) { return score_i8(acc, uq, urow); }

// The query prologue of a workgroup of four waves, wave wv of them one row at a time: NQ
// queries of QTq tiles each, q f32 [NQ][Lq][w], into B fragments qf [NQ QTq][KB][64] in LDS:
// tile t = QTq * (query of the pass) + (tile of the query), lane 16g + c of block (t, kb) =
// row 16 (tile of the query) + c of that query, elements 32kb + 8g .. + 7 (f16) or bytes
// 64kb + 16g .. + 15 (int8).  The rows go through pack_row_f16 / pack_row_i8, the
// normalisers of the stored rows; rows Lq .. 16 QTq - 1 of a query are zeros.  int8: the
// rows' u go to qu [16 NQ QTq], 0 for a row past Lq; f16 never touches qu.  The caller's
// barrier follows.  NQ = 1 is the scorers' prologue (row i of the query is row i of tile
// i / 16).  NQ and QTq are ints, or Tiles<n> where the kernel has them as template
// parameters: the counts are then constants while this function is compiled on its own
// (as plain ints they cost maxsim_res_kernel<1, NB> two registers).  maxsim_kernel and
// maxsim_search_kernel keep this loop written out: DESIGN.md 9g-7.
template <int N> using Tiles = std::integral_constant<int, N>;
template <int ST, class TNQ, class TQT>
__device__ __forceinline__ void pack_queries(const float *__restrict__ q, TNQ NQ, TQT QTq, int Lq, int w,
                                             typename Kind<ST>::Block *qf, float *qu, int wv, int lane)
{
    const int KB = w >> Kind<ST>::kShift;
    for (int i = wv; i < NQ * QTq * 16; i += 4) {
        const int qi = (i >> 4) / QTq, rq = i - 16 * qi * QTq;         // the query of the pass, its row
        const float *src = q + ((size_t)qi * Lq + rq) * w;            // read for rq < Lq only
        if constexpr (ST == SEARCH_F16) {
            h16x8 v[2] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
            if (rq < Lq) pack_row_f16(src, w, lane, v);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = lane + 64 * j;
                if (c < (w >> 3)) qf[frag_index(i, c, KB)] = v[j];
            }
        } else {
            i32x4 v = {0, 0, 0, 0};
            float u = 0.f;
            if (rq < Lq) v = pack_row_i8(src, w, lane, u);
            if (lane < (w >> 4)) qf[frag_index(i, lane, KB)] = v;
            if (lane == 0) qu[i] = u;
        }
    }
}

// The document epilogue.  mx[t]: this lane's running maximum over its rows 4g .. 4g + 3 of
// every group of the document against query row 16t + c (lane 16g + c), -inf where it saw
// none.  Two shuffles per tile fold the four g, which makes the max over the document
// exact; lane c then adds its columns c, 16 + c, ... in ascending t from +0 (a column past
// Lq adds +0) and the butterfly 8, 4, 2, 1 adds the 16 lanes: the order is fixed by Lq
// alone.  Every lane of a 16-lane row ends with the score; the callers take lane 0's.
template <int QT>
__device__ __forceinline__ float doc_score(const float *mx, int Lq, int lane)
{
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float m = mx[t];
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        s = __fadd_rn(s, 16 * t + (lane & 15) < Lq ? m : 0.f);
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
    return s;
}

// The u of a group's rows out of a ring dword (int8): lane 16g + c loaded the u of row
// 4g + (c & 3), so rows 4g .. 4g + 3, the rows of this lane's accumulator registers, sit in
// lanes 0 .. 3 of its own quad and come out by four DPP moves.
__device__ __forceinline__ void quad_u(float ring_u, float (&rrow)[4])
{
    const int ug = __float_as_int(ring_u);
    rrow[0] = __int_as_float(__builtin_amdgcn_mov_dpp(ug, 0x00, 0xf, 0xf, false));
    rrow[1] = __int_as_float(__builtin_amdgcn_mov_dpp(ug, 0x55, 0xf, 0xf, false));
    rrow[2] = __int_as_float(__builtin_amdgcn_mov_dpp(ug, 0xaa, 0xf, 0xf, false));
    rrow[3] = __int_as_float(__builtin_amdgcn_mov_dpp(ug, 0xff, 0xf, 0xf, false));
}

// The scans read the table in the constant address space: it does not change during a
// search and every index into it is wave-uniform, so it comes through the scalar cache
// and never enters the vector-memory counter that paces the ring (search.hip's row scales).
typedef const __attribute__((address_space(4))) int2 *TablePtr;

// The first document in [0, n_docs) whose first group is >= g, n_docs if none: the table's
// first groups ascend with the id.
__device__ __forceinline__ int first_doc_at(TablePtr tab, int n_docs, int g)
{
    int lo = 0, hi = n_docs;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].x < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The document masks of the masked scans (bert_hip.h "Deleting documents and filtered
// search"): kernels.h SearchMask with a document in the place of a row.  A
// document is wave-uniform in the scans, so its mask words are too, and come as the table
// does: through the constant address space.
typedef const __attribute__((address_space(4))) uint32_t *MaskPtr;

// a[i], i < nq <= N: the admissible word of query i of the pass (m.filt points at the pass's
// first filter) for the 32 documents around `doc`: ~tombstones & filter, the tombstones alone
// without a filter.  doc < n_docs: the words past ceil(n_docs / 32) are never indexed.
template <int N>
__device__ __forceinline__ void admit_words(const SearchMask &m, int nq, int doc, uint32_t (&a)[N])
{
    const MaskPtr tomb = (MaskPtr)(uintptr_t)m.tomb, filt = (MaskPtr)(uintptr_t)m.filt;
    const uint32_t live = ~tomb[doc >> 5];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i >= nq) break;
        a[i] = m.filt ? live & filt[(int64_t)i * m.stride + (doc >> 5)] : live;
    }
}

// Bit i of the result: query i of the pass admits `doc`, by the words admit_words gave for it.
template <int N>
__device__ __forceinline__ int admit_bits(const uint32_t (&a)[N], int nq, int doc)
{
    int ok = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i >= nq) break;
        ok |= (int)((a[i] >> (doc & 31)) & 1u) << i;
    }
    return ok;
}

// The scorers' test of a candidate under tombstones: the bit of an id in [0, n_docs).
__device__ __forceinline__ bool doc_deleted(const uint32_t *tomb, int id)
{
    return (((MaskPtr)(uintptr_t)tomb)[id >> 5] >> (id & 31)) & 1u;
}

// The document of source row t of an add call: src_off[i] (i < n_new, ascending,
// src_off[0] = 0) is the first source row of the call's i-th document, and row t belongs to
// the last document d whose src_off is <= t.  With table[d] = (first group, len) the row
// goes to slot 16 first + (t - src_off[d]).
__device__ __forceinline__ int source_doc(const int32_t *__restrict__ src_off, int n_new, int64_t t)
{
    int lo = 0, hi = n_new - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)src_off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the host side ----

// The dynamic LDS every token-store kernel may ask for, of the CU's 160 KiB.
constexpr int kLdsBudget = 160 * 1024;
constexpr int kMaxWgPerCu = 4;     // 16 waves of 8 KiB in flight per CU (approx_scan: up to 32 waves)
constexpr int kScanMaxWg = 1024;   // the scans' grid cap: two selection levels cover 1,024 lists

inline hipError_t allow_lds(const void *kernel)
{
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
}

// as many workgroups per CU as the LDS holds, at most kMaxWgPerCu
inline int64_t wg_per_cu(size_t lds)
{
    return std::max<int64_t>(1, std::min<int64_t>(kMaxWgPerCu, (int64_t)kLdsBudget / (int64_t)lds));
}

// max_wg > 0 caps the grid (the tests' way to many documents per wave); *ran_wg gets the result
inline int capped_grid(int64_t P, int max_wg, int *ran_wg)
{
    P = std::max<int64_t>(1, P);
    if (max_wg > 0) P = std::min<int64_t>(P, max_wg);
    if (ran_wg) *ran_wg = (int)P;
    return (int)P;
}

// The scorers' grid of persistent workgroups of four waves over n candidates: never more
// waves than candidates.
inline int scorer_grid(size_t lds, int n, int max_wg, int *ran_wg)
{
    return capped_grid(std::min<int64_t>(wg_per_cu(lds) * device_cu_count(), ((int64_t)n + 3) / 4), max_wg, ran_wg);
}

// The lists a scan may write per query, which sizes the scans' scratch (maxsim_search_scratch_bytes).
inline int scan_max_lists() { return std::min(kMaxWgPerCu * device_cu_count(), kScanMaxWg); }

// The scans' grid of workgroups of `waves` waves over the store's G groups: never more
// waves than groups, never more workgroups than the selection and the scratch take.
inline int scan_grid(size_t lds, int G, int waves, int max_wg, int *ran_wg)
{
    return capped_grid(std::min<int64_t>(std::min<int64_t>(wg_per_cu(lds) * device_cu_count(), scan_max_lists()),
                                         ((int64_t)G + waves - 1) / waves),
                       max_wg, ran_wg);
}

// f(Tiles<n>) for n = 1 .. 4 (the tiles of a query, the queries of a
// pass); like the switches it replaces, a larger n takes 4.
template <class F>
inline void with_tiles(int n, F &&f)
{
    switch (n) {
    case 1: f(Tiles<1>{}); break;
    case 2: f(Tiles<2>{}); break;
    case 3: f(Tiles<3>{}); break;
    default: f(Tiles<4>{}); break;
    }
}

}  // namespace emb
