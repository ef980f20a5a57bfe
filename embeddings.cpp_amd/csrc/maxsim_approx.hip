// Centroid interaction over the token store's codes (bertx_mvindex_candidates*,
// bertx_mvindex_search_pruned*, bert_hip.h "Pruned search"; mvindex.cpp):
// the first stage of a pruned MaxSim search.  Per pass of up to four 16-row query tiles
// (4, 2, 1 or 1 whole queries, the full scan's packing):
//   table:  T[c][16 t + r] = sim(query row r of tile t, centroid c), the scorers' MFMA
//           sequence with the centroids in the stored-row role, f32 [C][16, 32 or 64] (three
//           tiles take a line of four), so that one code selects one contiguous line;
//   scan:   approx(q, doc) = sum_i max_{j < len} T[code_j][i] over every document, 2 bytes
//           per token slot instead of the stored row, the per-wave lists of the full scan;
//   select: the n_cand best of the workgroups' sorted lists, by merging them.
// approx(q, doc) is, bit for bit, the scorers' score of q on a document whose rows are the
// centroids cent[code_j]: the same sims, the exact max, lane c's sum of its query's
// columns c, 16 + c, ... in ascending order from +0 (a row >= Lq adds +0) and the
// four-step butterfly.  One wave scores one whole document.
#include "maxsim_common.h"
#include "topk_list.h"

namespace emb {
namespace {

constexpr int kTableThreads = 256;  // 4 waves, each takes one centroid group
constexpr int kScanThreads = 512;   // 8 waves share one copy of the table in LDS
constexpr int kScanWaves = kScanThreads / 64;
// (kMaxWgPerCu workgroups of it: up to 32 waves per CU where the table leaves the LDS for it)

// The floats of one line of the table: 16 per tile, three tiles padded to four, so that a
// code becomes an address by a shift.
__host__ __device__ inline int line_floats(int TT) { return TT == 3 ? 64 : 16 * TT; }

template <int ST>
__host__ __device__ inline size_t table_lds_bytes(int TT, int w)
{
    return (size_t)TT * 16 * Kind<ST>::row_bytes(w) + 64 * 4;
}

// NQ queries of QTq tiles each, q f32 [NQ][Lq][w], TT = QTq NQ <= 4 tiles.  The prologue is
// the scorers' (maxsim_common.h pack_queries): tile t = QTq * (query of the pass) + (tile of
// the query).  Wave v of the
// grid takes centroid group v: its blocks in ascending k against every tile from zero
// accumulators; accumulator register r of lane 16g + c is (centroid 16 cg + 4g + r, query
// row c of tile t) and goes to T[centroid][16 t + c].
template <int ST>
__global__ __launch_bounds__(kTableThreads) void approx_table_kernel(const typename Kind<ST>::Block *__restrict__ cent,
                                                                     const float *__restrict__ cent_u, int C,
                                                                     const float *__restrict__ q, int QTq, int NQ,
                                                                     int Lq, int w, float *__restrict__ T)
{
    typedef Kind<ST> S;
    typedef typename S::Block Block;
    typedef typename S::Acc Acc;
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int KB = w >> S::kShift, TT = QTq * NQ, LINE = line_floats(TT);
    Block *qf = (Block *)smem;                                    // [TT][KB][64]
    float *qu = (float *)(qf + (size_t)TT * KB * 64);             // [64]

    pack_queries<ST>(q, NQ, QTq, Lq, w, qf, qu, wv, lane);
    lds_barrier();

    const int cg = (int)blockIdx.x * 4 + wv;
    if (cg >= (C >> 4)) return;
    const int g4 = lane >> 4, c = lane & 15;
    const Block *a = cent + (size_t)cg * KB * 64 + lane;
    Acc acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = Acc{0, 0, 0, 0};
    for (int kb = 0; kb < KB; ++kb) {
        const Block av = a[(size_t)kb * 64];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < TT) acc[t] = mma(av, qf[((size_t)t * KB + kb) * 64 + lane], acc[t]);
    }
    float4 ur = {0.f, 0.f, 0.f, 0.f};
    if constexpr (ST == SEARCH_I8) ur = *(const float4 *)(cent_u + 16 * cg + 4 * g4);
    const float urow[4] = {ur.x, ur.y, ur.z, ur.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t >= TT) break;
        float uq = 0.f;
        if constexpr (ST == SEARCH_I8) uq = qu[16 * t + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) T[(size_t)(16 * cg + 4 * g4 + r) * LINE + 16 * t + c] = sim(acc[t][r], uq, urow[r]);
    }
}

__host__ __device__ inline size_t scan_list_bytes(int NQ, int n_cand) { return (size_t)kScanWaves * NQ * n_cand * sizeof(Hit); }

// The documents are dealt to the grid's waves as maxsim_search_kernel deals them: wave v of
// W takes those whose first group lies in [v G / W, (v + 1) G / W), one contiguous run of
// groups (maxsim_common.h first_doc_at).  Lane l stands for column min(l, 16 TT - 1) of the table's lines: query row l & 15
// of tile l >> 4.  The run's codes come 128 at a time, one dword (two codes) per lane, the
// load after next always in flight (loads past the run re-read its last dword); a group's
// eight dwords are read out of the lanes into scalar registers, so a code is wave-uniform
// and its line is one contiguous read, free of bank conflicts in LDS.  The lane folds the
// line's value into its running max; slots past len select -inf (their code is 0, a valid
// line).  The wave-uniform test rbase + 16 >= len closes the document: the scorers'
// epilogue over the lanes' maxima for all queries of the pass at once (the xor steps 8, 2
// and 1 are DPP moves inside the row of 16 lanes), each score parked in lane `npend`, the
// lists offered when 64 are pending and at the end.  Then one barrier, wave i folds the waves'
// lists of query i and writes partial [query][P][n_cand].
// LDS_T: the table is first copied into LDS, [C][LINE] behind the lists; else the lookups
// read it from global memory.  The values, and so the results, are the same.
// Mask: nothing, the unmasked kernel, whose arguments end at partial; or one SearchMask over
// documents (filt at the pass's first filter), the masked kernel: maxsim_search_kernel's
// change at the document close, for either placement of the table.
template <bool LDS_T, class... Mask>
__global__ __launch_bounds__(kScanThreads) void approx_scan_kernel(const uint32_t *__restrict__ codes,
                                                                   const int2 *__restrict__ table, int n_docs, int G,
                                                                   const float *__restrict__ T, int C, int QTq, int NQ,
                                                                   int Lq, int n_cand, Hit *__restrict__ partial,
                                                                   Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int TT = QTq * NQ, LINE = line_floats(TT);
    const int shift = LINE == 64 ? 8 : LINE == 32 ? 7 : 6;        // a line's bytes = 1 << shift
    Hit *lists = (Hit *)smem;                                     // [kScanWaves][NQ][n_cand]
    const float *tl = (const float *)((const char *)smem + ((scan_list_bytes(NQ, n_cand) + 15) & ~(size_t)15));
    for (int i = tid; i < kScanWaves * NQ * n_cand; i += kScanThreads) lists[i] = Hit{-INFINITY, -1};
    if constexpr (LDS_T) {
        const float4 *src = (const float4 *)T;
        float4 *dst = (float4 *)tl;
        for (int i = tid; i < C * LINE / 4; i += kScanThreads) dst[i] = src[i];
    }
    lds_barrier();

    const int ws = __builtin_amdgcn_readfirstlane(wv);
    Hit *mine = lists + (size_t)ws * NQ * n_cand;
    const TablePtr tab = (TablePtr)(uintptr_t)table;
    const int64_t W = (int64_t)gridDim.x * kScanWaves, v = (int64_t)blockIdx.x * kScanWaves + ws;
    const int dA = first_doc_at(tab, n_docs, (int)(v * G / W));
    const int dB = first_doc_at(tab, n_docs, (int)((v + 1) * G / W));

    if (dA < dB) {   // wave-uniform
        const int gA = tab[dA].x, gB = dB < n_docs ? tab[dB].x : G;
        const int Gw = gB - gA;
        const uint32_t *cw = codes + (size_t)gA * 8;              // 8 dwords of codes per group
        const int last_dw = Gw * 8 - 1;
        const int col4 = 4 * min(lane, LINE - 1), qrow = lane & 15;
        auto load = [&](int chunk) { return cw[min(chunk * 64 + lane, last_dw)]; };
        // a code is below C: the assign kernel writes indices of centroids and 0 only
        auto look = [&](uint32_t code) {
            const uint32_t at = (code << shift) + (uint32_t)col4;
            if constexpr (LDS_T) return *(const float *)((const char *)tl + at);
            else return *(const float *)((const char *)T + at);
        };
        // the close's operands, constant per lane: tile t of this lane's query sits 16 t lanes
        // behind the query's first tile; it counts when the query has the tile and the row
        int src_lane[4];
        bool counts[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int first = ((lane >> 4) / QTq) * QTq;
            src_lane[t] = 16 * min(first + t, 3) + qrow;
            counts[t] = t < QTq && 16 * t + qrow < Lq;
        }
        uint32_t c0 = load(0), c1 = load(1);
        float mx = -INFINITY;
        int id = dA, len = tab[dA].y, len_next = tab[min(dA + 1, n_docs - 1)].y, rbase = 0;
        float ps[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int pid = -1, npend = 0;
        // masked: the admissible words of the open document and of the one behind it; per lane
        // the parked document's bit per query
        uint32_t aw[4] = {}, an[4] = {};
        int pok = 0;
        if constexpr (MK) {
            admit_words<4>(m, NQ, dA, aw);
            admit_words<4>(m, NQ, min(dA + 1, n_docs - 1), an);
        }
        auto flush = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (MK) {
                    if (i < NQ) list_offer(mine + (size_t)i * n_cand, n_cand, ps[i], pid, lane < npend && ((pok >> i) & 1), lane);
                } else {
                    if (i < NQ) list_offer(mine + (size_t)i * n_cand, n_cand, ps[i], pid, lane < npend, lane);
                }
            }
            npend = 0;
        };
        // the group whose codes are dwords 8 gi .. 8 gi + 7 of `cur`
        auto group = [&](uint32_t cur, int gi) {
            const int nv = len - rbase;                           // wave-uniform, >= 1
            if (nv >= 16) {
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)cur, 8 * gi + jj);
                    const float v0 = look(d & 0xffffu), v1 = look(d >> 16);
                    mx = fmaxf(mx, v0);
                    mx = fmaxf(mx, v1);
                }
            } else {
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)cur, 8 * gi + jj);
                    const float v0 = look(d & 0xffffu), v1 = look(d >> 16);
                    mx = fmaxf(mx, 2 * jj < nv ? v0 : -INFINITY);
                    mx = fmaxf(mx, 2 * jj + 1 < nv ? v1 : -INFINITY);
                }
            }
            if (rbase + 16 >= len) {   // wave-uniform: the document's last group
                // Every query of the pass at once, each in the lanes of its first tile: the
                // lane of row c adds its query's maxima of rows c, 16 + c, ... from +0 (a tile
                // or row the query does not have adds +0 once more, which changes no bit of a
                // sum that started from +0), then the butterfly 8, 4, 2, 1 inside the 16 lanes.
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float m = __shfl(mx, src_lane[t], 64);
                    s = __fadd_rn(s, counts[t] ? m : 0.f);
                }
                s = __fadd_rn(s, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0x128, 0xf, 0xf, true)));   // ^ 8
                s = __fadd_rn(s, __shfl_xor(s, 4, 64));
                s = __fadd_rn(s, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0x4e, 0xf, 0xf, true)));    // ^ 2
                s = __fadd_rn(s, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s), 0xb1, 0xf, 0xf, true)));    // ^ 1
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i >= NQ) break;
                    // the first lane of query i's first tile holds its score
                    const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 16 * QTq * i));
                    ps[i] = lane == npend ? s0 : ps[i];
                }
                pid = lane == npend ? id : pid;
                if constexpr (MK) {
                    const int ok = admit_bits<4>(aw, NQ, id);   // bit i: query i of the pass admits the document
                    pok = lane == npend ? ok : pok;
                    npend += ok != 0;                           // no query admits it: the lane is taken again
                } else {
                    ++npend;
                }
                ++id;
                mx = -INFINITY;
                len = len_next;
                len_next = tab[min(id + 1, n_docs - 1)].y;
                if constexpr (MK) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) aw[i] = an[i];
                    // wave-uniform: the document behind the one that opens starts a word
                    if (((id + 1) & 31) == 0 && id + 1 < n_docs) admit_words<4>(m, NQ, id + 1, an);
                }
                rbase = 0;
                if (npend == 64) flush();
            } else {
                rbase += 16;
            }
        };
        for (int ch = 0; ch * 8 < Gw; ++ch) {
            const uint32_t cur = c0;
            c0 = c1;
            c1 = load(ch + 2);
#pragma unroll
            for (int gi = 0; gi < 8; ++gi) {
                if (ch * 8 + gi >= Gw) break;   // wave-uniform
                group(cur, gi);
            }
        }
        flush();
    }
    lds_barrier();

    if (ws < NQ) {
        Hit *dst = lists + ((size_t)ws * NQ + ws) * n_cand;
        for (int o = 0; o < kScanWaves; ++o) {
            if (o == ws) continue;
            const Hit *src = lists + ((size_t)o * NQ + ws) * n_cand;
            Hit e0{-INFINITY, -1}, e1{-INFINITY, -1};
            if (lane < n_cand) e0 = src[lane];
            if (lane + 64 < n_cand) e1 = src[lane + 64];
            list_offer(dst, n_cand, e0.s, e0.id, lane < n_cand && e0.id >= 0, lane);
            list_offer(dst, n_cand, e1.s, e1.id, lane + 64 < n_cand && e1.id >= 0, lane);
        }
        Hit *out = partial + ((size_t)ws * gridDim.x + blockIdx.x) * n_cand;
        for (int j = lane; j < n_cand; j += 64) out[j] = dst[j];
    }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x)
{
    x = min(x, (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xb1, 0xf, 0xf, true));
    x = min(x, (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4e, 0xf, 0xf, true));
    x = min(x, (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x141, 0xf, 0xf, true));
    x = min(x, (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x140, 0xf, 0xf, true));
    return min(min((uint32_t)__builtin_amdgcn_readlane((int)x, 0), (uint32_t)__builtin_amdgcn_readlane((int)x, 16)),
               min((uint32_t)__builtin_amdgcn_readlane((int)x, 32), (uint32_t)__builtin_amdgcn_readlane((int)x, 48)));
}

constexpr int kMergeSeg = 32;       // lists one wave merges: 32 * 128 pairs = 32 KiB of LDS

// The k best of a query's lists by merging: the scan's lists are sorted by `better` (fill
// last), so the k best of P of them are k pops from their heads.  Workgroup (q, y), one
// wave, copies the lists y seg .. y seg + seg - 1 of query q into LDS; lane l holds the head
// of list l; per pop the best head is the highest score (wave_max_f32, exact) and among its
// lanes the lowest unsigned id, which is `better`; that lane moves on to its list's next
// entry, the fill behind the last.  The result is that of sorting all the pairs, which is
// what the full scan's select_kernel does with its unsorted blocks; here a pop costs a few
// dozen instructions where a sort of 32 lists costs 66 barrier stages (52 us measured).
// Written to hits [q][gridDim.y][k] when given (the first level), else to scores / ids [q][k].
__global__ __launch_bounds__(64) void merge_select_kernel(const Hit *__restrict__ partial, int all_P, int k, int seg,
                                                          Hit *__restrict__ hits, float *__restrict__ scores,
                                                          int32_t *__restrict__ ids)
{
    __shared__ Hit s[kMergeSeg * 128];
    const int lane = threadIdx.x, q = blockIdx.x;
    const int p0 = (int)blockIdx.y * seg, P = min(all_P - p0, seg), n = P * k;
    const Hit *src = partial + ((size_t)q * all_P + p0) * k;
    for (int i = lane; i < n; i += 64) s[i] = src[i];
    __syncthreads();
    int pos = 0;
    Hit head{-INFINITY, -1};
    if (lane < P) head = s[lane * k];
    for (int j = 0; j < k; ++j) {
        const float m = wave_max_f32(head.s);
        const uint32_t mine = head.s == m ? (uint32_t)head.id : 0xffffffffu;
        const uint32_t id = wave_min_u32(mine);
        const unsigned long long win = __ballot(head.s == m && (uint32_t)head.id == id);
        const int wl = win ? __builtin_ctzll(win) : 0;            // (no winner: a NaN score; lane 0's head then)
        const float ws = __shfl(head.s, wl, 64);
        const int32_t wi = __shfl(head.id, wl, 64);
        if (lane == 0) {
            if (hits) {
                hits[((size_t)q * gridDim.y + blockIdx.y) * k + j] = Hit{ws, wi};
            } else {
                scores[(size_t)q * k + j] = ws;
                ids[(size_t)q * k + j] = wi;
            }
        }
        if (lane == wl && lane < P) {
            ++pos;
            head = pos < k ? s[lane * k + pos] : Hit{-INFINITY, -1};
        }
    }
}

// One workgroup per query: the k best of its n_cand <= 128 (exact score, id) pairs by
// `better`, each pair placed by the count of pairs that come before it.  Pairs with id -1
// are the fill (-inf, -1), equal among themselves, and are ordered by their position.
__global__ __launch_bounds__(128) void rerank_select_kernel(const float *__restrict__ exact,
                                                            const int32_t *__restrict__ ids, int n_cand, int k,
                                                            float *__restrict__ out_s, int32_t *__restrict__ out_i)
{
    __shared__ Hit s[128];
    const int tid = threadIdx.x, q = blockIdx.x;
    Hit e{-INFINITY, -1};
    if (tid < n_cand) {
        const int32_t id = ids[(size_t)q * n_cand + tid];
        if (id >= 0) e = Hit{exact[(size_t)q * n_cand + tid], id};
    }
    s[tid] = e;
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < 128; ++j) {
        const Hit o = s[j];
        rank += better(o.s, o.id, e.s, e.id) || (o.s == e.s && o.id == e.id && j < tid);
    }
    if (rank < k) {
        out_s[(size_t)q * k + rank] = e.s;
        out_i[(size_t)q * k + rank] = e.id;
    }
}

template <int ST>
int launch_table(const void *cent, const float *cent_u, int C, const float *Q, int QTq, int nq, int Lq, int w, float *T,
                 hipStream_t s)
{
    const size_t lds = table_lds_bytes<ST>(QTq * nq, w);
    if (lds > (size_t)kLdsBudget) return -1;
    typedef typename Kind<ST>::Block Block;
    approx_table_kernel<ST><<<(unsigned)((C / 16 + 3) / 4), kTableThreads, lds, s>>>((const Block *)cent, cent_u, C, Q, QTq,
                                                                                     nq, Lq, w, T);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int maxsim_approx_prepare_device()
{
    hipError_t e = allow_lds((const void *)approx_table_kernel<SEARCH_F16>);
    if (e == hipSuccess) e = allow_lds((const void *)approx_table_kernel<SEARCH_I8>);
    if (e == hipSuccess) e = allow_lds((const void *)approx_scan_kernel<true>);
    if (e == hipSuccess) e = allow_lds((const void *)approx_scan_kernel<false>);
    if (e == hipSuccess) e = allow_lds((const void *)approx_scan_kernel<true, SearchMask>);
    if (e == hipSuccess) e = allow_lds((const void *)approx_scan_kernel<false, SearchMask>);
    return e == hipSuccess ? 0 : -1;
}

int launch_maxsim_candidates(const uint16_t *codes, const void *d_table, int n_docs, int64_t used_groups, int storage,
                             int w, const void *cent, const float *cent_u, int C, const float *d_q, int nq, int Lq,
                             int n_cand, float *tscratch, void *scratch, float *d_approx, int32_t *d_ids, int stages,
                             int *form, hipStream_t s, int max_wg, int *ran_wg, const SearchMask *mask)
{
    if (Lq < 1 || Lq > 64 || n_cand < 1 || n_cand > 128 || n_docs < 0 || used_groups < 0 || used_groups > 0x7ffffff0ll ||
        w % 64 || w < 64 || w > 1024 || C < 16 || C > 65536 || C % 16 || !codes || !cent || !tscratch || !scratch)
        return -1;
    if (mask && !mask->tomb) return -1;
    if ((storage != SEARCH_F16 && storage != SEARCH_I8) || (storage == SEARCH_I8 && !cent_u)) return -1;
    const int QTq = (Lq + 15) / 16;
    if (nq < 1 || nq * QTq > 4) return -1;
    if (stages & 1) {
        const int rc = storage == SEARCH_I8 ? launch_table<SEARCH_I8>(cent, cent_u, C, d_q, QTq, nq, Lq, w, tscratch, s)
                                            : launch_table<SEARCH_F16>(cent, nullptr, C, d_q, QTq, nq, Lq, w, tscratch, s);
        if (rc != 0) return rc;
    }
    if (!(stages & 2)) return 0;
    const int G = (int)used_groups;
    const size_t lists = (scan_list_bytes(nq, n_cand) + 15) & ~(size_t)15;
    const size_t tbytes = (size_t)4 * line_floats(QTq * nq) * C;
    const bool in_lds = lists + tbytes <= (size_t)kLdsBudget;
    const size_t lds = in_lds ? lists + tbytes : lists;
    const int P = scan_grid(lds, G, kScanWaves, max_wg, ran_wg);   // the full scan's rule, which sized the scratch
    if (mask && in_lds)
        approx_scan_kernel<true, SearchMask><<<(unsigned)P, kScanThreads, lds, s>>>(
            (const uint32_t *)codes, (const int2 *)d_table, n_docs, G, tscratch, C, QTq, nq, Lq, n_cand, (Hit *)scratch, *mask);
    else if (mask)
        approx_scan_kernel<false, SearchMask><<<(unsigned)P, kScanThreads, lds, s>>>(
            (const uint32_t *)codes, (const int2 *)d_table, n_docs, G, tscratch, C, QTq, nq, Lq, n_cand, (Hit *)scratch, *mask);
    else if (in_lds)
        approx_scan_kernel<true><<<(unsigned)P, kScanThreads, lds, s>>>((const uint32_t *)codes, (const int2 *)d_table, n_docs,
                                                                        G, tscratch, C, QTq, nq, Lq, n_cand, (Hit *)scratch);
    else
        approx_scan_kernel<false><<<(unsigned)P, kScanThreads, lds, s>>>((const uint32_t *)codes, (const int2 *)d_table,
                                                                         n_docs, G, tscratch, C, QTq, nq, Lq, n_cand,
                                                                         (Hit *)scratch);
    if (hipGetLastError() != hipSuccess) return -3;
    if (form) *form = in_lds ? 1 : 2;
    // the n_cand best of the P lists per query: one level up to kMergeSeg lists, else two
    // (the first level's lists lie behind the grid's, the layout of maxsim_search_scratch_bytes)
    Hit *part = (Hit *)scratch, *part2 = part + (size_t)4 * scan_max_lists() * 128;
    const int S = (P + kMergeSeg - 1) / kMergeSeg;
    if (S > 1) {
        merge_select_kernel<<<dim3((unsigned)nq, (unsigned)S), 64, 0, s>>>(part, P, n_cand, kMergeSeg, part2, nullptr, nullptr);
        if (hipGetLastError() != hipSuccess) return -3;
        merge_select_kernel<<<dim3((unsigned)nq, 1), 64, 0, s>>>(part2, S, n_cand, S, nullptr, d_approx, d_ids);
    } else {
        merge_select_kernel<<<dim3((unsigned)nq, 1), 64, 0, s>>>(part, P, n_cand, P, nullptr, d_approx, d_ids);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_maxsim_rerank_select(const float *exact, const int32_t *ids, int nq, int n_cand, int k, float *out_s,
                                int32_t *out_i, hipStream_t s)
{
    if (nq < 1 || n_cand < 1 || n_cand > 128 || k < 1 || k > n_cand) return -1;
    rerank_select_kernel<<<(unsigned)nq, 128, 0, s>>>(exact, ids, n_cand, k, out_s, out_i);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
