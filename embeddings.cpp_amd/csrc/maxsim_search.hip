// Full-scan MaxSim top-k over the token store (bertx_mvindex_search*, bert_hip.h;
// mvindex.cpp): the score arithmetic of maxsim.hip / maxsim_i8.hip joined
// to the list machinery of search.hip.  One streaming pass over every stored group scores
// up to four 16-row tiles of query rows, which is 4, 2, 1 or 1 whole queries of 1, 2, 3
// or 4 tiles each, and keeps each query's k best (score, id) in LDS; a selection kernel
// then takes the k best of the workgroups' lists by sorting them in LDS.
//
// score(query, doc) is, bit for bit, what the scorers return: the same pack_row_f16 /
// pack_row_i8 of the query rows (maxsim_common.h pack_queries), per 16-row group the same
// MFMAs in ascending k from a zero accumulator, rows >= len selected to -inf, the exact
// max, and the scorers' own epilogue (maxsim_common.h doc_score).  One wave scores one
// whole document, so a score depends on that query and that document's rows only: not on the other queries of the call, B, k, the
// document count or where the document sits.
#include "maxsim_common.h"
#include "topk_list.h"

namespace emb {
namespace {

constexpr int kThreads = 256;      // 4 waves, each streams its own contiguous run of documents
constexpr int kSelSeg = 32;        // lists one workgroup of the selection takes: 32 * 128 = 4,096 pairs in LDS
constexpr int kSelMax = kSelSeg * 128;
static_assert(kScanMaxWg == kSelSeg * kSelSeg, "two selection levels cover the grid's lists");

// A storage kind (maxsim_common.h Kind) with its ring: the blocks of a ring unit and the
// units of the ring (8 KiB in flight per wave either way, the scorers' depth).
template <int ST> struct Store;
template <> struct Store<SEARCH_F16> : Kind<SEARCH_F16> {
    static constexpr int kUnit = 2, kRingUnits = 4;
};
template <> struct Store<SEARCH_I8> : Kind<SEARCH_I8> {
    static constexpr int kUnit = 1, kRingUnits = 8;
};

// LDS: the TT tiles of query fragments, the 64 query u (int8; kept for both kinds), one
// list of k per wave and query.
template <int ST>
__host__ __device__ inline size_t msearch_lds_bytes(int TT, int NQ, int w, int k)
{
    return (size_t)TT * 16 * Store<ST>::row_bytes(w) + 64 * 4 + (size_t)4 * NQ * k * sizeof(Hit);
}

// NQ queries of QTq tiles each, q f32 [NQ][Lq][w]; G = the store's used groups.
// Prologue: the scorers' (maxsim_common.h pack_queries), tile t = QTq * (query of the
// pass) + (tile of the query).
// Ranges: wave v of the grid's W takes the documents whose first group lies in
// [v G / W, (v + 1) G / W): two binary searches (first_doc_at over the table in the
// constant address space, TablePtr), uniform over the wave.  Documents are
// contiguous in the store, so that is one contiguous run of groups, streamed through one
// register ring that is refilled across document boundaries (loads past the run's last
// block re-read that block).  int8: the rows' u ride in the ring as in maxsim_i8_kernel.
// After a group's last block its rows fold into the lane's running maxima; the
// wave-uniform test rbase + 16 >= len closes the document: the scorers' epilogue per
// query, the score parked in lane `npend` of a pending register, the next document's len
// fetched one document ahead.  The pending scores are offered to the wave's own lists
// once per pass over the ring when the next pass could overflow the 64 lanes, and at the
// end; nothing in the stream crosses waves.  Then one barrier, wave q folds the four
// waves' lists of query q and writes partial [query][P][k].
// Mask: nothing, the unmasked kernel, whose arguments end at partial; or one SearchMask over
// documents (filt at the pass's first filter), the masked kernel.  The mask
// acts where a document closes.  Its admissible words (maxsim_common.h admit_words, one per
// query of the pass, wave-uniform, through the scalar cache) are held for the open document
// and for the one behind it; the word of the next 32 documents is asked for when the document
// before them opens, a whole document ahead of its first use, as len_next is.  A document that
// no query of the pass admits takes no pending lane; one that some admit takes a lane, and the
// queries' bits are parked beside its scores (`pok`) and become each query's offer predicate.
// The scores themselves are computed as ever.
template <int QTq, int NQ, int ST, class... Mask>
__global__ __launch_bounds__(kThreads) void maxsim_search_kernel(const typename Store<ST>::Block *__restrict__ store,
                                                                 const float *__restrict__ scales,
                                                                 const int2 *__restrict__ table, int n_docs, int G,
                                                                 const float *__restrict__ q, int Lq, int w, int k,
                                                                 Hit *__restrict__ partial, Mask... mask)
{
    constexpr bool MK = sizeof...(Mask) != 0;
    SearchMask m{nullptr, nullptr, 0};
    if constexpr (MK) m = first_mask(mask...);
    typedef Store<ST> S;
    typedef typename S::Block Block;
    typedef typename S::Acc Acc;
    constexpr int TT = QTq * NQ, UB = S::kUnit, NU = S::kRingUnits;
    static_assert(TT <= 4, "a pass holds four tiles");
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int KB = w >> S::kShift;
    Block *qf = (Block *)smem;                                    // [TT][KB][64]
    float *qu = (float *)(qf + (size_t)TT * KB * 64);             // [64]
    Hit *lists = (Hit *)(qu + 64);                                // [4][NQ][k]

    // pack_queries<ST>(q, Tiles<NQ>, Tiles<QTq>, ...) written out: called as a function it
    // changes the f16 kernels' registers and occupancy
    for (int i = wv; i < TT * 16; i += 4) {
        const int t = i >> 4, qi = t / QTq, rq = ((t - qi * QTq) << 4) + (i & 15);
        const float *src = q + ((size_t)qi * Lq + min(rq, Lq - 1)) * w;
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
    for (int i = tid; i < 4 * NQ * k; i += kThreads) lists[i] = Hit{-INFINITY, -1};
    lds_barrier();

    const int ws = __builtin_amdgcn_readfirstlane(wv);
    Hit *mine = lists + (size_t)ws * NQ * k;                      // this wave's NQ lists
    const TablePtr tab = (TablePtr)(uintptr_t)table;
    const int64_t W = (int64_t)gridDim.x * 4, v = (int64_t)blockIdx.x * 4 + ws;
    const int dA = first_doc_at(tab, n_docs, (int)(v * G / W));
    const int dB = first_doc_at(tab, n_docs, (int)((v + 1) * G / W));

    if (dA < dB) {   // wave-uniform
        const int gA = tab[dA].x, gB = dB < n_docs ? tab[dB].x : G;
        const int Gw = gB - gA;                                   // this wave's groups
        const int U = Gw * (KB / UB);                             // units; KB is even for f16
        const int last_blk = Gw * KB - 1;
        const Block *base = store + (size_t)gA * KB * 64;
        const int g4 = lane >> 4;
        const int urow = 4 * g4 + (lane & 3);                     // int8: the row of a group whose u this lane loads
        const float *ubase = scales + (size_t)gA * 16 + urow;
        float uq[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) uq[t] = ST == SEARCH_I8 ? qu[16 * t + (lane & 15)] : 0.f;

        // the load pointer: block lb of the run, which is block lkb of its group lg
        int lb = 0, lkb = 0, lg = 0;
        auto load = [&](Block (&blk)[UB], float &u) {
            blk[0] = (base + (size_t)min(lb, last_blk) * 64)[lane];
            if constexpr (UB == 2) blk[1] = (base + (size_t)min(lb + 1, last_blk) * 64)[lane];
            if constexpr (ST == SEARCH_I8) u = ubase[(size_t)min(lg, Gw - 1) * 16];
            lb += UB;
            lkb += UB;
            if (lkb == KB) {
                lkb = 0;
                ++lg;
            }
        };

        // the ring is filled and refilled in the order it is consumed (search.hip)
        Block ring[NU][UB];
        float ring_u[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            ring_u[j] = 0.f;
            load(ring[j], ring_u[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
        Acc acc[TT];
        float mx[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            acc[t] = Acc{0, 0, 0, 0};
            mx[t] = -INFINITY;
        }
        // the open document: its id and len, the next one's len, the document row of the
        // open group's row 0; all wave-uniform
        int id = dA, len = tab[dA].y, len_next = tab[min(dA + 1, n_docs - 1)].y, rbase = 0, kb = 0;
        // finished documents not yet offered: lane i < npend holds the i-th one's id and scores
        float ps[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) ps[i] = -INFINITY;
        int pid = -1, npend = 0;
        // masked: the admissible words of the open document and of the one behind it; per lane
        // the parked document's bit per query
        uint32_t aw[NQ] = {}, an[NQ] = {};
        int pok = 0;
        if constexpr (MK) {
            admit_words<NQ>(m, NQ, dA, aw);
            admit_words<NQ>(m, NQ, min(dA + 1, n_docs - 1), an);
        }
        auto flush = [&]() {
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                bool on = lane < npend;
                if constexpr (MK) on = on && ((pok >> i) & 1);
                list_offer(mine + (size_t)i * k, k, ps[i], pid, on, lane);
            }
            npend = 0;
        };

        // one unit out of ring slot j; refill: ask for the blocks NU units on into the same slot
        auto unit = [&](int j, bool refill) {
            const Block a0 = ring[j][0], a1 = ring[j][UB - 1];
            // int8: the u of rows 4g .. 4g + 3, lanes 0 .. 3 of this lane's quad; taken in every
            // unit and before the refill (maxsim_i8_kernel)
            float rrow[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (ST == SEARCH_I8) quad_u(ring_u[j], rrow);
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const Block b0 = qf[((size_t)t * KB + kb) * 64 + lane];
                acc[t] = mma(a0, b0, acc[t]);
                if constexpr (UB == 2) {
                    const Block b1 = qf[((size_t)t * KB + kb + 1) * 64 + lane];
                    acc[t] = mma(a1, b1, acc[t]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (refill) load(ring[j], ring_u[j]);
            __builtin_amdgcn_sched_barrier(0);
            kb += UB;
            if (kb == KB) {
                // accumulator register r of lane 16g + c: (row 4g + r of the group, query row c of tile t)
                const int row0 = rbase + 4 * g4;
#pragma unroll
                for (int t = 0; t < TT; ++t) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float s = sim(acc[t][r], uq[t], rrow[r]);
                        mx[t] = fmaxf(mx[t], row0 + r < len ? s : -INFINITY);
                    }
                    acc[t] = Acc{0, 0, 0, 0};
                }
                kb = 0;
                if (rbase + 16 >= len) {   // wave-uniform: the document's last group
                    int ok = 1;            // masked: bit i set when query i of the pass admits the document
                    if constexpr (MK) ok = admit_bits<NQ>(aw, NQ, id);
#pragma unroll
                    for (int i = 0; i < NQ; ++i) {
                        // doc_score<QTq> of the query's maxima (maxsim_common.h) written out, the
                        // maxima reset on the way: called as a function it costs this kernel
                        // its ring waits
                        float s = 0.f;
#pragma unroll
                        for (int t = 0; t < QTq; ++t) {
                            float m = mx[i * QTq + t];
                            m = fmaxf(m, __shfl_xor(m, 16, 64));
                            m = fmaxf(m, __shfl_xor(m, 32, 64));
                            s = __fadd_rn(s, 16 * t + (lane & 15) < Lq ? m : 0.f);
                            mx[i * QTq + t] = -INFINITY;
                        }
#pragma unroll
                        for (int o = 8; o >= 1; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
                        // lane 0's sum is the score
                        const float s0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s)));
                        ps[i] = lane == npend ? s0 : ps[i];
                    }
                    pid = lane == npend ? id : pid;
                    if constexpr (MK) {
                        pok = lane == npend ? ok : pok;
                        npend += ok != 0;   // no query admits it: the lane is taken again
                    } else {
                        ++npend;
                    }
                    ++id;
                    len = len_next;
                    len_next = tab[min(id + 1, n_docs - 1)].y;
                    if constexpr (MK) {
#pragma unroll
                        for (int i = 0; i < NQ; ++i) aw[i] = an[i];
                        // wave-uniform: the document behind the one that opens starts a word
                        if (((id + 1) & 31) == 0 && id + 1 < n_docs) admit_words<NQ>(m, NQ, id + 1, an);
                    }
                    rbase = 0;
                } else {
                    rbase += 16;
                }
            }
        };
        // Whole passes over the ring with no exit inside, then the last U % NU units, which
        // ask for nothing more (maxsim_i8_kernel).  A pass closes at most NU documents.
        int u0 = 0;
        for (; u0 + NU <= U; u0 += NU) {
#pragma unroll
            for (int j = 0; j < NU; ++j) unit(j, true);
            if (npend > 64 - NU) flush();
        }
#pragma unroll
        for (int j = 0; j < NU - 1; ++j) {
            if (u0 + j >= U) break;   // wave-uniform
            unit(j, false);
        }
        flush();
    }
    lds_barrier();

    // wave i folds the other waves' lists of query i into its own and writes it out
    if (ws < NQ) {
        Hit *dst = lists + ((size_t)ws * NQ + ws) * k;
        for (int o = 0; o < 4; ++o) {
            if (o == ws) continue;
            const Hit *src = lists + ((size_t)o * NQ + ws) * k;
            Hit e0{-INFINITY, -1}, e1{-INFINITY, -1};
            if (lane < k) e0 = src[lane];
            if (lane + 64 < k) e1 = src[lane + 64];
            list_offer(dst, k, e0.s, e0.id, lane < k && e0.id >= 0, lane);
            list_offer(dst, k, e1.s, e1.id, lane + 64 < k && e1.id >= 0, lane);
        }
        Hit *out = partial + ((size_t)ws * gridDim.x + blockIdx.x) * k;
        for (int j = lane; j < k; j += 64) out[j] = dst[j];
    }
}

// The k best of a query's lists.  search.hip's merge kernel folds lists one insertion
// after the other, which is right for its few hundred lists of which most entries lose
// against the running k-th; here a query has up to a thousand lists whose entries are all
// contenders (a wave sees a few dozen documents), and the chain of insertions took 260 us
// at k = 128.  Instead workgroup (q, y) loads the lists y seg .. y seg + seg - 1 of query q
// (at most kSelMax pairs, the rest of the power of two N filled with (-inf, -1)), sorts
// them by `better` with a bitonic network in LDS and writes the first k: to hits
// [q][gridDim.y][k] when hits is given (the first level), else to scores / ids [q][k].
// `better` is a total order with the fill last, so the result is that of the lists.
__global__ __launch_bounds__(kThreads) void select_kernel(const Hit *__restrict__ partial, int all_P, int k, int seg,
                                                          int N, Hit *__restrict__ hits, float *__restrict__ scores,
                                                          int32_t *__restrict__ ids)
{
    __shared__ Hit s[kSelMax];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int p0 = (int)blockIdx.y * seg, P = min(all_P - p0, seg), n = P * k;
    const Hit *src = partial + ((size_t)q * all_P + p0) * k;
    for (int i = tid; i < N; i += kThreads) s[i] = i < n ? src[i] : Hit{-INFINITY, -1};
    __syncthreads();
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (N >> 1); i += kThreads) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo + stride;
                const Hit a = s[lo], b = s[hi];
                // descending blocks where bit `size` of the index is clear (the whole array at the last size)
                const bool swap = (lo & size) == 0 ? better(b.s, b.id, a.s, a.id) : better(a.s, a.id, b.s, b.id);
                if (swap) {
                    s[lo] = b;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += kThreads) {
        const Hit e = s[j];   // (k <= N: n >= k unless the fill completes the list)
        if (hits) {
            hits[((size_t)q * gridDim.y + blockIdx.y) * k + j] = e;
        } else {
            scores[(size_t)q * k + j] = e.s;
            ids[(size_t)q * k + j] = e.id;
        }
    }
}

int pow2_at_least(int n)
{
    int N = 2;
    while (N < n) N <<= 1;
    return N;
}

// f(QTq, NQ as integral constants) for the pass of nq queries of qtq tiles; false when the
// pass does not fit four tiles (no kernel is instantiated for it).
template <class F>
bool with_pass(int qtq, int nq, F &&f)
{
    bool fits = false;
    with_tiles(qtq, [&](auto a) {
        with_tiles(nq, [&](auto b) {
            if constexpr (decltype(a)::value * decltype(b)::value <= 4) {
                if (decltype(a)::value == qtq && decltype(b)::value == nq) {
                    f(a, b);
                    fits = true;
                }
            }
        });
    });
    return fits;
}

template <int ST, class... Mask>
hipError_t allow_lds_all()
{
    hipError_t e = hipSuccess;
    for (int qtq = 1; qtq <= 4; ++qtq)
        for (int nq = 1; nq <= 4 / qtq && e == hipSuccess; ++nq)
            with_pass(qtq, nq, [&](auto a, auto b) {
                e = allow_lds((const void *)maxsim_search_kernel<decltype(a)::value, decltype(b)::value, ST, Mask...>);
            });
    return e;
}

// mask: none (the unmasked kernels) or the call's SearchMask
template <int ST, class... Mask>
int launch_all(const void *store, const float *scales, const void *table, int n_docs, int G, int w, const float *d_q,
               int B, int Lq, int k, void *scratch, float *d_scores, int32_t *d_ids, hipStream_t s, int max_wg, int *ran_wg,
               Mask... mask)
{
    const int QTq = (Lq + 15) / 16, per_pass = 4 / QTq;
    for (int b0 = 0; b0 < B; b0 += per_pass) {
        const int nq = std::min(per_pass, B - b0);
        const size_t lds = msearch_lds_bytes<ST>(QTq * nq, nq, w, k);
        if (lds > (size_t)kLdsBudget) return -1;
        const int P = scan_grid(lds, G, 4, max_wg, ran_wg);
        const float *Q = d_q + (size_t)b0 * Lq * w;
        Hit *part = (Hit *)scratch;
        const bool fits = with_pass(QTq, nq, [&](auto a, auto b) {
            // (the pass's own filters: a shared filter has stride 0)
            maxsim_search_kernel<decltype(a)::value, decltype(b)::value, ST, Mask...><<<(unsigned)P, kThreads, lds, s>>>(
                (const typename Store<ST>::Block *)store, scales, (const int2 *)table, n_docs, G, Q, Lq, w, k, part,
                pass_mask(mask, b0)...);
        });
        if (!fits) return -1;
        if (hipGetLastError() != hipSuccess) return -3;
        // the k best of the P lists per query: one level up to kSelSeg lists, else two
        const int S = (P + kSelSeg - 1) / kSelSeg;
        Hit *part2 = part + (size_t)4 * scan_max_lists() * 128;
        float *sc = d_scores + (size_t)b0 * k;
        int32_t *id = d_ids + (size_t)b0 * k;
        if (S > 1) {
            select_kernel<<<dim3((unsigned)nq, (unsigned)S), kThreads, 0, s>>>(part, P, k, kSelSeg,
                                                                               pow2_at_least(kSelSeg * k), part2, nullptr,
                                                                               nullptr);
            if (hipGetLastError() != hipSuccess) return -3;
            select_kernel<<<dim3((unsigned)nq, 1), kThreads, 0, s>>>(part2, S, k, S, pow2_at_least(S * k), nullptr, sc, id);
        } else {
            select_kernel<<<dim3((unsigned)nq, 1), kThreads, 0, s>>>(part, P, k, P, pow2_at_least(std::max(P * k, k)),
                                                                     nullptr, sc, id);
        }
        if (hipGetLastError() != hipSuccess) return -3;
    }
    return 0;
}

}  // namespace

int maxsim_search_prepare_device()
{
    hipError_t e = allow_lds_all<SEARCH_F16>();
    if (e == hipSuccess) e = allow_lds_all<SEARCH_I8>();
    if (e == hipSuccess) e = allow_lds_all<SEARCH_F16, SearchMask>();
    if (e == hipSuccess) e = allow_lds_all<SEARCH_I8, SearchMask>();
    return e == hipSuccess ? 0 : -1;
}

size_t maxsim_search_scratch_bytes()
{
    // the workgroups' lists, then the first selection level's: 4 queries, k = 128
    const size_t P = (size_t)scan_max_lists();
    return 4 * (P + (P + kSelSeg - 1) / kSelSeg) * 128 * sizeof(Hit);
}

int launch_maxsim_search(const void *store, const float *scales, int storage, const void *d_table, int n_docs,
                         int64_t used_groups, int w, const float *d_q, int B, int Lq, int k, void *scratch,
                         float *d_scores, int32_t *d_ids, hipStream_t s, int max_wg, int *ran_wg, const SearchMask *mask)
{
    if (B < 1 || Lq < 1 || Lq > 64 || k < 1 || k > 128 || n_docs < 0 || used_groups < 0 || used_groups > 0x7ffffff0ll ||
        w % 64 || w < 64 || w > 1024 || !scratch)
        return -1;
    if ((storage != SEARCH_F16 && storage != SEARCH_I8) || (storage == SEARCH_I8 && !scales)) return -1;
    if (mask) {
        if (!mask->tomb) return -1;
        if (storage == SEARCH_I8)
            return launch_all<SEARCH_I8>(store, scales, d_table, n_docs, (int)used_groups, w, d_q, B, Lq, k, scratch,
                                         d_scores, d_ids, s, max_wg, ran_wg, *mask);
        return launch_all<SEARCH_F16>(store, nullptr, d_table, n_docs, (int)used_groups, w, d_q, B, Lq, k, scratch, d_scores,
                                      d_ids, s, max_wg, ran_wg, *mask);
    }
    if (storage == SEARCH_I8)
        return launch_all<SEARCH_I8>(store, scales, d_table, n_docs, (int)used_groups, w, d_q, B, Lq, k, scratch, d_scores,
                                     d_ids, s, max_wg, ran_wg);
    return launch_all<SEARCH_F16>(store, nullptr, d_table, n_docs, (int)used_groups, w, d_q, B, Lq, k, scratch, d_scores,
                                  d_ids, s, max_wg, ran_wg);
}

}  // namespace emb
