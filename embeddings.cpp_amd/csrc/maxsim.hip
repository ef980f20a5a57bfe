// Late interaction (ColBERT's MaxSim) over a device-resident token store
// (bertx_mvindex_*, bert_hip.h; mvindex.cpp).
//
// Store: documents of len >= 1 token vectors of width w in the f16 fragment order of
// the embedding index (search.hip): 16-row groups, a group's w / 32 blocks of 1 KiB
// consecutive, lane 16g + f of a block = row f, elements 8g .. 8g + 7.  Every document
// starts on a group boundary and takes ceil(len / 16) groups; a table of
// (first group, len) per document says where.  The slots of a document's last group
// past len are never written and may hold anything.
//
// pack_row_f16 is the one normaliser of stored rows and of queries:
//   ss = sum x_i^2 in f32 (order below, a function of w alone); ss == 0: zeros; else
//   rinv = 1 / sqrt(ss) (two correctly rounded f32 operations), v_i = f16(x_i * rinv).
//
// score(doc) = sum_{i < Lq} max_{j < len} sim(q_i, c_j): sim is the search kernel's
// arithmetic (both operands f16, the w / 32 MFMAs of the row's group in ascending k,
// an f32 accumulator from 0), the max is exact, the sum over i is f32 in an order
// fixed by Lq alone.  One wave scores one whole document, so a score depends on the
// query and the document's own rows only, bit for bit.
#include "maxsim_common.h"

namespace emb {
namespace {

constexpr int kThreads = 256;      // 4 waves, each scores whole documents on its own
constexpr int kRingUnits = 4;      // prefetch ring per wave: 4 units of 2 blocks = 8 KiB in flight

// Source rows t0 .. t0 + count - 1 of one add call (rows = row t0) into their slots; one
// wave per row.  src_off says which of the call's n_new documents a row belongs to
// (maxsim_common.h source_doc), table[that document] = (first group, len) where it goes:
// slot 16 first + (t - src_off).
__global__ __launch_bounds__(kThreads) void mv_pack_kernel(const float *__restrict__ rows, int64_t t0, int64_t count,
                                                           int w, const int32_t *__restrict__ src_off,
                                                           const int2 *__restrict__ table, int n_new,
                                                           h16x8 *__restrict__ store)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= count) return;
    const int64_t t = t0 + r;
    const int d = source_doc(src_off, n_new, t);
    const int2 e = table[d];
    const int64_t j = t - src_off[d];
    if (j >= e.y) return;   // (never: the host sizes count by the lens)
    h16x8 v[2];
    pack_row_f16(rows + (size_t)r * w, w, lane, v);
    const int64_t slot = (int64_t)e.x * 16 + j;
    const int chunks = w >> 3, KB = w >> 5;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = lane + 64 * k;
        if (c < chunks) store[frag_index(slot, c, KB)] = v[k];
    }
}

__host__ __device__ inline size_t maxsim_lds_bytes(int QT, int w) { return (size_t)QT * 16 * w * 2; }

// Persistent workgroups.  Prologue: the Lq query rows normalised into B fragments in LDS
// (maxsim_common.h pack_queries, one query of QT tiles).  Then wave v of the
// grid takes candidates v, v + waves, ...: no barrier and no cross-wave step follows
// the prologue.  Per candidate: the document's ceil(len / 16) w / 32 blocks stream
// through a register ring of kRingUnits units of 2 blocks (loads past the document's
// last block re-read that block); after a group's last block accumulator register r
// of lane 16g + c is (row 4g + r of the group, query c): rows >= len become -inf and
// the four fold into the lane's running maxima, which start at -inf.  After the
// document the epilogue (maxsim_common.h doc_score) sums the maxima; lane 0 stores.
// An id outside [0, n_docs) gets -inf and touches nothing else.
// Tomb: nothing, the unmasked kernel; or the store's tombstones (const uint32_t *), the masked
// kernel: a deleted document is treated exactly as an id outside [0, n_docs); its bit is read
// for ids in range only.
template <int QT, class... Tomb>
__global__ __launch_bounds__(kThreads) void maxsim_kernel(const h16x8 *__restrict__ store,
                                                          const int2 *__restrict__ table, int n_docs,
                                                          const float *__restrict__ q, int Lq, int w,
                                                          const int32_t *__restrict__ ids, int n,
                                                          float *__restrict__ out, Tomb... tomb)
{
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int KB = w >> 5, chunks = w >> 3;
    h16x8 *qf = (h16x8 *)smem;                                    // [QT][KB][64]

    // pack_queries<SEARCH_F16>(q, Tiles<1>, Tiles<QT>, ...) written out: called as a function
    // it costs maxsim_kernel<1> two registers in the ring loop
    for (int i = wv; i < QT * 16; i += 4) {
        h16x8 v[2] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
        if (i < Lq) pack_row_f16(q + (size_t)i * w, w, lane, v);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = lane + 64 * k;
            if (c < chunks) qf[frag_index(i, c, KB)] = v[k];
        }
    }
    lds_barrier();

    const int ws = __builtin_amdgcn_readfirstlane(wv);
    const int stride = (int)gridDim.x * 4;
    constexpr int NU = kRingUnits;
    const int g4 = lane >> 4;
    for (int c = (int)blockIdx.x * 4 + ws; c < n; c += stride) {
        const int id = __builtin_amdgcn_readfirstlane(ids ? ids[c] : c);
        bool gone = (unsigned)id >= (unsigned)n_docs;
        if constexpr (sizeof...(Tomb) != 0) {
            if (!gone) gone = doc_deleted(first_tomb(tomb...), id);
        }
        if (gone) {
            if (lane == 0) out[c] = -INFINITY;
            continue;
        }
        const int2 e = table[id];
        const int first = __builtin_amdgcn_readfirstlane(e.x), len = __builtin_amdgcn_readfirstlane(e.y);
        const int U = ((len + 15) >> 4) * (KB >> 1);              // units of 2 blocks; KB is even
        const int last_blk = 2 * U - 1;
        const h16x8 *base = store + (size_t)first * KB * 64;
        auto load = [&](int blk) { return (base + (size_t)min(blk, last_blk) * 64)[lane]; };

        // the ring is filled and refilled in the order it is consumed (search.hip)
        h16x8 ring[NU][2];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            ring[j][0] = load(2 * j);
            ring[j][1] = load(2 * j + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 acc[QT];
        float mx[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            mx[t] = -INFINITY;
        }
        int kb = 0, row0 = 4 * g4;                                // row0: this lane's first row of the group, in the document
        for (int u0 = 0; u0 < U; u0 += NU) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const int u = u0 + j;
                if (u >= U) goto done;   // wave-uniform; no path re-enters the ring out of order
                {
                    const h16x8 a0 = ring[j][0], a1 = ring[j][1];
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        const h16x8 b0 = qf[((size_t)t * KB + kb) * 64 + lane];
                        const h16x8 b1 = qf[((size_t)t * KB + kb + 1) * 64 + lane];
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, acc[t], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    ring[j][0] = load(2 * (u + NU));
                    ring[j][1] = load(2 * (u + NU) + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    kb += 2;
                    if (kb == KB) {
#pragma unroll
                        for (int t = 0; t < QT; ++t) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) mx[t] = fmaxf(mx[t], row0 + r < len ? acc[t][r] : -INFINITY);
                            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                        kb = 0;
                        row0 += 16;
                    }
                }
            }
        }
    done:
        const float s = doc_score<QT>(mx, Lq, lane);
        if (lane == 0) out[c] = s;
    }
}

}  // namespace

int maxsim_prepare_device()
{
    hipError_t e = hipSuccess;
    for (int qt = 1; qt <= 4 && e == hipSuccess; ++qt)
        with_tiles(qt, [&](auto QT) {
            e = allow_lds((const void *)maxsim_kernel<decltype(QT)::value>);
            if (e == hipSuccess) e = allow_lds((const void *)maxsim_kernel<decltype(QT)::value, const uint32_t *>);
        });
    return e == hipSuccess ? maxsim_i8_prepare_device() : -1;
}

int launch_mv_pack(const float *d_rows, int64_t t0, int64_t count, int w, const int32_t *d_src_off,
                   const void *d_table, int n_new, void *store, hipStream_t s)
{
    if (count <= 0 || n_new < 1 || w % 64 || w < 64 || w > 1024) return -1;
    const int64_t blocks = (count + 3) / 4;
    if (blocks > 0x7fffffff) return -1;
    mv_pack_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(d_rows, t0, count, w, d_src_off, (const int2 *)d_table, n_new,
                                                         (h16x8 *)store);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_maxsim(const void *store, const void *d_table, int n_docs, int w, const float *d_q, int Lq,
                  const int32_t *d_ids, int n, float *d_out, hipStream_t s, int max_wg, int *ran_wg, const uint32_t *tomb)
{
    // (the candidate index advances by at most 4 * 4 * CUs per step, in int32)
    if (Lq < 1 || Lq > 64 || n < 1 || n > 0x7fff0000 || n_docs < 0 || w % 64 || w < 64 || w > 1024) return -1;
    const int QT = (Lq + 15) / 16;
    const size_t lds = maxsim_lds_bytes(QT, w);
    if (lds > (size_t)kLdsBudget) return -1;
    const unsigned P = (unsigned)scorer_grid(lds, n, max_wg, ran_wg);
    with_tiles(QT, [&](auto qt) {
        if (tomb)
            maxsim_kernel<decltype(qt)::value, const uint32_t *><<<P, kThreads, lds, s>>>(
                (const h16x8 *)store, (const int2 *)d_table, n_docs, d_q, Lq, w, d_ids, n, d_out, tomb);
        else
            maxsim_kernel<decltype(qt)::value><<<P, kThreads, lds, s>>>((const h16x8 *)store, (const int2 *)d_table, n_docs, d_q,
                                                                        Lq, w, d_ids, n, d_out);
    });
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
