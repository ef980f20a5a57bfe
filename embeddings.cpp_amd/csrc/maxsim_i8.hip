// int8 storage of the late-interaction token store (bertx_mvindex_create_ex with
// BERTX_INDEX_I8, bert_hip.h; mvindex.cpp): maxsim.hip's pack kernel and
// scorer over the embedding index's int8 rows.
//
// Store: the layout of maxsim.hip in the i8 fragment order of search.hip: 16-row groups,
// a group's w / 64 blocks of 1 KiB consecutive, lane 16g + f of a block = row f, bytes
// 16g .. 16g + 15; every document starts on a group boundary; one f32 per token slot in
// a second buffer.  Slots past a document's len, and their f32, are never written.
//
// pack_row_i8 is the one normaliser of stored rows and of queries: q = quantize_row_i8
// of the raw row (quant_i8.h; its scale is dropped), n2 = sum q_i^2 in int32 (exact,
// < 2^24), u = 1 / sqrt((float)n2) (two correctly rounded f32 operations), 0 for n2 == 0.
// The row stands for q_i * u, a unit vector.
//
// sim(a, c) = score_i8(isum, u_a, u_c) with the exact int32 isum of v_mfma_i32_16x16x64_i8;
// score(doc) = sum_{i < Lq} max_{j < len} sim(q_i, c_j), the max exact and the sum in the
// order of maxsim_kernel.  No step depends on an order the caller cannot reproduce.
#include "maxsim_common.h"

namespace emb {
namespace {

constexpr int kThreads = 256;      // 4 waves, each scores whole documents on its own
constexpr int kRingUnits = 8;      // prefetch ring per wave: 8 units of 1 block = 8 KiB in flight

// mv_pack_kernel over an int8 store: the same (src_off, table) lookup, one wave per row.
__global__ __launch_bounds__(kThreads) void mv_pack_i8_kernel(const float *__restrict__ rows, int64_t t0, int64_t count,
                                                              int w, const int32_t *__restrict__ src_off,
                                                              const int2 *__restrict__ table, int n_new,
                                                              i32x4 *__restrict__ store, float *__restrict__ scales)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= count) return;
    const int64_t t = t0 + r;
    const int d = source_doc(src_off, n_new, t);
    const int2 e = table[d];
    const int64_t j = t - src_off[d];
    if (j >= e.y) return;   // (never: the host sizes count by the lens)
    float u;
    const i32x4 v = pack_row_i8(rows + (size_t)r * w, w, lane, u);
    const int64_t slot = (int64_t)e.x * 16 + j;
    if (lane < (w >> 4)) store[frag_index(slot, lane, w >> 6)] = v;
    if (lane == 0) scales[slot] = u;
}

__host__ __device__ inline size_t maxsim_i8_lds_bytes(int QT, int w) { return (size_t)QT * 16 * w + 64 * 4; }

// The shape of maxsim_kernel.  Prologue: the Lq query rows packed (pack_row_i8's steps, one
// wave per row, four rows of a wave at a time) into B fragments in LDS, lane 16g + c of
// block (t, kb) = query 16t + c, bytes 64kb + 16g .. + 15, and their u beside them;
// queries Lq .. 16 QT - 1 are zeros with u = 0.  Then wave v of the grid takes candidates
// v, v + waves, ... with no barrier and no cross-wave step.  Per candidate the document's
// ceil(len / 16) w / 64 blocks stream through a register ring of kRingUnits units (loads
// past the document's last block re-read that block), in whole passes over the ring and
// a tail (below).  A unit is one block and one dword per lane of its group's u:
// lane 16g + c asks for the u of row 4g + (c & 3), so the four u a lane needs sit in its
// own quad and come out by four DPP moves (maxsim_common.h quad_u).  The u ride in the ring, not a group ahead
// through the scalar cache as search.hip's do: a wave that scores one document alone
// (1,000 candidates) would wait out one scalar miss per group, and a vector load issued
// out of ring order would drain the ring through the in-order vector-memory counter.
// Every unit loads its dword whether or not it ends a group, so the count of loads in
// flight is the same on every path; a document's groups are whole, so the dword is
// always inside the buffer.  After a group's last block accumulator register r of lane
// 16g + c is (row 4g + r of the group, query c): sim = score_i8(acc, u_query, u_row),
// rows >= len select -inf, and the four fold into the lane's running maxima.  The
// epilogue is the scorers' one (maxsim_common.h doc_score).
// An id outside [0, n_docs) gets -inf and touches nothing else.
// Tomb: nothing, the unmasked kernel; or the store's tombstones (const uint32_t *), the masked
// kernel: a deleted document is treated exactly as an id outside [0, n_docs); its bit is read
// for ids in range only.
template <int QT, class... Tomb>
__global__ __launch_bounds__(kThreads) void maxsim_i8_kernel(const i32x4 *__restrict__ store,
                                                             const float *__restrict__ scales,
                                                             const int2 *__restrict__ table, int n_docs,
                                                             const float *__restrict__ q, int Lq, int w,
                                                             const int32_t *__restrict__ ids, int n,
                                                             float *__restrict__ out, Tomb... tomb)
{
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int KB = w >> 6;
    i32x4 *qf = (i32x4 *)smem;                                    // [QT][KB][64]
    float *qu = (float *)(qf + (size_t)QT * KB * 64);             // [64]

    // pack_row_i8 on four rows at a time, step by step: the four loads are in flight
    // together and the rows' reductions interleave (a row past Lq reads row Lq - 1 and
    // is then replaced by zeros, so that the steps stay free of branches)
    for (int i0 = wv; i0 < QT * 16; i0 += 16) {
        if (i0 >= Lq) {   // wave-uniform: none of the four is a query row
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (lane < (w >> 4)) qf[frag_index(i0 + 4 * p, lane, KB)] = i32x4{0, 0, 0, 0};
                if (lane == 0) qu[i0 + 4 * p] = 0.f;
            }
            continue;
        }
        float x[4][16], amax[4], u[4];
        i32x4 v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) load_row_i8(q + (size_t)min(i0 + 4 * p, Lq - 1) * w, w, lane, x[p]);
#pragma unroll
        for (int p = 0; p < 4; ++p) amax[p] = row_amax_i8(x[p]);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float scale;
            v[p] = quantize_values_i8(x[p], amax[p], scale);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) u[p] = unit_scale_i8(v[p]);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = i0 + 4 * p;
            if (lane < (w >> 4)) qf[frag_index(i, lane, KB)] = i < Lq ? v[p] : i32x4{0, 0, 0, 0};
            if (lane == 0) qu[i] = i < Lq ? u[p] : 0.f;
        }
    }
    lds_barrier();

    const int ws = __builtin_amdgcn_readfirstlane(wv);
    const int stride = (int)gridDim.x * 4;
    constexpr int NU = kRingUnits;
    const int g4 = lane >> 4;
    float uq[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) uq[t] = qu[16 * t + (lane & 15)];
    const int urow = 4 * g4 + (lane & 3);                         // the row of a group whose u this lane loads

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
        const int G = (len + 15) >> 4;
        const int U = G * KB;                                     // units of 1 block
        const int last_blk = U - 1;
        const i32x4 *base = store + (size_t)first * KB * 64;
        const float *ubase = scales + (size_t)first * 16 + urow;
        // the load pointer: block lb of the document, which is block lkb of its group lg
        int lb = 0, lkb = 0, lg = 0;
        auto load = [&](i32x4 &blk, float &u) {
            blk = (base + (size_t)min(lb, last_blk) * 64)[lane];
            u = ubase[(size_t)min(lg, G - 1) * 16];
            ++lb;
            if (++lkb == KB) {
                lkb = 0;
                ++lg;
            }
        };

        // the ring is filled and refilled in the order it is consumed (search.hip)
        i32x4 ring[NU];
        float ring_u[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            load(ring[j], ring_u[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
        i32x4 acc[QT];
        float mx[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            acc[t] = i32x4{0, 0, 0, 0};
            mx[t] = -INFINITY;
        }
        int kb = 0, row0 = 4 * g4;                                // row0: this lane's first row of the group, in the document
        // one unit out of ring slot j; refill: ask for the block NU units on into the same slot
        auto unit = [&](int j, bool refill) {
            const i32x4 a = ring[j];
            // the u of rows 4g .. 4g + 3: lanes 0 .. 3 of this lane's quad.  Taken in every
            // unit and before the refill, so that the slot's old dword is dead when the
            // new one is asked for (else the compiler keeps both and waits for every load
            // in flight to copy one over the other)
            float rrow[4];
            quad_u(ring_u[j], rrow);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const i32x4 b = qf[((size_t)t * KB + kb) * 64 + lane];
                acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[t], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (refill) load(ring[j], ring_u[j]);
            __builtin_amdgcn_sched_barrier(0);
            if (++kb == KB) {
#pragma unroll
                for (int t = 0; t < QT; ++t) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float sim = score_i8(acc[t][r], uq[t], rrow[r]);
                        mx[t] = fmaxf(mx[t], row0 + r < len ? sim : -INFINITY);
                    }
                    acc[t] = i32x4{0, 0, 0, 0};
                }
                kb = 0;
                row0 += 16;
            }
        };
        // Whole passes over the ring with no exit inside, so that the loop's latch has one
        // predecessor and every unit waits for its own slot only (an exit inside the pass
        // merges with the latch and makes the compiler drain every load at the loop head);
        // then the last U % NU units, which ask for nothing more.
        int u0 = 0;
        for (; u0 + NU <= U; u0 += NU) {
#pragma unroll
            for (int j = 0; j < NU; ++j) unit(j, true);
        }
#pragma unroll
        for (int j = 0; j < NU - 1; ++j) {
            if (u0 + j >= U) break;   // wave-uniform
            unit(j, false);
        }
        const float s = doc_score<QT>(mx, Lq, lane);
        if (lane == 0) out[c] = s;
    }
}

}  // namespace

int maxsim_i8_prepare_device()
{
    hipError_t e = hipSuccess;
    for (int qt = 1; qt <= 4 && e == hipSuccess; ++qt)
        with_tiles(qt, [&](auto QT) {
            e = allow_lds((const void *)maxsim_i8_kernel<decltype(QT)::value>);
            if (e == hipSuccess) e = allow_lds((const void *)maxsim_i8_kernel<decltype(QT)::value, const uint32_t *>);
        });
    return e == hipSuccess ? 0 : -1;
}

int launch_mv_pack_i8(const float *d_rows, int64_t t0, int64_t count, int w, const int32_t *d_src_off,
                      const void *d_table, int n_new, void *store, float *scales, hipStream_t s)
{
    if (count <= 0 || n_new < 1 || w % 64 || w < 64 || w > 1024 || !scales) return -1;
    const int64_t blocks = (count + 3) / 4;
    if (blocks > 0x7fffffff) return -1;
    mv_pack_i8_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(d_rows, t0, count, w, d_src_off, (const int2 *)d_table, n_new,
                                                            (i32x4 *)store, scales);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_maxsim_i8(const void *store, const float *scales, const void *d_table, int n_docs, int w, const float *d_q,
                     int Lq, const int32_t *d_ids, int n, float *d_out, hipStream_t s, int max_wg, int *ran_wg,
                     const uint32_t *tomb)
{
    // (the candidate index advances by at most 4 * 4 * CUs per step, in int32)
    if (Lq < 1 || Lq > 64 || n < 1 || n > 0x7fff0000 || n_docs < 0 || w % 64 || w < 64 || w > 1024 || !scales) return -1;
    const int QT = (Lq + 15) / 16;
    const size_t lds = maxsim_i8_lds_bytes(QT, w);
    if (lds > (size_t)kLdsBudget) return -1;
    const unsigned P = (unsigned)scorer_grid(lds, n, max_wg, ran_wg);
    with_tiles(QT, [&](auto qt) {
        if (tomb)
            maxsim_i8_kernel<decltype(qt)::value, const uint32_t *><<<P, kThreads, lds, s>>>(
                (const i32x4 *)store, scales, (const int2 *)d_table, n_docs, d_q, Lq, w, d_ids, n, d_out, tomb);
        else
            maxsim_i8_kernel<decltype(qt)::value><<<P, kThreads, lds, s>>>((const i32x4 *)store, scales, (const int2 *)d_table,
                                                                           n_docs, d_q, Lq, w, d_ids, n, d_out);
    });
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
