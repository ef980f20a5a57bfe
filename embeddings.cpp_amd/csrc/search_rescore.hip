// Scores of listed rows of the embedding index (bertx_index_score_ids, bert_hip.h;
// DESIGN.md 9e-3): scores[b][j] = the score of (query b, row ids[b][j]) with exactly the
// bits the fused search (search.hip, search_bin.hip) gives that pair.
//
// One wave per (query, 16 listed rows).  f16 and int8 gather the 16 rows into one A
// fragment of the search's MFMA: lane 16g + f loads chunk g of block kb from the slot of
// row ids[f] in that row's own group, where the search's lane 16g + f finds row f of the
// group it streams.  The B fragment holds the query in all 16 columns, made as the
// search's prologue makes it (f16: the cast; int8: quantize_row_i8).  The d / 32 (d / 64)
// MFMAs run in ascending k from a zero accumulator, as the search's do, and an output
// element of an MFMA depends on its own row of A and its own column of B only, so
// register r of lane l holds the search's bits for row 4 (l >> 4) + r.  The matrix core
// runs at 1/16 use; with at most 128 rows per query that is not the cost that matters.
// Binary: lane f < 16 holds row ids[f]'s chunks and takes the popcount expression of
// bin_bits.h against the query's wave-uniform bits.
#include "bin_bits.h"
#include "kernels.h"
#include "quant_i8.h"

#include <algorithm>

namespace emb {
namespace {

// scores [B][n]: -inf for an id outside [0, n_rows).  ids_out (may be null) [B][n]: the id,
// or -1 where the score is -inf.  The rows of such ids are not read (row 0's slot of the
// allocation is, and its result dropped).
// Tomb: nothing, the unmasked kernel; or the index's tombstones (const uint32_t *, index_mask.hip),
// the masked kernel: a deleted row is treated exactly as an id outside [0, n_rows).
template <int ST, class... Tomb>
__global__ __launch_bounds__(64) void score_ids_kernel(const void *__restrict__ corpus,
                                                       const float *__restrict__ row_scale,
                                                       const float *__restrict__ queries, int d, int n_rows,
                                                       const int32_t *__restrict__ ids, int n,
                                                       float *__restrict__ scores, int32_t *__restrict__ ids_out,
                                                       Tomb... tomb)
{
    const int lane = threadIdx.x, f = lane & 15, g = lane >> 4;
    const size_t b = blockIdx.y;
    const int j = blockIdx.x * 16 + f;
    const float *x = queries + b * d;
    const int32_t id = j < n ? ids[b * n + j] : -1;
    bool ok = (uint32_t)id < (uint32_t)n_rows;
    if constexpr (sizeof...(Tomb) != 0) {
        if (ok) ok = !((first_tomb(tomb...)[id >> 5] >> (id & 31)) & 1u);
    }
    const int64_t row = ok ? id : 0;
    float v;
    bool writer;
    if constexpr (ST == SEARCH_F16) {
        const int KB = d >> 5;
        const h16x8 *a_ptr = (const h16x8 *)corpus + (size_t)(row >> 4) * KB * 64 + 16 * g + (row & 15);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < KB; ++kb) {
            const h16x8 a = a_ptr[(size_t)kb * 64];
            const float4 p = *(const float4 *)(x + 32 * kb + 8 * g);
            const float4 q = *(const float4 *)(x + 32 * kb + 8 * g + 4);
            const h16x8 bq = {(h16)p.x, (h16)p.y, (h16)p.z, (h16)p.w, (h16)q.x, (h16)q.y, (h16)q.z, (h16)q.w};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bq, acc, 0, 0, 0);
        }
        // row f of the fragment is register f & 3 of the lanes 16 (f >> 2) + any column
        v = (f & 3) == 0 ? acc[0] : (f & 3) == 1 ? acc[1] : (f & 3) == 2 ? acc[2] : acc[3];
        writer = (f >> 2) == g;
    } else if constexpr (ST == SEARCH_I8) {
        __shared__ i32x4 qv[64];   // chunk c of the quantized query: elements 16c .. 16c + 15
        float qs;
        qv[lane] = quantize_row_i8(x, d, lane, qs);
        lds_barrier();
        const int KB = d >> 6;
        const i32x4 *a_ptr = (const i32x4 *)corpus + (size_t)(row >> 4) * KB * 64 + 16 * g + (row & 15);
        i32x4 acc = {0, 0, 0, 0};
        for (int kb = 0; kb < KB; ++kb)
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_ptr[(size_t)kb * 64], qv[4 * kb + g], acc, 0, 0, 0);
        const int isum = (f & 3) == 0 ? acc[0] : (f & 3) == 1 ? acc[1] : (f & 3) == 2 ? acc[2] : acc[3];
        v = score_i8(isum, qs, ok ? row_scale[row] : 0.f);
        writer = (f >> 2) == g;
    } else {
        const int NB = (d + 127) >> 7;
        int ham = 0;
        for (int c = 0; c < NB; ++c)
            ham = bin_distance(((const uint4 *)corpus)[bin_slot(row, NB, c)], bin_chunk(x, d, c, lane), ham);
        v = bin_score(d, ham);
        writer = g == 0;
    }
    if (writer && j < n) {
        scores[b * n + j] = ok ? v : -INFINITY;
        if (ids_out) ids_out[b * n + j] = ok ? id : -1;
    }
}

template <int ST, class... Tomb>
void launch_score_ids(dim3 grid, const void *corpus, const float *scales, const float *Q, int d, int n_rows,
                      const int32_t *I, int n, float *S, int32_t *O, hipStream_t s, Tomb... tomb)
{
    score_ids_kernel<ST, Tomb...><<<grid, 64, 0, s>>>(corpus, scales, Q, d, n_rows, I, n, S, O, tomb...);
}

template <class... Tomb>
void launch_score_ids_of(int storage, dim3 grid, const void *corpus, const float *scales, const float *Q, int d, int n_rows,
                         const int32_t *I, int n, float *S, int32_t *O, hipStream_t s, Tomb... tomb)
{
    if (storage == SEARCH_F16)
        launch_score_ids<SEARCH_F16>(grid, corpus, nullptr, Q, d, n_rows, I, n, S, O, s, tomb...);
    else if (storage == SEARCH_I8)
        launch_score_ids<SEARCH_I8>(grid, corpus, scales, Q, d, n_rows, I, n, S, O, s, tomb...);
    else
        launch_score_ids<SEARCH_BIN>(grid, corpus, nullptr, Q, d, n_rows, I, n, S, O, s, tomb...);
}

}  // namespace

int launch_index_score_ids(const void *corpus, const float *scales, int storage, int64_t n_rows, int d,
                           const float *d_queries, int B, const int32_t *d_ids, int n, float *d_scores,
                           int32_t *d_ids_out, hipStream_t s, const uint32_t *tomb)
{
    if (B < 1 || n < 1 || n > 128 || d % 64 || d < 64 || d > 1024 || n_rows < 0 || n_rows > 0x7ffffff0 || !corpus) return -1;
    if ((storage != SEARCH_F16 && storage != SEARCH_I8 && storage != SEARCH_BIN) || (storage == SEARCH_I8 && !scales))
        return -1;
    constexpr int kMaxY = 32768;   // queries of one launch (the grid's y)
    for (int b0 = 0; b0 < B; b0 += kMaxY) {
        const dim3 grid((unsigned)((n + 15) / 16), (unsigned)std::min(kMaxY, B - b0));
        const float *Q = d_queries + (size_t)b0 * d;
        const int32_t *I = d_ids + (size_t)b0 * n;
        float *S = d_scores + (size_t)b0 * n;
        int32_t *O = d_ids_out ? d_ids_out + (size_t)b0 * n : nullptr;
        if (tomb)
            launch_score_ids_of(storage, grid, corpus, scales, Q, d, (int)n_rows, I, n, S, O, s, tomb);
        else
            launch_score_ids_of(storage, grid, corpus, scales, Q, d, (int)n_rows, I, n, S, O, s);
        if (hipGetLastError() != hipSuccess) return -3;
    }
    return 0;
}

}  // namespace emb
