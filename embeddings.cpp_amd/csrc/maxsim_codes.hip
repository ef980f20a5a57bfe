// Centroid codes of the token store (bertx_mvindex_set_centroids, bert_hip.h "Centroid
// codes"; mvindex.cpp): one uint16 per token slot, the centroid nearest to
// the slot's stored row.
//
// The code of a row is what the full-scan search returns for it against a store of the
// centroids: the row's stored values widened (f16 -> f32; q * u on int8) go through the
// query packer (pack_row_f16 / pack_row_i8: the normaliser runs again), the centroids stand
// in the stored-row role of the scorers' MFMA sequence, ascending k from a zero
// accumulator, and the centroid of highest sim wins, equal sims going to the lower index.
// A row stored as zeros has sim 0 to every centroid and gets code 0.
#include "maxsim_common.h"

namespace emb {
namespace {

constexpr int kThreads = 256;      // 4 waves, each codes one 16-slot group of the store

// LDS per wave: the 16 rows as query fragments, one widened row, the 16 query u.
template <int ST>
__host__ __device__ inline size_t assign_lds_bytes(int w)
{
    return 4 * (16 * Kind<ST>::row_bytes(w) + (size_t)w * 4 + 64);
}

// Wave v of the grid takes group g0 + v (a wave past g1 works on group g1 - 1 and writes
// nothing, so that every wave reaches the barrier).  Prologue, per row of the group: each
// lane widens the chunks of the stored row that the packer will ask it for into the wave's
// f32 row in LDS (a lane reads back only what it wrote itself), the packer runs on that
// row, and the fragments go to the wave's query tile, lane 16g + c of block kb = row c.
// Then the centroid groups stream through the MFMA in ascending order: accumulator
// register r of lane 16g + c is (centroid 16 cg + 4g + r, row c); a lane keeps the best of
// its centroids with a strict >, ascending, so the lowest index of equal sims stays; two
// shuffles fold the four g by (sim, lower index).  Lanes 0 .. 15 store the codes.  Slots
// past a document's len are coded like any other here (whatever they hold, the index is
// below C) and set to 0 by mv_code_tails_kernel afterwards.
template <int ST>
__global__ __launch_bounds__(kThreads) void mv_assign_kernel(const typename Kind<ST>::Block *__restrict__ store,
                                                             const float *__restrict__ scales, int64_t g0, int64_t g1,
                                                             int w, const typename Kind<ST>::Block *__restrict__ cent,
                                                             const float *__restrict__ cent_u, int C,
                                                             uint16_t *__restrict__ codes)
{
    typedef Kind<ST> S;
    typedef typename S::Block Block;
    typedef typename S::Acc Acc;
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int KB = w >> S::kShift;
    const size_t per_wave = 16 * S::row_bytes(w) + (size_t)w * 4 + 64;
    char *mine = (char *)smem + (size_t)wv * per_wave;
    Block *qf = (Block *)mine;                                    // [KB][64]
    float *xs = (float *)(mine + 16 * S::row_bytes(w));           // [w]
    float *qu = xs + w;                                           // [16]
    const int64_t gv = g0 + (int64_t)blockIdx.x * 4 + wv;
    const bool live = gv < g1;
    const int64_t g = live ? gv : g1 - 1;

    for (int i = 0; i < 16; ++i) {
        const int64_t slot = g * 16 + i;
        if constexpr (ST == SEARCH_F16) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = lane + 64 * j;
                if (c < (w >> 3)) {
                    const h16x8 v = store[frag_index(slot, c, KB)];
#pragma unroll
                    for (int e = 0; e < 8; ++e) xs[8 * c + e] = (float)v[e];
                }
            }
            h16x8 p[2];
            pack_row_f16(xs, w, lane, p);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = lane + 64 * j;
                if (c < (w >> 3)) qf[frag_index(i, c, KB)] = p[j];
            }
        } else {
            const float u = scales[slot];
            if (lane < (w >> 4)) {
                const i32x4 v = store[frag_index(slot, lane, KB)];
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    xs[16 * lane + e] = __fmul_rn((float)(int8_t)((v[e >> 2] >> (8 * (e & 3))) & 0xff), u);
            }
            float pu;
            const i32x4 p = pack_row_i8(xs, w, lane, pu);
            if (lane < (w >> 4)) qf[frag_index(i, lane, KB)] = p;
            if (lane == 0) qu[i] = pu;
        }
    }
    lds_barrier();

    const int g4 = lane >> 4;
    float uq = 0.f;
    if constexpr (ST == SEARCH_I8) uq = qu[lane & 15];
    float best = -INFINITY;
    int bi = 0;
    const int CG = C >> 4;
    for (int cg = 0; cg < CG; ++cg) {
        const Block *a = cent + (size_t)cg * KB * 64 + lane;
        Acc acc = Acc{0, 0, 0, 0};
        for (int kb = 0; kb < KB; ++kb) acc = mma(a[(size_t)kb * 64], qf[(size_t)kb * 64 + lane], acc);
        float4 ur = {0.f, 0.f, 0.f, 0.f};
        if constexpr (ST == SEARCH_I8) ur = *(const float4 *)(cent_u + 16 * cg + 4 * g4);
        const float urow[4] = {ur.x, ur.y, ur.z, ur.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s = sim(acc[r], uq, urow[r]);
            if (s > best) {
                best = s;
                bi = 16 * cg + 4 * g4 + r;
            }
        }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float os = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (os > best || (os == best && oi < bi)) {
            best = os;
            bi = oi;
        }
    }
    if (live && lane < 16) codes[g * 16 + lane] = (uint16_t)bi;
}

// One thread per document d0 + i: the slots of its last group past len get code 0.
__global__ __launch_bounds__(kThreads) void mv_code_tails_kernel(const int2 *__restrict__ table, int d0, int d1,
                                                                 uint16_t *__restrict__ codes)
{
    const int id = d0 + (int)(blockIdx.x * kThreads + threadIdx.x);
    if (id >= d1) return;
    const int2 e = table[id];
    const int64_t base = (int64_t)e.x * 16;
    const int end = (e.y + 15) / 16 * 16;
    for (int j = e.y; j < end; ++j) codes[base + j] = 0;
}

template <int ST>
int launch_assign(const void *store, const float *scales, int64_t g0, int64_t g1, int w, const void *cent,
                  const float *cent_u, int C, uint16_t *codes, hipStream_t s)
{
    const size_t lds = assign_lds_bytes<ST>(w);
    if (lds > (size_t)kLdsBudget) return -1;
    const int64_t blocks = (g1 - g0 + 3) / 4;
    if (blocks > 0x7fffffff) return -1;
    typedef typename Kind<ST>::Block Block;
    mv_assign_kernel<ST><<<(unsigned)blocks, kThreads, lds, s>>>((const Block *)store, scales, g0, g1, w,
                                                                 (const Block *)cent, cent_u, C, codes);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int maxsim_codes_prepare_device()
{
    hipError_t e = allow_lds((const void *)mv_assign_kernel<SEARCH_F16>);
    if (e == hipSuccess) e = allow_lds((const void *)mv_assign_kernel<SEARCH_I8>);
    return e == hipSuccess ? 0 : -1;
}

int launch_mv_assign(const void *store, const float *scales, int storage, const void *d_table, int64_t g0, int64_t g1,
                     int d0, int d1, int w, const void *cent, const float *cent_u, int C, uint16_t *codes, hipStream_t s)
{
    if (g0 < 0 || g1 < g0 || d0 < 0 || d1 < d0 || w % 64 || w < 64 || w > 1024 || C < 16 || C > 65536 || C % 16 || !cent ||
        !codes)
        return -1;
    if ((storage != SEARCH_F16 && storage != SEARCH_I8) || (storage == SEARCH_I8 && (!scales || !cent_u))) return -1;
    if (g1 == g0) return 0;
    const int rc = storage == SEARCH_I8 ? launch_assign<SEARCH_I8>(store, scales, g0, g1, w, cent, cent_u, C, codes, s)
                                        : launch_assign<SEARCH_F16>(store, nullptr, g0, g1, w, cent, nullptr, C, codes, s);
    if (rc != 0 || d1 == d0) return rc;
    mv_code_tails_kernel<<<(unsigned)((d1 - d0 + kThreads - 1) / kThreads), kThreads, 0, s>>>((const int2 *)d_table, d0, d1,
                                                                                              codes);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
