// Residual-coded token storage (BERTX_INDEX_RES2 / _RES4; bert_hip.h "Residual codes";
// mvindex.cpp): a token slot keeps its uint16 centroid code, NB = 2 or 4
// bits per element and one f32 u, and no row.
//
// A stored element is e_i = c_i + wt[b_i], one f16 addition of the centroid's stored f16
// value and the bucket's f16 weight; sim(q, tok) = acc * u with acc the f16 scorer's
// accumulation of q16 . e (maxsim.hip) and u = 1 / sqrt(sum e_i^2), the sum exact.
//
// Bits in HBM, in the order the scorer's lanes want them: per 16-slot group w / 64 units of
// two 32-element blocks; per unit 64 lanes of NB / 2 dwords; lane 16g + f holds row f's
// elements 32 kb + 8g .. + 7 of the unit's blocks, element j of a block at bit NB j.
//   NB 2: one dword, block 2 unit in the low half, block 2 unit + 1 in the high half;
//   NB 4: two dwords, one per block.
// That is the canonical order of bertx_mvindex_doc_residual cut into 2- or 4-byte pieces
// (element i in byte i NB / 8 at bit NB (i mod 8 / NB)); unpack_res_bits below and
// mvindex.cpp's reader are its inverse.
#include "maxsim_common.h"

namespace emb {
namespace {

constexpr int kThreads = 256;      // 4 waves: each scores whole documents / encodes one group on its own
constexpr int kRingUnits = 4;      // prefetch ring per wave: 4 units of 2 gathered chunks and their bits

// The staging table of an add: the call's documents with their first groups counted from
// the call's first group, so that the f16 pack and assign kernels see a store of their own.
__global__ __launch_bounds__(kThreads) void res_rel_table_kernel(const int2 *__restrict__ table, int n_new, int g0,
                                                                 int2 *__restrict__ rel)
{
    const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n_new) return;
    const int2 e = table[i];
    rel[i] = int2{e.x - g0, e.y};
}

// Where the 16-byte chunk (block kb, lane quarter g) of centroid `code` sits in the centroid
// image, less the block: frag_index(code, 4 kb + g, KB) = cent_base(code, g, KB) + 64 kb.
__device__ __forceinline__ uint32_t cent_base(uint32_t code, int g, int KB)
{
    return (code >> 4) * (uint32_t)KB * 64u + 16u * (uint32_t)g + (code & 15u);
}

// Wave v of the grid encodes group v of the staging image (f16 rows, the f16 store's
// layout) whose codes are already written: lane 16g + f takes row f's elements 8g .. 8g + 7
// of every block.  r = f32(v) - f32(c); b = #{k : cut_k < r}; e = c + wt[b] in f16; ss =
// sum e^2 in f64 (exact: every square is a multiple of 2^-48 and ss < 32), the row's four
// lanes added by two shuffles; u = 1 / sqrtf((float)ss).  Slots past a document's len are
// encoded like any other from whatever the staging image holds (their code is 0); they never count.
template <int NB>
__global__ __launch_bounds__(kThreads) void res_encode_kernel(const h16x8 *__restrict__ staging, int groups, int w,
                                                              const uint16_t *__restrict__ codes,
                                                              const h16x8 *__restrict__ cent,
                                                              const float *__restrict__ cuts,
                                                              const uint16_t *__restrict__ wts,
                                                              uint32_t *__restrict__ bits, float *__restrict__ u)
{
    constexpr int NC = (1 << NB) - 1, DW = NB / 2;
    const int lane = threadIdx.x & 63, g4 = lane >> 4;
    const int grp = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (grp >= groups) return;
    const int KB = w >> 5;
    float cut[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) cut[k] = cuts[k];
    const uint32_t code = codes[(size_t)grp * 16 + (lane & 15)];
    const h16x8 *cb = cent + cent_base(code, g4, KB);
    const h16x8 *sb = staging + (size_t)grp * KB * 64 + lane;
    uint32_t *ob = bits + ((size_t)grp * (KB >> 1) * 64 + lane) * DW;
    double ss = 0.0;
    for (int un = 0; un < (KB >> 1); ++un) {
        uint32_t word[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int kb = 2 * un + d;
            const h16x8 v = sb[(size_t)kb * 64], c = cb[(size_t)kb * 64];
            uint32_t m = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float r = add_rn((float)v[j], -(float)c[j]);
                uint32_t b = 0;
#pragma unroll
                for (int k = 0; k < NC; ++k) b += cut[k] < r ? 1u : 0u;
                const h16 e = c[j] + as_h(wts[b]);
                ss += (double)e * (double)e;
                m |= b << (NB * j);
            }
            word[d] = m;
        }
        if constexpr (NB == 2) {
            ob[(size_t)un * 64] = word[0] | (word[1] << 16);
        } else {
            ob[(size_t)un * 128] = word[0];
            ob[(size_t)un * 128 + 1] = word[1];
        }
    }
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lane < 16) {
        const float s = (float)ss;
        // sqrtf, not __fsqrt_rn (maxsim_pack.h unit_scale_i8)
        u[(size_t)grp * 16 + lane] = ss > 0.0 ? __fdiv_rn(1.0f, sqrtf(s)) : 0.f;
    }
}

__host__ __device__ inline size_t res_lds_bytes(int QT, int w, int NB)
{
    return (size_t)QT * 16 * w * 2 + ((size_t)4 << (2 * NB));
}

// maxsim_kernel's skeleton (maxsim.hip): persistent workgroups, the query normalised into B
// fragments in LDS in the prologue (maxsim_common.h pack_queries), beside them the pair
// table pt[b0 | b1 << NB] = the packed f16 (wt[b0], wt[b1]); then wave v of the grid takes candidates v, v + waves, ...
// with no barrier and no cross-wave step.  Per candidate a load cursor runs kRingUnits
// units ahead of the MFMAs: per unit (two blocks of a 16-slot group) lane 16g + f gathers
// the two 16-byte chunks of row f's centroid from the centroid image and loads the unit's
// NB / 2 dwords of bits; the rows' codes come one group at a time, four groups ahead of the
// cursor, and u two groups ahead of its use (loads past the document re-read its last
// group).  A unit is decoded on arrival: two adjacent elements' bits index the pair table
// (one ds_read_b32), one packed f16 add gives two elements of the A fragment.  After a
// group's last block accumulator register r of lane 16g + c is (row 4g + r, query c): it is
// multiplied by u[4g + r], rows >= len become -inf, and the four fold into the lane's
// running maximum.  The epilogue is the scorers' one (maxsim_common.h doc_score).
// Tomb: nothing, the unmasked kernel; or the store's tombstones (const uint32_t *), the masked
// kernel: a deleted document is treated exactly as an id outside [0, n_docs); its bit is read
// for ids in range only.
template <int QT, int NB, class... Tomb>
__global__ __launch_bounds__(kThreads) void maxsim_res_kernel(const uint32_t *__restrict__ bits,
                                                              const float *__restrict__ us,
                                                              const uint16_t *__restrict__ codes,
                                                              const h16x8 *__restrict__ cent,
                                                              const uint32_t *__restrict__ pair,
                                                              const int2 *__restrict__ table, int n_docs,
                                                              const float *__restrict__ q, int Lq, int w,
                                                              const int32_t *__restrict__ ids, int n,
                                                              float *__restrict__ out, Tomb... tomb)
{
    constexpr int DW = NB / 2, NP = 1 << (2 * NB);
    typedef uint32_t Bits __attribute__((ext_vector_type(DW)));
    extern __shared__ uint4 smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int KB = w >> 5, UG = KB >> 1;
    h16x8 *qf = (h16x8 *)smem;                                    // [QT][KB][64]
    const uint32_t *pt = (const uint32_t *)(qf + (size_t)QT * KB * 64);   // [NP]

    pack_queries<SEARCH_F16>(q, Tiles<1>{}, Tiles<QT>{}, Lq, w, qf, nullptr, wv, lane);
    for (int i = tid; i < NP; i += kThreads) ((uint32_t *)pt)[i] = pair[i];
    lds_barrier();

    const int ws = __builtin_amdgcn_readfirstlane(wv);
    const int stride = (int)gridDim.x * 4;
    constexpr int NU = kRingUnits;
    const int g4 = lane >> 4, f = lane & 15;
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
        const int G = (len + 15) >> 4, U = G * UG;
        const Bits *bbase = (const Bits *)bits + (size_t)first * UG * 64 + lane;
        const uint16_t *cbase = codes + (size_t)first * 16 + f;
        const float *ubase = us + (size_t)first * 16 + 4 * g4;
        auto load_code = [&](int gi) { return (uint32_t)cbase[(size_t)min(gi, G - 1) * 16]; };
        auto load_u = [&](int gi) { return *(const float4 *)(ubase + (size_t)min(gi, G - 1) * 16); };

        // the load cursor: group lg, block lkb of it, the codes of groups lg .. lg + 3
        uint32_t cq0 = load_code(0), cq1 = load_code(1), cq2 = load_code(2), cq3 = load_code(3);
        int lg = 0, lkb = 0;
        const h16x8 *crow = cent + cent_base(cq0, g4, KB);
        h16x8 ring[NU][2];
        Bits rbits[NU];
        auto fetch = [&](int j) {
            ring[j][0] = crow[(size_t)lkb * 64];
            ring[j][1] = crow[(size_t)(lkb + 1) * 64];
            rbits[j] = bbase[((size_t)min(lg, G - 1) * UG + (lkb >> 1)) * 64];
            lkb += 2;
            if (lkb == KB) {   // wave-uniform
                lkb = 0;
                ++lg;
                cq0 = cq1;
                cq1 = cq2;
                cq2 = cq3;
                cq3 = load_code(lg + 3);
                crow = cent + cent_base(cq0, g4, KB);
            }
        };
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            fetch(j);
            __builtin_amdgcn_sched_barrier(0);
        }
        float4 u0 = load_u(0), u1 = load_u(1), u2 = load_u(2);
        f32x4 acc[QT];
        float mx[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            mx[t] = -INFINITY;
        }
        int kb = 0, row0 = 4 * g4, cg = 0;
        for (int un0 = 0; un0 < U; un0 += NU) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                if (un0 + j >= U) goto done;   // wave-uniform; no path re-enters the ring out of order
                {
                    const h16x8 c0 = ring[j][0], c1 = ring[j][1];
                    const Bits bw = rbits[j];
                    uint32_t a0[4], a1[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        uint32_t i0, i1;
                        if constexpr (NB == 2) {
                            i0 = (bw[0] >> (4 * p)) & 15u;
                            i1 = (bw[0] >> (16 + 4 * p)) & 15u;
                        } else {
                            i0 = (bw[0] >> (8 * p)) & 255u;
                            i1 = (bw[DW - 1] >> (8 * p)) & 255u;
                        }
                        const h16x2 e0 = h16x2{c0[2 * p], c0[2 * p + 1]} + as_h2(pt[i0]);
                        const h16x2 e1 = h16x2{c1[2 * p], c1[2 * p + 1]} + as_h2(pt[i1]);
                        a0[p] = __builtin_bit_cast(uint32_t, e0);
                        a1[p] = __builtin_bit_cast(uint32_t, e1);
                    }
                    const h16x8 A0 = __builtin_bit_cast(h16x8, uint4{a0[0], a0[1], a0[2], a0[3]});
                    const h16x8 A1 = __builtin_bit_cast(h16x8, uint4{a1[0], a1[1], a1[2], a1[3]});
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        const h16x8 b0 = qf[((size_t)t * KB + kb) * 64 + lane];
                        const h16x8 b1 = qf[((size_t)t * KB + kb + 1) * 64 + lane];
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, b0, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1, b1, acc[t], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    fetch(j);
                    __builtin_amdgcn_sched_barrier(0);
                    kb += 2;
                    if (kb == KB) {
                        const float ur[4] = {u0.x, u0.y, u0.z, u0.w};
#pragma unroll
                        for (int t = 0; t < QT; ++t) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                mx[t] = fmaxf(mx[t], row0 + r < len ? __fmul_rn(acc[t][r], ur[r]) : -INFINITY);
                            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                        kb = 0;
                        row0 += 16;
                        ++cg;
                        u0 = u1;
                        u1 = u2;
                        u2 = load_u(cg + 2);
                    }
                }
            }
        }
    done:
        const float s = doc_score<QT>(mx, Lq, lane);
        if (lane == 0) out[c] = s;
    }
}

template <int NB>
int launch_maxsim_res_nb(const uint32_t *bits, const float *u, const uint16_t *codes, const void *cent, const uint32_t *pair,
                         const void *d_table, int n_docs, int w, const float *d_q, int Lq, const int32_t *d_ids, int n,
                         float *d_out, hipStream_t s, int max_wg, int *ran_wg, const uint32_t *tomb)
{
    const int QT = (Lq + 15) / 16;
    const size_t lds = res_lds_bytes(QT, w, NB);
    if (lds > (size_t)kLdsBudget) return -1;
    const unsigned P = (unsigned)scorer_grid(lds, n, max_wg, ran_wg);
    with_tiles(QT, [&](auto qt) {
        if (tomb)
            maxsim_res_kernel<decltype(qt)::value, NB, const uint32_t *><<<P, kThreads, lds, s>>>(
                bits, u, codes, (const h16x8 *)cent, pair, (const int2 *)d_table, n_docs, d_q, Lq, w, d_ids, n, d_out, tomb);
        else
            maxsim_res_kernel<decltype(qt)::value, NB><<<P, kThreads, lds, s>>>(
                bits, u, codes, (const h16x8 *)cent, pair, (const int2 *)d_table, n_docs, d_q, Lq, w, d_ids, n, d_out);
    });
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int maxsim_res_prepare_device()
{
    hipError_t e = hipSuccess;
    for (int qt = 1; qt <= 4 && e == hipSuccess; ++qt)
        with_tiles(qt, [&](auto QT) {
            e = allow_lds((const void *)maxsim_res_kernel<decltype(QT)::value, 2>);
            if (e == hipSuccess) e = allow_lds((const void *)maxsim_res_kernel<decltype(QT)::value, 4>);
            if (e == hipSuccess) e = allow_lds((const void *)maxsim_res_kernel<decltype(QT)::value, 2, const uint32_t *>);
            if (e == hipSuccess) e = allow_lds((const void *)maxsim_res_kernel<decltype(QT)::value, 4, const uint32_t *>);
        });
    return e == hipSuccess ? 0 : -1;
}

int launch_res_rel_table(const void *d_table_new, int n_new, int64_t g0, void *d_rel, hipStream_t s)
{
    if (n_new < 1 || g0 < 0 || g0 > 0x7fffffffll || !d_table_new || !d_rel) return -1;
    res_rel_table_kernel<<<(unsigned)((n_new + kThreads - 1) / kThreads), kThreads, 0, s>>>((const int2 *)d_table_new, n_new,
                                                                                           (int)g0, (int2 *)d_rel);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_res_encode(const void *staging, int64_t groups, int w, int nbits, const uint16_t *codes, const void *cent,
                      const float *cuts, const uint16_t *wts, uint32_t *bits, float *u, hipStream_t s)
{
    if (groups < 0 || groups > 0x7ffffff0ll || w % 64 || w < 64 || w > 1024 || (nbits != 2 && nbits != 4) || !staging ||
        !codes || !cent || !cuts || !wts || !bits || !u)
        return -1;
    if (groups == 0) return 0;
    const unsigned blocks = (unsigned)((groups + 3) / 4);
    if (nbits == 2)
        res_encode_kernel<2><<<blocks, kThreads, 0, s>>>((const h16x8 *)staging, (int)groups, w, codes, (const h16x8 *)cent,
                                                         cuts, wts, bits, u);
    else
        res_encode_kernel<4><<<blocks, kThreads, 0, s>>>((const h16x8 *)staging, (int)groups, w, codes, (const h16x8 *)cent,
                                                         cuts, wts, bits, u);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_maxsim_res(const uint32_t *bits, const float *u, const uint16_t *codes, const void *cent, const uint32_t *pair,
                      int nbits, const void *d_table, int n_docs, int w, const float *d_q, int Lq, const int32_t *d_ids, int n,
                      float *d_out, hipStream_t s, int max_wg, int *ran_wg, const uint32_t *tomb)
{
    if (Lq < 1 || Lq > 64 || n < 1 || n > 0x7fff0000 || n_docs < 0 || w % 64 || w < 64 || w > 1024 ||
        (nbits != 2 && nbits != 4) || !bits || !u || !pair)
        return -1;   // (codes and cent are read for stored documents only, which need them to exist)
    return nbits == 2 ? launch_maxsim_res_nb<2>(bits, u, codes, cent, pair, d_table, n_docs, w, d_q, Lq, d_ids, n, d_out, s,
                                                max_wg, ran_wg, tomb)
                      : launch_maxsim_res_nb<4>(bits, u, codes, cent, pair, d_table, n_docs, w, d_q, Lq, d_ids, n, d_out, s,
                                                max_wg, ran_wg, tomb);
}

}  // namespace emb
