// SPLADE sparse term weights (bert_hip.h "Sparse"): the masked-LM head of a
// BertForMaskedLM checkpoint with its decoder fused into a per-sentence max-pool.
//
//   x     the row's final-LayerNorm values, the bits of the per-token output (the two
//         source forms of project.hip); a_k = f16(x_k)
//   u_j   = bt_j + sum_k a_k f16(Wt_jk)     f32 MFMA over ascending blocks of 32 k
//   g_j   = 0.5 u_j (1 + erff(u_j * 0.70710678f))
//   h_j   = f16((g_j - mean) * rstd * gamma_j + beta_j), mean = sum_j g_j / d,
//           rstd = 1 / sqrt(sum_j (g_j - mean)^2 / d + 1e-5); both sums: per lane its
//           features in ascending order, the lanes 16 then 32 apart, then the four
//           waves in index order -- an order that depends on d only
//   l_v   = sum_k h_k f16(E_vk)             f32 MFMA, ascending k
//   m_v   = max over the sentence's rows of l_v, + b_v (rounding is monotone: the bits
//           of max (l_v + b_v))
//   w_v   = log1pf(m_v > 0 ? m_v : +0)
//
// Both weight images are in the block order of build_proj_image (engine.h
// build_rows_image): block (kb, t) = rows 16t .. 16t + 15 x k 32kb .. 32kb + 31 at
// (kb * rows / 16 + t) KiB, lane 16g + f = row 16t + f, elements 8g .. 8g + 7.
//
// Transform: a workgroup of 4 waves owns 32 token rows.  Wt is the MFMA's A operand
// (features on the tile's rows), the tokens the B operand built in registers from the
// source row, two token tiles per wave; wave w owns the feature tiles w, w + 4, .. (d / 64
// of them), so a row's LayerNorm sums meet through LDS.  Wt streams through LDS one
// 32-k block of all d features at a time (d * 64 bytes), the next block in flight.
//
// Decoder: a workgroup of 4 waves (2 x 2) owns 128 tokens x 128 terms, each wave 64 x 64
// as 4 x 4 MFMA tiles; tokens are the A operand, terms the B operand, so accumulator
// register r of lane 16g + c is (token 4g + r, term c).  Both operands go through LDS
// in slices of 64 k (16 KiB each), the next slice's global loads in flight while the
// current one multiplies.  The logits stay in registers: per sentence that meets the
// token tile a lane takes the max over its rows, two shuffles fold g, the bias is
// added, and the positive results go to the +0-filled output by atomicMax on their bits
// (non-negative floats order as unsigned integers: exact and order-free).  A tile
// inside one sentence skips the row masks.
#include "device_common.h"
#include "kernels.h"

namespace emb {
namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------------------------
// transform
// ---------------------------------------------------------------------------------
constexpr int kTfRows = 32;   // token rows per workgroup

__device__ __forceinline__ float gelu_erf(float u)
{
    return mul_rn(mul_rn(0.5f, u), add_rn(1.0f, erff(mul_rn(u, 0.70710678f))));
}

// the sum of v over the lanes that hold one token (16 and 32 apart), then over the four
// waves in index order through part[wave][32]; every wave returns the same bits
__device__ __forceinline__ void token_sums(float (&v)[2], float *part, int wv, int lane)
{
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        v[tt] = add_rn(v[tt], __shfl_xor(v[tt], 16, 64));
        v[tt] = add_rn(v[tt], __shfl_xor(v[tt], 32, 64));
    }
    lds_barrier();   // the previous use of part is over
    if (lane < 16) {
        part[wv * 32 + lane] = v[0];
        part[wv * 32 + 16 + lane] = v[1];
    }
    lds_barrier();
    const int c = lane & 15;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        float s = part[16 * tt + c];
#pragma unroll
        for (int w = 1; w < 4; ++w) s = add_rn(s, part[w * 32 + 16 * tt + c]);
        v[tt] = s;
    }
}

// NTW: the most feature tiles a wave owns (d <= 256 NTW); it owns d / 64 of them.
// Token rows past T - 1 are computed on row T - 1's source and never stored.
template <int NTW, bool Z16>
__global__ __launch_bounds__(kThreads) void sparse_transform_kernel(const void *__restrict__ src,
                                                                    const float2 *__restrict__ st,
                                                                    const float *__restrict__ lw,
                                                                    const float *__restrict__ lb, int d,
                                                                    const h16x8 *__restrict__ wimg,
                                                                    const float *__restrict__ bt,
                                                                    const float *__restrict__ gamma,
                                                                    const float *__restrict__ beta, int T,
                                                                    h16 *__restrict__ h)
{
    __shared__ h16x8 wl[NTW * 4 * 64];   // one 32-k block of all d features (64 KiB at d = 1024)
    float *part = (float *)wl;           // the LayerNorm partials [wave][32], once the K loop is over
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int KB = d >> 5, ntw = d >> 6, units = (d >> 4) * 64;   // 16-byte units per block

    int64_t row[2];
    size_t off[2];
    float rs[2] = {0.f, 0.f}, t0[2] = {0.f, 0.f};
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        row[tt] = (int64_t)blockIdx.x * kTfRows + 16 * tt + c;
        const size_t r = (size_t)(row[tt] < T ? row[tt] : (int64_t)T - 1);
        if constexpr (Z16) {
            const float2 s2 = st[r];
            rs[tt] = s2.y;
            t0[tt] = -s2.x * s2.y;
        }
        off[tt] = r * (size_t)d + 8 * g;
    }

    f32x4 acc[2][NTW];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int i = 0; i < NTW; ++i) acc[tt][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    h16x8 pre[NTW];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int j = 0; j < NTW; ++j)
            if (j * kThreads < units) pre[j] = wimg[(size_t)kb * units + j * kThreads + tid];
    };
    fetch(0);
    for (int kb = 0; kb < KB; ++kb) {
        if (kb) lds_barrier();   // every wave has read the previous block
#pragma unroll
        for (int j = 0; j < NTW; ++j)
            if (j * kThreads < units) wl[j * kThreads + tid] = pre[j];
        lds_barrier();
        if (kb + 1 < KB) fetch(kb + 1);
        const int k0 = 32 * kb;
        h16x8 b[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            if constexpr (Z16) {
                const h16x8 y = *(const h16x8 *)((const h16 *)src + off[tt] + k0);
                const f32x4 w0 = *(const f32x4 *)(lw + k0 + 8 * g), w1 = *(const f32x4 *)(lw + k0 + 8 * g + 4);
                const f32x4 b0 = *(const f32x4 *)(lb + k0 + 8 * g), b1 = *(const f32x4 *)(lb + k0 + 8 * g + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    b[tt][e] = (h16)fmaf(rs[tt], (float)y[e], fmaf(t0[tt], w0[e], b0[e]));
                    b[tt][4 + e] = (h16)fmaf(rs[tt], (float)y[4 + e], fmaf(t0[tt], w1[e], b1[e]));
                }
            } else {
                const float *x = (const float *)src + off[tt] + k0;
                const f32x4 x0 = *(const f32x4 *)x, x1 = *(const f32x4 *)(x + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    b[tt][e] = (h16)x0[e];
                    b[tt][4 + e] = (h16)x1[e];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i)
            if (i < ntw) {
                const h16x8 a = wl[(4 * i + wv) * 64 + lane];
                acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[0], acc[0][i], 0, 0, 0);
                acc[1][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[1], acc[1][i], 0, 0, 0);
            }
    }

    // register e of tile i: feature 16 (4i + wv) + 4g + e of token c
    float sum[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NTW; ++i)
        if (i < ntw) {
            const f32x4 bb = *(const f32x4 *)(bt + 16 * (4 * i + wv) + 4 * g);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[tt][i][e] = gelu_erf(add_rn(acc[tt][i][e], bb[e]));
                    sum[tt] = add_rn(sum[tt], acc[tt][i][e]);
                }
        }
    token_sums(sum, part, wv, lane);
    const float mean[2] = {__fdiv_rn(sum[0], (float)d), __fdiv_rn(sum[1], (float)d)};
    float m2[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NTW; ++i)
        if (i < ntw) {
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[tt][i][e] = add_rn(acc[tt][i][e], -mean[tt]);
                    m2[tt] = add_rn(m2[tt], mul_rn(acc[tt][i][e], acc[tt][i][e]));
                }
        }
    token_sums(m2, part, wv, lane);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        if (row[tt] >= T) continue;
        const float rstd = __fdiv_rn(1.0f, __fsqrt_rn(add_rn(__fdiv_rn(m2[tt], (float)d), 1e-5f)));
#pragma unroll
        for (int i = 0; i < NTW; ++i)
            if (i < ntw) {
                const int j = 16 * (4 * i + wv) + 4 * g;
                const f32x4 ga = *(const f32x4 *)(gamma + j), be = *(const f32x4 *)(beta + j);
                h16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (h16)add_rn(mul_rn(mul_rn(acc[tt][i][e], rstd), ga[e]), be[e]);
                *(h16x4 *)(h + (size_t)row[tt] * d + j) = o;
            }
    }
}

template <bool Z16>
int launch_tf(int d, unsigned blocks, hipStream_t s, const void *src, const float2 *st, const float *lw, const float *lb,
              const h16x8 *wimg, const float *bt, const float *gamma, const float *beta, int T, h16 *h)
{
#define SPARSE_TF(N) sparse_transform_kernel<N, Z16><<<blocks, kThreads, 0, s>>>(src, st, lw, lb, d, wimg, bt, gamma, beta, T, h)
    if (d <= 256) SPARSE_TF(4);
    else if (d <= 512) SPARSE_TF(8);
    else if (d <= 768) SPARSE_TF(12);
    else SPARSE_TF(16);
#undef SPARSE_TF
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---------------------------------------------------------------------------------
// decoder with the fused segmented max
// ---------------------------------------------------------------------------------
constexpr int kBM = 128, kBN = kSparseVocabTile, kSlice = 64;   // tokens, terms, k per LDS slice
constexpr int kGroup = 16;   // token tiles that walk the vocab tiles together (launch order)
static_assert(kBN == 128, "the decoder's wave layout is 2 x 2 waves of 64 x 64");

__global__ __launch_bounds__(kThreads) void sparse_fill_kernel(uint32_t *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = 0u;
}

__global__ __launch_bounds__(kThreads) void sparse_finish_kernel(float *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = log1pf(out[i]);
}

// h f16 [T][d]; eimg: the decoder image of VT vocab tiles; out uint32 view of f32
// [n_seqs][V], +0 before the launch.  Grid: groups of kGroup token tiles, each group
// walking every vocab tile (id = (group * VT + vt) * kGroup + tile in group).
__global__ __launch_bounds__(kThreads) void sparse_decoder_kernel(const h16 *__restrict__ h, int T, int d,
                                                                  const h16x8 *__restrict__ eimg, int VT, int V,
                                                                  const float *__restrict__ bias,
                                                                  const int32_t *__restrict__ cu, int n_seqs,
                                                                  int MT, uint32_t *__restrict__ out)
{
    __shared__ h16x8 al[2 * 8 * 64], bl[2 * 8 * 64];   // [kk][tile][lane], 16 KiB each
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 15, g = lane >> 4, wm = wv >> 1, wn = wv & 1;
    const int grp = blockIdx.x / (VT * kGroup), rem = blockIdx.x % (VT * kGroup);
    const int mt = grp * kGroup + rem % kGroup, vt = rem / kGroup;
    if (mt >= MT) return;   // (the last group's missing tiles; uniform, before any barrier)
    const int m0 = mt * kBM, n0 = vt * kBN, S = d / kSlice;
    const size_t NT = (size_t)VT * (kBN / 16);   // 16-row blocks per k block of the image

    // A: thread -> (row 32j + tid / 8, the 8 k at 8 (tid % 8)); rows past T - 1 read row T - 1
    const int aq = tid & 7, ar = tid >> 3;
    const h16 *ap[4];
    int au[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 32 * j + ar, rr = m0 + r < T ? m0 + r : T - 1;
        ap[j] = h + (size_t)rr * d + 8 * aq;
        au[j] = ((aq >> 2) * 8 + (r >> 4)) * 64 + 16 * (aq & 3) + (r & 15);
    }
    h16x8 pa[4], pb[4];
    auto fetch = [&](int s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pa[j] = *(const h16x8 *)(ap[j] + s * kSlice);
            const int u = j * kThreads + tid;   // [kk][tile][lane]
            pb[j] = eimg[((size_t)(2 * s + (u >> 9)) * NT + (size_t)vt * 8) * 64 + (u & 511)];
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int s = 0; s < S; ++s) {
        if (s) lds_barrier();   // every wave has read the previous slice
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            al[au[j]] = pa[j];
            bl[j * kThreads + tid] = pb[j];
        }
        lds_barrier();
        if (s + 1 < S) fetch(s + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            h16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = al[(kk * 8 + 4 * wm + i) * 64 + lane];
                b[i] = bl[(kk * 8 + 4 * wn + i) * 64 + lane];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // acc[i][j][r]: token m0 + 64 wm + 16 i + 4 g + r, term n0 + 64 wn + 16 j + c
    const int w0 = m0 + 64 * wm, w1 = w0 + 64;   // this wave's rows
    float bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 64 * wn + 16 * j + c;
        bv[j] = n < V ? bias[n] : 0.f;
    }
    auto store = [&](int sq, const float (&m)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = fmaxf(m[j], __shfl_xor(m[j], 16, 64));
            v = fmaxf(v, __shfl_xor(v, 32, 64));
            v = add_rn(v, bv[j]);
            const int n = n0 + 64 * wn + 16 * j + c;
            if (g == 0 && n < V && v > 0.f) atomicMax(out + (size_t)sq * V + n, __builtin_bit_cast(uint32_t, v));
        }
    };
    // the first sentence that ends behind m0
    int lo = 0, hi = n_seqs;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid + 1] > m0) hi = mid; else lo = mid + 1;
    }
    for (int sq = lo; sq < n_seqs; ++sq) {
        const int r0 = cu[sq], r1 = cu[sq + 1];
        if (r0 >= m0 + kBM) break;
        if (r1 <= w0 || r0 >= w1) continue;   // none of this wave's rows (uniform)
        float m[4];
        if (r0 <= w0 && r1 >= w1) {
            // every row of the wave is the sentence's
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = acc[0][j][0];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v = fmaxf(v, acc[i][j][r]);
                m[j] = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = -__builtin_inff();
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = w0 + 16 * i + 4 * g + r;
                    if (t >= r0 && t < r1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], acc[i][j][r]);
                    }
                }
        }
        store(sq, m);
    }
}

}  // namespace

int launch_sparse_transform(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b,
                            const float *x32, int32_t d, const void *wimg, const float *bt, const float *gamma,
                            const float *beta, int32_t T, uint16_t *h, hipStream_t s)
{
    if (d % 64 || d < 64 || d > 1024 || T < 1 || !wimg || !bt || !gamma || !beta || !h) return -1;
    if ((z != nullptr) == (x32 != nullptr) || (z && (!stats || !ln_w || !ln_b))) return -1;
    const unsigned blocks = (unsigned)(((int64_t)T + kTfRows - 1) / kTfRows);
    if (z) return launch_tf<true>(d, blocks, s, z, stats, ln_w, ln_b, (const h16x8 *)wimg, bt, gamma, beta, T, (h16 *)h);
    return launch_tf<false>(d, blocks, s, x32, nullptr, nullptr, nullptr, (const h16x8 *)wimg, bt, gamma, beta, T, (h16 *)h);
}

int launch_sparse_decoder(const uint16_t *h, int32_t T, int32_t d, const void *eimg, int32_t V, const float *bias,
                          const int32_t *cu, int32_t n_seqs, float *out, hipStream_t s)
{
    if (d % 64 || d < 64 || d > 1024 || T < 1 || V < 1 || n_seqs < 1 || !h || !eimg || !bias || !cu || !out) return -1;
    const size_t n = (size_t)n_seqs * V;
    const int64_t MT = ((int64_t)T + kBM - 1) / kBM, VT = ((int64_t)V + kBN - 1) / kBN;
    const int64_t blocks = (MT + kGroup - 1) / kGroup * kGroup * VT, fb = (int64_t)((n + kThreads - 1) / kThreads);
    if (blocks > 0x7fffffff || fb > 0x7fffffff) return -1;
    sparse_fill_kernel<<<(unsigned)fb, kThreads, 0, s>>>((uint32_t *)out, n);
    sparse_decoder_kernel<<<(unsigned)blocks, kThreads, 0, s>>>((const h16 *)h, T, d, (const h16x8 *)eimg, (int)VT, V, bias,
                                                                cu, n_seqs, (int)MT, (uint32_t *)out);
    sparse_finish_kernel<<<(unsigned)fb, kThreads, 0, s>>>(out, n);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
