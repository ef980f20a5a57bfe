// The ColBERT projector (bert_hip.h "Projection"): the final-LayerNorm row
// of a token, rounded to f16 in registers, times the file's linear.weight, then scaled
// to unit length -- the rows launch_mv_pack and bertx_mvindex_add_device take.
//
//   x     the row's final-LayerNorm values, the bits of the per-token output
//         (f16 chain: tokens_f32_kernel's fmaf(r, z, fmaf(-mean r, gamma, beta));
//          f32 / q8 chains: the row of the final f32 buffer)
//   a_k   = f16(x_k), w_jk = f16(W_jk) (at load, engine.cpp build_proj_image)
//   p_j   = sum_k a_k w_jk: v_mfma_f32_16x16x32_f16 over ascending blocks of 32 k, f32 from 0
//   ss    = sum_{j < dim} p_j p_j: per lane its 4 dim / 64 .. features in ascending order,
//           then the lanes 16, then 32 apart; every product and sum rounded on its own
//   out_j = p_j * (1 / sqrt(ss)) (sqrt, then the division), the row +0 where ss == 0;
//           +0 for dim <= j < width
//
// W image: width = 64 ceil(dim / 64) rows (rows >= dim zero) in the SEARCH_F16 block
// order, block (kb, t) = features 16t .. 16t + 15 x k 32kb .. 32kb + 31 at
// (kb * width / 16 + t) * 1 KiB, lane 16g + f = feature 16t + f, elements 8g .. 8g + 7.
//
// Shape: workgroups of 4 waves and 64 output rows, 16 rows per wave.  W is the MFMA's A
// operand (features on the tile's rows), the wave's 16 token rows the B operand, built
// from the wave's own rows in registers: accumulator register r of lane 16g + c of tile
// t is (feature 16t + 4g + r, token c), so a token's squares add up inside a lane and
// over two shuffles, and a lane stores 4 consecutive floats per tile.  W streams
// through LDS in slices of 64 k shared by the four waves (2 KiB per tile: 32 KiB at
// width 256); the next slice is in flight from L2 while the current one multiplies.
// A row's result depends on that row's x and on W only: no value crosses tokens.
#include "device_common.h"
#include "kernels.h"

namespace emb {
namespace {

constexpr int kThreads = 256;
constexpr int kSliceBlocks = 2;   // K-blocks of 32 per LDS slice (d % 64 == 0)

// NT = width / 16 feature tiles.  Z16: src is z f16 [>= rows][d] with st, lw, lb (the f16
// chain); else x f32 [rows][d].  rows (or null: the identity): output row i projects
// source row rows[i].  Output rows past n_out - 1 are computed on row n_out - 1's source
// (a valid row) and never stored.
template <int NT, bool Z16>
__global__ __launch_bounds__(kThreads) void project_kernel(const void *__restrict__ src, const float2 *__restrict__ st,
                                                           const float *__restrict__ lw, const float *__restrict__ lb,
                                                           int d, const h16x8 *__restrict__ wimg, int dim,
                                                           const int32_t *__restrict__ rows, int n_out,
                                                           float *__restrict__ out)
{
    __shared__ h16x8 wl[kSliceBlocks * NT * 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int S = d >> 6;   // slices
    const int64_t i = (int64_t)blockIdx.x * 64 + wv * 16 + c;   // this lane's token: its output row
    const int64_t ic = i < n_out ? i : (int64_t)n_out - 1;
    const size_t r = rows ? (size_t)rows[ic] : (size_t)ic;
    float rs = 0.f, t0 = 0.f;
    if constexpr (Z16) {
        const float2 s2 = st[r];
        rs = s2.y;
        t0 = -s2.x * s2.y;
    }
    const size_t row_off = r * (size_t)d + 8 * g;

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    constexpr int PER = kSliceBlocks * NT * 64 / kThreads;   // 16-byte units per thread and slice
    h16x8 pre[PER];
    auto fetch = [&](int s) {
#pragma unroll
        for (int j = 0; j < PER; ++j) pre[j] = wimg[(size_t)s * (kSliceBlocks * NT * 64) + j * kThreads + tid];
    };
    fetch(0);
    for (int s = 0; s < S; ++s) {
        if (s) lds_barrier();   // every wave has read the previous slice
#pragma unroll
        for (int j = 0; j < PER; ++j) wl[j * kThreads + tid] = pre[j];
        lds_barrier();
        if (s + 1 < S) fetch(s + 1);
#pragma unroll
        for (int kk = 0; kk < kSliceBlocks; ++kk) {
            const int k0 = 32 * (kSliceBlocks * s + kk);
            h16x8 b;
            if constexpr (Z16) {
                const h16x8 y = *(const h16x8 *)((const h16 *)src + row_off + k0);
                const f32x4 w0 = *(const f32x4 *)(lw + k0 + 8 * g), w1 = *(const f32x4 *)(lw + k0 + 8 * g + 4);
                const f32x4 b0 = *(const f32x4 *)(lb + k0 + 8 * g), b1 = *(const f32x4 *)(lb + k0 + 8 * g + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    b[e] = (h16)fmaf(rs, (float)y[e], fmaf(t0, w0[e], b0[e]));
                    b[4 + e] = (h16)fmaf(rs, (float)y[4 + e], fmaf(t0, w1[e], b1[e]));
                }
            } else {
                const float *x = (const float *)src + row_off + k0;
                const f32x4 x0 = *(const f32x4 *)x, x1 = *(const f32x4 *)(x + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    b[e] = (h16)x0[e];
                    b[4 + e] = (h16)x1[e];
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[(kk * NT + t) * 64 + lane], b, acc[t], 0, 0, 0);
        }
    }

    // register r of tile t: feature 16t + 4g + r of token c (dim % 32 == 0: a lane's four
    // features of a tile are all below dim or all padding)
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (16 * t + 4 * g < dim) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ss = add_rn(ss, mul_rn(acc[t][e], acc[t][e]));
        }
    ss = add_rn(ss, __shfl_xor(ss, 16, 64));
    ss = add_rn(ss, __shfl_xor(ss, 32, 64));
    const bool zero = ss == 0.f;
    const float rinv = zero ? 0.f : __fdiv_rn(1.0f, __fsqrt_rn(ss));
    if (i >= n_out) return;
    float *o = out + (size_t)i * (16 * NT) + 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!zero && 16 * t + 4 * g < dim) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = mul_rn(acc[t][e], rinv);
        }
        *(f32x4 *)(o + 16 * t) = v;
    }
}

template <bool Z16>
int launch(int NT, unsigned blocks, hipStream_t s, const void *src, const float2 *st, const float *lw, const float *lb,
           int d, const h16x8 *wimg, int dim, const int32_t *rows, int n_out, float *out)
{
    switch (NT) {
    case 4: project_kernel<4, Z16><<<blocks, kThreads, 0, s>>>(src, st, lw, lb, d, wimg, dim, rows, n_out, out); break;
    case 8: project_kernel<8, Z16><<<blocks, kThreads, 0, s>>>(src, st, lw, lb, d, wimg, dim, rows, n_out, out); break;
    case 12: project_kernel<12, Z16><<<blocks, kThreads, 0, s>>>(src, st, lw, lb, d, wimg, dim, rows, n_out, out); break;
    case 16: project_kernel<16, Z16><<<blocks, kThreads, 0, s>>>(src, st, lw, lb, d, wimg, dim, rows, n_out, out); break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

int launch_project(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b, const float *x32,
                   int32_t d, const void *wimg, int32_t dim, const int32_t *d_rows, int32_t n_out, float *out,
                   hipStream_t s)
{
    if (d % 64 || d < 64 || d > 1024 || dim % 32 || dim < 32 || dim > 256 || n_out < 1 || !wimg || !out) return -1;
    if ((z != nullptr) == (x32 != nullptr) || (z && (!stats || !ln_w || !ln_b))) return -1;
    const int NT = (dim + 63) / 64 * 4;
    const unsigned blocks = (unsigned)(((int64_t)n_out + 63) / 64);
    if (z) return launch<true>(NT, blocks, s, z, stats, ln_w, ln_b, d, (const h16x8 *)wimg, dim, d_rows, n_out, out);
    return launch<false>(NT, blocks, s, x32, nullptr, nullptr, nullptr, d, (const h16x8 *)wimg, dim, d_rows, n_out, out);
}

}  // namespace emb
