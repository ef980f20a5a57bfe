// The q8-activation chain's two quantized kernels (q4_0 / q4_1 / q8_0 files,
// activation mode 1): the reference re-quantizes every GEMM input row to q8_0
// (q4_0, q8_0 weights) or q8_1 (q4_1 weights) per 32-element block and takes
// integer block dots (ggml through bert.cpp:995-1016, 1040, 1059, 1066;
// oracle/bert_oracle.c matmul).  Per projection Y = X W^T:
//   1. q8_quantize_kernel: X f32 [M][K] -> int8 [M][K], block scales (and the
//      q8_1 sums) as era_quantize_row_q8_0 / _q8_1 compute them, bit for bit;
//   2. q8_gemm_kernel: per block the exact integer dot on v_mfma_i32_16x16x32_i8
//      (K = 32 = one block), its term in f32 with the oracle's roundings (mul_rn /
//      add_rn: no contraction), terms added in ascending block order into an f32 accumulator.
// Every other kernel of the chain is the f32 chain's (f32.hip) in its exact
// instantiation (uncontracted LayerNorm, attention and pool sums in the
// reference's order): a last-bit difference in a projection's input becomes
// whole rounding steps of its quantizer.
#include "device_common.h"
#include "host_common.h"
#include "kernels.h"

namespace emb {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// One thread per 4 elements, 8 lanes per block.  Rows >= T (tile padding) are
// quantized as zeros without being read.  Scale planes are block-major,
// d[b * M + row], so the GEMM reads a lane's four rows as one 16-B word.
// KIND 0 (q8_0): d holds f32(f16(amax / 127)), the scale the dot uses; KIND 1
// (q8_1): d the f32 scale itself, s = (float)(sum q) * d.
template <int KIND>
__global__ __launch_bounds__(256) void q8_quantize_kernel(const float *__restrict__ X, int T, int M, int K,
                                                          int8_t *__restrict__ q, float *__restrict__ d,
                                                          float *__restrict__ s)
{
    const int k4 = K / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)M * k4) return;   // (whole 8-lane groups: K % 32 == 0)
    const int row = (int)(idx / k4), c4 = (int)(idx % k4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < T) v = *(const f32x4 *)(X + (size_t)row * K + 4 * c4);
    float amax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
#pragma unroll
    for (int o = 1; o <= 4; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float dd = __fdiv_rn(amax, 127.0f);
    const float id = dd != 0.f ? __fdiv_rn(1.0f, dd) : 0.f;
    int qi[4], si = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        qi[e] = (int)roundf(mul_rn(v[e], id));   // ties away from zero, as roundf
        si += qi[e];
    }
    *(uint32_t *)(q + (size_t)row * K + 4 * c4) = (uint32_t)(qi[0] & 255) | ((uint32_t)(qi[1] & 255) << 8) |
                                                  ((uint32_t)(qi[2] & 255) << 16) | ((uint32_t)(qi[3] & 255) << 24);
    if (KIND == 1) {
#pragma unroll
        for (int o = 1; o <= 4; o <<= 1) si += __shfl_xor(si, o, 64);
    }
    if ((threadIdx.x & 7) == 0) {
        const size_t o = (size_t)(c4 / 8) * M + row;
        d[o] = KIND == 0 ? (float)(h16)dd : dd;
        if (KIND == 1) s[o] = mul_rn((float)si, dd);
    }
}

// nibble values 0 .. 15 in the four bytes of v -> v - 8 per byte (int8), no
// borrow between the bytes
__device__ __forceinline__ uint32_t unbias8(uint32_t v) { return ((v | 0x80808080u) - 0x08080808u) ^ 0x80808080u; }

__device__ __forceinline__ long pack64(uint32_t lo, uint32_t hi) { return (long)((uint64_t)lo | ((uint64_t)hi << 32)); }

// Y[m][n] = epi(sum_b term_b(m, n)) on 64-token x 64-feature tiles: 4 waves of
// 32 tokens x 32 features (one weight group of the lane-order layout, kernels.h),
// no LDS: per K-step (two blocks) a lane reads its own weight record (the B
// operands of the four fragments u = 2a + s: lane 16g + f = elements 8g .. 8g+7 of
// feature f), unpacks it in registers, and reads the A operands (token l & 15,
// the same eight elements) from the int8 rows.  The element order inside a
// lane's eight bytes is the weight record's (q4: e0 e4 e1 e5 e2 e6 e3 e7; q8_0:
// e0 e2 e1 e3 e4 e6 e5 e7): the X bytes are permuted to match, an integer sum
// does not care.  D: lane = feature l & 15, registers = tokens 4 (l >> 4) + r.
// Each block's i32 result is converted and scaled into the f32 accumulator of
// its output, blocks in ascending order whatever the tile (so a sentence's bits
// do not depend on its batch).  EPI as f32_gemm_kernel.
template <int FMT, int EPI>
__global__ __launch_bounds__(256) void q8_gemm_kernel(const void *__restrict__ wq, const uint16_t *__restrict__ wd,
                                                      const uint16_t *__restrict__ wmn,
                                                      const int8_t *__restrict__ xq, const float *__restrict__ xd,
                                                      const float *__restrict__ xs, const float *__restrict__ bias,
                                                      const float *__restrict__ res, float *__restrict__ Y, int M,
                                                      int N, int K, int nN, const uint16_t *__restrict__ gelu_tab)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int G = N / 32;
    const int m0 = (blockIdx.x / nN) * 64 + 32 * (w >> 1);
    const int grp = (blockIdx.x % nN) * 2 + (w & 1);
    if (grp >= G) return;   // whole waves, and the kernel has no barrier
    const int f = lane & 15, g = lane >> 4;
    float acc[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][a][r] = 0.f;
    const int8_t *xrow = xq + (size_t)(m0 + f) * K + 8 * g;   // tile i: + 16 i K
    const int srow = m0 + 4 * g;                               // tile i: + 16 i
    const i32x4 zero = {0, 0, 0, 0};
    for (int ks = 0; ks < K / 64; ++ks) {
        const size_t rec = ((size_t)ks * G + grp) * 64 + lane;
        long bw[4];
        if (FMT == FMT_Q8_0) {
            const uint4 v0 = ((const uint4 *)wq)[2 * rec], v1 = ((const uint4 *)wq)[2 * rec + 1];
            bw[0] = pack64(v0.x ^ 0x80808080u, v0.y ^ 0x80808080u);
            bw[1] = pack64(v0.z ^ 0x80808080u, v0.w ^ 0x80808080u);
            bw[2] = pack64(v1.x ^ 0x80808080u, v1.y ^ 0x80808080u);
            bw[3] = pack64(v1.z ^ 0x80808080u, v1.w ^ 0x80808080u);
        } else {
            const uint4 v = ((const uint4 *)wq)[rec];
            const uint32_t wu[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                uint32_t lo = wu[u] & 0x0F0F0F0Fu, hi = (wu[u] >> 4) & 0x0F0F0F0Fu;
                if (FMT == FMT_Q4_0) { lo = unbias8(lo); hi = unbias8(hi); }
                bw[u] = pack64(lo, hi);
            }
        }
        const size_t di = ((size_t)ks * G + grp) * 16 + f;   // four f16 (u = 0 .. 3) per feature
        const uint2 dv = ((const uint2 *)wd)[di];
        const float wdf[4] = {(float)as_h((uint16_t)dv.x), (float)as_h((uint16_t)(dv.x >> 16)),
                              (float)as_h((uint16_t)dv.y), (float)as_h((uint16_t)(dv.y >> 16))};
        float wmf[4] = {0.f, 0.f, 0.f, 0.f};
        if (FMT == FMT_Q4_1) {
            const uint2 mv = ((const uint2 *)wmn)[di];
            wmf[0] = (float)as_h((uint16_t)mv.x); wmf[1] = (float)as_h((uint16_t)(mv.x >> 16));
            wmf[2] = (float)as_h((uint16_t)mv.y); wmf[3] = (float)as_h((uint16_t)(mv.y >> 16));
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const size_t so = (size_t)(2 * ks + s) * M + srow;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint2 xv = *(const uint2 *)(xrow + (size_t)16 * i * K + 64 * ks + 32 * s);
                uint32_t lo, hi;
                if (FMT == FMT_Q8_0) {   // e0 e2 e1 e3 | e4 e6 e5 e7
                    lo = (xv.x & 0xFF0000FFu) | ((xv.x & 0x0000FF00u) << 8) | ((xv.x >> 8) & 0x0000FF00u);
                    hi = (xv.y & 0xFF0000FFu) | ((xv.y & 0x0000FF00u) << 8) | ((xv.y >> 8) & 0x0000FF00u);
                } else {                 // e0 e4 e1 e5 | e2 e6 e3 e7
                    lo = (xv.x & 0xFFu) | ((xv.y & 0xFFu) << 8) | ((xv.x & 0xFF00u) << 8) | ((xv.y & 0xFF00u) << 16);
                    hi = ((xv.x >> 16) & 0xFFu) | (((xv.y >> 16) & 0xFFu) << 8) | ((xv.x >> 24) << 16) |
                         ((xv.y >> 24) << 24);
                }
                const long ax = pack64(lo, hi);
                const f32x4 xdv = *(const f32x4 *)(xd + so + 16 * i);
                f32x4 xsv = {0.f, 0.f, 0.f, 0.f};
                if (FMT == FMT_Q4_1) xsv = *(const f32x4 *)(xs + so + 16 * i);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int u = 2 * a + s;
                    const i32x4 c = __builtin_amdgcn_mfma_i32_16x16x32_i8(ax, bw[u], zero, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        // (wd * xd) * sumi [+ wm * xs], every operation rounded (oracle matmul)
                        float t = mul_rn(mul_rn(wdf[u], xdv[r]), (float)c[r]);
                        if (FMT == FMT_Q4_1) t = add_rn(t, mul_rn(wmf[u], xsv[r]));
                        acc[i][a][r] = add_rn(acc[i][a][r], t);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int n = 32 * grp + 16 * a + f;
        const float bv = bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t o = (size_t)(m0 + 16 * i + 4 * g + r) * N + n;
                float v = bv + acc[i][a][r];
                if (EPI == 1) v = era_table(gelu_tab, v);
                if (EPI == 2) v = v + res[o];
                Y[o] = v;
            }
    }
}

template <int FMT>
void q8_gemm_fmt(const DevWeight &W, const int8_t *xq, const float *xd, const float *xs, int M, const float *bias,
                 int epi, const float *res, float *Y, hipStream_t s, const uint16_t *gelu_tab)
{
    const int nN = (W.N / 32 + 1) / 2, grid = (M / 64) * nN;
    if (epi == 0)
        q8_gemm_kernel<FMT, 0><<<grid, 256, 0, s>>>(W.qs, W.d, W.m, xq, xd, xs, bias, res, Y, M, W.N, W.K, nN, gelu_tab);
    else if (epi == 1)
        q8_gemm_kernel<FMT, 1><<<grid, 256, 0, s>>>(W.qs, W.d, W.m, xq, xd, xs, bias, res, Y, M, W.N, W.K, nN, gelu_tab);
    else
        q8_gemm_kernel<FMT, 2><<<grid, 256, 0, s>>>(W.qs, W.d, W.m, xq, xd, xs, bias, res, Y, M, W.N, W.K, nN, gelu_tab);
}

}  // namespace

int launch_q8_quantize(const float *X, int32_t T, int32_t M, int32_t K, int32_t kind, int8_t *q, float *d, float *s,
                       hipStream_t st)
{
    if (M <= 0 || M % 64 || K <= 0 || K % 32 || T < 0 || T > M || (kind != 0 && kind != 1) || !X || !q || !d ||
        (kind == 1 && !s))
        return -1;
    const size_t n = (size_t)M * (K / 4);
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (kind == 0) q8_quantize_kernel<0><<<grid, 256, 0, st>>>(X, T, M, K, q, d, s);
    else q8_quantize_kernel<1><<<grid, 256, 0, st>>>(X, T, M, K, q, d, s);
    return 0;
}

int launch_q8_gemm(const DevWeight &W, const int8_t *xq, const float *xd, const float *xs, int32_t M,
                   const float *bias, int32_t epi, const float *res, float *Y, hipStream_t s, const uint16_t *gelu_tab)
{
    if ((W.fmt != FMT_Q4_0 && W.fmt != FMT_Q4_1 && W.fmt != FMT_Q8_0) || W.kx || W.K <= 0 || W.K % 64 || W.N <= 0 ||
        W.N % 32 || M <= 0 || M % 64 || epi < 0 || epi > 2 || (epi == 2 && !res) || (epi == 1 && !gelu_tab) ||
        !W.qs || !W.d || (W.fmt == FMT_Q4_1 && (!W.m || !xs)) || !xq || !xd || !bias || !Y)
        return -1;
    if (W.fmt == FMT_Q4_0) q8_gemm_fmt<FMT_Q4_0>(W, xq, xd, xs, M, bias, epi, res, Y, s, gelu_tab);
    else if (W.fmt == FMT_Q4_1) q8_gemm_fmt<FMT_Q4_1>(W, xq, xd, xs, M, bias, epi, res, Y, s, gelu_tab);
    else q8_gemm_fmt<FMT_Q8_0>(W, xq, xd, xs, M, bias, epi, res, Y, s, gelu_tab);
    return 0;
}

}  // namespace emb
