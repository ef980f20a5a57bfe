// The classification head of a cross-encoder (BertForSequenceClassification): the
// sentences' final-LayerNorm [CLS] rows, pooler dense + tanh, classifier.  All f32,
// one form for the f16, f32 and q8-activation chains (kernels.h).  Small next to the
// encoder; what it keeps is the order of every sum, fixed by d alone, so a sentence's
// logits are the same bits alone and inside any batch.
#include "device_common.h"
#include "host_common.h"
#include "kernels.h"

namespace emb {
namespace {

// Stage 0, f16 chain: x[b] = LN(y[row]) = r z - r mean gamma + beta, the expression
// cls_l2_kernel and tokens_f32_kernel use (norm.hip), not normalised.
__global__ __launch_bounds__(256) void head_gather_kernel(const h16 *__restrict__ z, const float2 *__restrict__ stats,
                                                          const float *__restrict__ lw, const float *__restrict__ lb,
                                                          const int32_t *__restrict__ cu, int d, float *__restrict__ x)
{
    const int b = blockIdx.x;
    const int row = cu ? cu[b] : b;
    const float2 st = stats[row];
    const float r = st.y, t0 = -st.x * st.y;
    for (int c = threadIdx.x; c < d; c += 256)
        x[(size_t)b * d + c] = fmaf(r, (float)z[(size_t)row * d + c], fmaf(t0, lw[c], lb[c]));
}

// Stage 0, f32 / q8 chains: row cu[b] of the final LayerNorm output.
__global__ __launch_bounds__(256) void head_gather_f32_kernel(const float *__restrict__ x32,
                                                              const int32_t *__restrict__ cu, int d,
                                                              float *__restrict__ x)
{
    const int b = blockIdx.x;
    const size_t row = (size_t)cu[b];
    for (int c = threadIdx.x; c < d; c += 256) x[(size_t)b * d + c] = x32[row * d + c];
}

// Stage 1: p[m][n] = tanh(bp[n] + sum_k x[m][k] wp[n][k]) for the (16 sentences, 16
// features) tile of a workgroup on v_mfma_f32_16x16x4_f32.  Four waves, wave w the
// quarter [w d/4, (w + 1) d/4) of k in chunks of 16: lane (r = l & 15, g = l >> 4)
// loads the four values k0 + 4g .. 4g + 3 of sentence row r and of feature row r with
// one 16-B load each, and MFMA j of the chunk takes element j of both, so its four k
// slots hold k0 + 4g + j.  An output element is therefore one chain of d/64 chunks x
// 4 MFMAs per wave, in that order, and the four waves' sums meet as (w0 + w1) + (w2 +
// w3): nothing in the order depends on the tile's position or on n.  Sentence rows
// m >= n enter as zeros and are not stored.  D: lane l holds feature l & 15 of
// sentences 4 (l >> 4) + r (f32.hip's layout).
__global__ __launch_bounds__(256) void head_pooler_kernel(const float *__restrict__ x, int n, int d,
                                                          const float *__restrict__ wp, const float *__restrict__ bp,
                                                          float *__restrict__ p)
{
    __shared__ f32x4 part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    const int r = lane & 15, g = lane >> 4;
    const int kq = d / 4, k_lo = w * kq;
    const bool xrow = m0 + r < n;
    const float *xp = x + (size_t)(xrow ? m0 + r : 0) * d + k_lo + 4 * g;
    const float *wr = wp + (size_t)(n0 + r) * d + k_lo + 4 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kq; k0 += 16) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (xrow) a = *(const f32x4 *)(xp + k0);
        const f32x4 b = *(const f32x4 *)(wr + k0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w != 0) return;
    const f32x4 s01 = part[0][lane] + part[1][lane], s23 = part[2][lane] + part[3][lane];
    const f32x4 sum = s01 + s23;
    const float bv = bp[n0 + r];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int m = m0 + 4 * g + e;
        if (m < n) p[(size_t)m * d + n0 + r] = tanhf(bv + sum[e]);
    }
}

// Stage 2: logit[b][c] = bc[c] + wc[c] . p[b], one wave per sentence: lane l sums its
// columns l, l + 64, ... in ascending order (one FMA chain), then the xor-shuffle tree
// of wave_sum -- the same tree for every (sentence, label).
__global__ __launch_bounds__(64) void head_classifier_kernel(const float *__restrict__ p, int d,
                                                             const float *__restrict__ wc,
                                                             const float *__restrict__ bc, int n_labels,
                                                             float *__restrict__ logits)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *pr = p + (size_t)b * d;
    for (int c = 0; c < n_labels; ++c) {
        const float *wr = wc + (size_t)c * d;
        float a = 0.f;
        for (int k = lane; k < d; k += 64) a = fmaf(wr[k], pr[k], a);
        a = wave_sum(a);
        if (lane == 0) logits[(size_t)b * n_labels + c] = bc[c] + a;
    }
}

}  // namespace

void launch_head_gather(const uint16_t *z, const float2 *stats, const float *ln_w, const float *ln_b, const int32_t *cu,
                        int32_t n_seqs, int32_t d, float *x, hipStream_t s)
{
    head_gather_kernel<<<n_seqs, 256, 0, s>>>((const h16 *)z, stats, ln_w, ln_b, cu, d, x);
}

void launch_head_gather_f32(const float *x32, const int32_t *cu, int32_t n_seqs, int32_t d, float *x, hipStream_t s)
{
    head_gather_f32_kernel<<<n_seqs, 256, 0, s>>>(x32, cu, d, x);
}

int launch_head(const float *x, int32_t n_seqs, int32_t d, const float *wp, const float *bp, const float *wc,
                const float *bc, int32_t n_labels, float *p, float *logits, hipStream_t s)
{
    if (n_seqs <= 0 || d <= 0 || d % 64 || d > 1024 || n_labels < 1 || n_labels > HEAD_MAX_LABELS) return -1;
    head_pooler_kernel<<<dim3(d / 16, (n_seqs + 15) / 16), 256, 0, s>>>(x, n_seqs, d, wp, bp, p);
    head_classifier_kernel<<<n_seqs, 64, 0, s>>>(p, d, wc, bc, n_labels, logits);
    return 0;
}

}  // namespace emb
