// Single-query attention for [CLS] pooling (gfx950).
//
// Under CLS pooling only the first row of every sentence leaves the last layer,
// so that layer's attention needs one query per (sentence, head): row cu[b]
// against the sentence's own keys (bert.cpp:1018-1036 for that one row).  One
// query fills no MFMA tile; the kernel is bound by the single read of the
// sentence's K and V:
//   * a workgroup of 256 threads per (head, sentence) walks the keys in chunks
//     of 256: a thread per key for the scores (the key's dh halves as 16-byte
//     loads, the query in registers), then dh/8 column groups x 2048/dh key groups
//     for P V (16-byte loads of V, f32 accumulators per thread);
//   * softmax is the online form over the chunks (running maximum and sum, the
//     accumulators rescaled per chunk), so any length runs with the same LDS;
//   * chunking and every reduction tree depend on the sentence's own length
//     only: a sentence gives the same bits alone, in any batch, at any max_len.
// A sentence's workgroups also gather the residual row of the compact last layer
// (zc[b] = z[cu[b]], each head its own dh columns; stc[b] = st[cu[b]]) and clear
// their share of the padding rows n_seqs <= row < Mc of the compact buffers, so the
// pruned layer costs no extra launch and its GEMMs read only initialised rows.
#include "device_common.h"
#include "kernels.h"

namespace emb {

namespace {

constexpr int CLS_THREADS = 256;

template <int DH>
__global__ __launch_bounds__(CLS_THREADS) void attention_cls_kernel(
    const h16 *__restrict__ qkv, const int32_t *__restrict__ cu, int n_seqs, int d, int Mc, float scale,
    h16 *__restrict__ attc, const h16 *__restrict__ z, const float2 *__restrict__ st, h16 *__restrict__ zc,
    float2 *__restrict__ stc)
{
    constexpr int NV = DH / 8;                 // 16-byte pieces of a head row
    constexpr int KG = CLS_THREADS / NV;       // key groups of the P V stage
    __shared__ float p_s[CLS_THREADS];
    __shared__ float red_s[8];
    __shared__ float acc_s[KG][DH + 1];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int start = cu[b], len = cu[b + 1] - start;
    const size_t ld = (size_t)3 * d;
    const int cg = tid % NV, kg = tid / NV;

    // the query, kept as f16 pieces
    h16x8 q[NV];
    if (len > 0) {
        const h16 *qp = qkv + (size_t)start * ld + h * DH;
#pragma unroll
        for (int j = 0; j < NV; ++j) q[j] = *(const h16x8 *)(qp + 8 * j);
    }
    const h16 *kbase = qkv + (size_t)start * ld + d + h * DH;
    const h16 *vbase = qkv + (size_t)start * ld + 2 * d + h * DH + 8 * cg;

    float m_run = -INFINITY, l_run = 0.f;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < len; c0 += CLS_THREADS) {
        // scores: a key per thread
        const int i = c0 + tid;
        float sc = -INFINITY;
        if (i < len) {
            const h16 *kp = kbase + (size_t)i * ld;
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const h16x8 kv = *(const h16x8 *)(kp + 8 * j);
#pragma unroll
                for (int e = 0; e < 8; ++e) a = fmaf((float)q[j][e], (float)kv[e], a);
            }
            sc = a * scale;
        }
        // chunk maximum over the workgroup
        float mx = sc;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        if (lane == 0) red_s[w] = mx;
        __syncthreads();
        const float m_new = fmaxf(m_run, fmaxf(fmaxf(red_s[0], red_s[1]), fmaxf(red_s[2], red_s[3])));
        const float p = i < len ? __expf(sc - m_new) : 0.f;
        p_s[tid] = p;
        const float ps = wave_sum(p);
        if (lane == 0) red_s[4 + w] = ps;
        __syncthreads();
        const float corr = __expf(m_run - m_new);   // first chunk: exp(-inf) = 0 on zeros
        l_run = l_run * corr + ((red_s[4] + red_s[5]) + (red_s[6] + red_s[7]));
        m_run = m_new;
        // P V: column group cg (8 columns), keys kg, kg + KG, ... of the chunk
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= corr;
        const int n_c = min(CLS_THREADS, len - c0);
#pragma unroll 4
        for (int k = kg; k < n_c; k += KG) {
            const h16x8 vv = *(const h16x8 *)(vbase + (size_t)(c0 + k) * ld);
            const float pk = p_s[k];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, (float)vv[e], acc[e]);
        }
        __syncthreads();   // p_s / red_s are rewritten by the next chunk
    }
    // the key groups' partial rows, summed in group order
#pragma unroll
    for (int e = 0; e < 8; ++e) acc_s[kg][8 * cg + e] = acc[e];
    __syncthreads();
    float o = 0.f;
    if (tid < DH) {
        // (key groups past the sentence's length hold exact zeros)
        const int ng = min(KG, len);
        for (int g = 0; g < ng; ++g) o += acc_s[g][tid];
        o = len > 0 ? o / l_run : 0.f;
    }
    __syncthreads();   // every LDS read is complete before the first store
    if (tid < DH) attc[(size_t)b * d + h * DH + tid] = (h16)o;

    // The workgroup's share of the compact buffers' other rows and columns: the DH
    // columns of head h (d = n_head DH, so the heads cover a row), of the padding
    // rows n_seqs + b, n_seqs + b + n_seqs, ... < Mc.  Zeros there, and with z the
    // residual gather zc[b] = z[cu[b]], stc[b] = st[cu[b]] in columns of this head.
    const h16x8 zero = {(h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f, (h16)0.f};
    const int first = n_seqs + b;
    const int nr = first < Mc ? (Mc - first + n_seqs - 1) / n_seqs : 0;
    const bool gather = z != nullptr;
    for (int i = tid; i < nr * NV; i += CLS_THREADS) {
        const size_t off = (size_t)(first + (i / NV) * n_seqs) * d + h * DH + 8 * (i % NV);
        *(h16x8 *)(attc + off) = zero;
        if (gather) *(h16x8 *)(zc + off) = zero;
    }
    if (gather) {
        if (tid < NV)
            *(h16x8 *)(zc + (size_t)b * d + h * DH + 8 * tid) = *(const h16x8 *)(z + (size_t)start * d + h * DH + 8 * tid);
        if (h == 0) {
            if (tid == 0) stc[b] = st[start];
            for (int i = tid; i < nr; i += CLS_THREADS) stc[first + i * n_seqs] = float2{0.f, 0.f};
        }
    }
}

}  // namespace

int launch_attention_cls(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs, int32_t n_head, int32_t d, int32_t Mc,
                         uint16_t *attc, const uint16_t *z, const float2 *st, uint16_t *zc, float2 *stc, hipStream_t s)
{
    if (n_seqs <= 0 || n_head <= 0 || d % n_head || d % 8 || Mc < n_seqs) return -1;
    const int dh = d / n_head;
    const float scale = 1.0f / sqrtf((float)dh);
    const dim3 grid(n_head, n_seqs);
    if (dh == 64)
        attention_cls_kernel<64><<<grid, CLS_THREADS, 0, s>>>((const h16 *)qkv, cu, n_seqs, d, Mc, scale, (h16 *)attc,
                                                              (const h16 *)z, st, (h16 *)zc, stc);
    else if (dh == 32)
        attention_cls_kernel<32><<<grid, CLS_THREADS, 0, s>>>((const h16 *)qkv, cu, n_seqs, d, Mc, scale, (h16 *)attc,
                                                              (const h16 *)z, st, (h16 *)zc, stc);
    else
        return -1;
    return 0;
}

}  // namespace emb
