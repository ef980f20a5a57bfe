// Host-only weight layout code (repack.h): file-format tensors -> the device
// layouts described at the top of kernels.h.
#include "repack.h"

namespace emb {

// f32 weights (ftype 0 files, bert.cpp:499-503): each row w becomes the f16 pair
// hi = f16(w), lo = f16(w - hi) laid out as ONE f16 row of 2K, [hi | lo]; the GEMM
// reads X twice along that K (DevWeight::kx), so acc = X W_hi^T + X W_lo^T in f32
// with the weights good to ~2^-22 instead of f16's 2^-11.
void repack_linear_f32(const std::vector<const HostTensor *> &parts, Piece &qs, Piece &dpl, Piece &mpl, int &N_out,
                       int &K_out)
{
    const int K = parts[0]->ne0;
    std::vector<HostTensor> hl(parts.size());
    std::vector<const HostTensor *> hp;
    for (size_t i = 0; i < parts.size(); ++i) {
        const HostTensor &t = *parts[i];
        HostTensor &o = hl[i];
        o.fmt = FMT_F16; o.ne0 = 2 * K; o.ne1 = t.ne1;
        o.bytes.assign((size_t)t.ne1 * 2 * K * 2, 0);
        std::vector<float> row((size_t)K);
        for (int r = 0; r < t.ne1; ++r) {
            dequant_row(t.fmt, t.bytes.data() + fmt_row_bytes(t.fmt, K) * r, row.data(), K);
            uint16_t *dst = (uint16_t *)o.bytes.data() + (size_t)r * 2 * K;
            for (int k = 0; k < K; ++k) {
                const uint16_t h = f32_to_f16(row[(size_t)k]);
                dst[k] = h;
                dst[K + k] = f32_to_f16(row[(size_t)k] - f16_to_f32(h));
            }
        }
        hp.push_back(&o);
    }
    repack_linear(hp, FMT_F16, qs, dpl, mpl, N_out, K_out);
}

// Linear weight [N][K] (file rows) -> the lane-order device layout (kernels.h).
void repack_linear(const std::vector<const HostTensor *> &parts, int fmt_dev, Piece &qs, Piece &dpl, Piece &mpl,
                   int &N_out, int &K_out)
{
    if (fmt_dev == FMT_F32) {
        repack_linear_f32(parts, qs, dpl, mpl, N_out, K_out);
        return;
    }
    const int K = parts[0]->ne0;
    int N = 0;
    for (const HostTensor *t : parts) N += t->ne1;
    N_out = N;
    K_out = K;
    const size_t G = (size_t)N / 32;
    const size_t QB = fmt_dev == FMT_F16 ? 64 : fmt_dev == FMT_Q8_0 ? 32 : 16;
    qs.bytes.assign((size_t)(K / 64) * G * 64 * QB, 0);
    if (fmt_dev != FMT_F16) dpl.bytes.assign((size_t)N * (K / 32) * 2, 0);
    if (fmt_dev == FMT_Q4_1) mpl.bytes.assign((size_t)N * (K / 32) * 2, 0);
    uint16_t *dd = (uint16_t *)dpl.bytes.data();
    uint16_t *mm = fmt_dev == FMT_Q4_1 ? (uint16_t *)mpl.bytes.data() : nullptr;
    static const int pos4[4] = {0, 2, 1, 3};
    int n = 0;
    for (const HostTensor *t : parts) {
        const size_t rb = fmt_row_bytes(t->fmt, K), bb = fmt_block_bytes(t->fmt);
        for (int r = 0; r < t->ne1; ++r, ++n) {
            const uint8_t *src = t->bytes.data() + rb * r;
            const size_t grp = (size_t)n / 32;
            const int a = (n % 32) / 16, f = n % 16;
            for (int blk = 0; blk < K / 32; ++blk) {
                const size_t ks = (size_t)blk / 2;
                const int u = 2 * a + (blk & 1);
                const size_t rec0 = (ks * G + grp) * 64;            // lane-record index of lane 0
                const size_t di = ((ks * G + grp) * 16 + f) * 4 + u;
                for (int e = 0; e < 32; ++e) {
                    const int g = e / 8, i = e % 8;
                    uint8_t *o = qs.bytes.data() + (rec0 + 16 * g + f) * QB;
                    const int k = 32 * blk + e;
                    if (fmt_dev == FMT_F16) {
                        uint16_t h;
                        if (t->fmt == FMT_F16) std::memcpy(&h, src + 2 * k, 2);
                        else { float v; std::memcpy(&v, src + 4 * k, 4); h = f32_to_f16(v); }
                        std::memcpy(o + 16 * u + 2 * i, &h, 2);
                    } else if (fmt_dev == FMT_Q8_0) {
                        const int8_t q = (int8_t)src[bb * blk + 2 + e];
                        o[8 * u + 4 * (i / 4) + pos4[i % 4]] = (uint8_t)((uint8_t)q ^ 0x80u);
                    } else {
                        const uint8_t *nib = src + bb * blk + (fmt_dev == FMT_Q4_1 ? 4 : 2);
                        const uint32_t q = e < 16 ? (nib[e] & 15u) : (uint32_t)(nib[e - 16] >> 4);
                        uint32_t w;
                        std::memcpy(&w, o + 4 * u, 4);
                        w |= q << (4 * (i / 2) + 16 * (i % 2));
                        std::memcpy(o + 4 * u, &w, 4);
                    }
                }
                if (fmt_dev != FMT_F16) std::memcpy(&dd[di], src + bb * blk, 2);
                if (mm) std::memcpy(&mm[di], src + bb * blk + 2, 2);
            }
        }
    }
}

// LN fold constants (kernels.h) of a projection W (the concatenated parts) that
// reads LN(y) = gamma (y - mean) r + beta: c1[n] = sum_k W[n][k] gamma[k],
// c2[n] = b[n] + sum_k W[n][k] beta[k], with W as the GEMM multiplies it (each
// weight rounded once to f16 after dequantization, or the f32 value itself for
// the hi/lo pairs of f32 files), summed in double.
void fold_ln(const std::vector<const HostTensor *> &parts, const std::vector<const HostTensor *> &bias,
             const HostTensor &gamma, const HostTensor &beta, Piece &c1, Piece &c2, bool exact)
{
    const int K = parts[0]->ne0;
    const float *gm = (const float *)gamma.bytes.data(), *bt = (const float *)beta.bytes.data();
    std::vector<float> row((size_t)K), o1, o2;
    for (const HostTensor *t : parts) {
        const size_t rb = fmt_row_bytes(t->fmt, K);
        for (int r = 0; r < t->ne1; ++r) {
            dequant_row(t->fmt, t->bytes.data() + rb * r, row.data(), K);
            double s1 = 0.0, s2 = 0.0;
            for (int k = 0; k < K; ++k) {
                // the weight as the GEMM multiplies it: f16-rounded, or hi + lo (f32 files)
                const double w = exact ? (double)row[(size_t)k] : (double)f16_to_f32(f32_to_f16(row[(size_t)k]));
                s1 += w * gm[k];
                s2 += w * bt[k];
            }
            o1.push_back((float)s1);
            o2.push_back((float)s2);
        }
    }
    size_t n = 0;
    for (const HostTensor *b : bias) {
        const float *bv = (const float *)b->bytes.data();
        for (int i = 0; i < b->ne0; ++i, ++n) o2[n] = (float)((double)o2[n] + (double)bv[i]);
    }
    c1.bytes.assign((const uint8_t *)o1.data(), (const uint8_t *)(o1.data() + o1.size()));
    c2.bytes.assign((const uint8_t *)o2.data(), (const uint8_t *)(o2.data() + o2.size()));
}

// Embedding table in its file format -> aligned planes.
void repack_table(const HostTensor &t, Piece &qs, Piece &dpl, Piece &mpl)
{
    const int rows = t.ne1, cols = t.ne0;
    if (t.fmt == FMT_F32 || t.fmt == FMT_F16) {
        qs.bytes = t.bytes;
        return;
    }
    const size_t nblk = (size_t)rows * (cols / 32), bb = fmt_block_bytes(t.fmt);
    const size_t qb = t.fmt == FMT_Q8_0 ? 32 : 16;
    qs.bytes.assign(nblk * qb, 0);
    dpl.bytes.assign(nblk * 2, 0);
    if (t.fmt == FMT_Q4_1) mpl.bytes.assign(nblk * 2, 0);
    for (size_t i = 0; i < nblk; ++i) {
        const uint8_t *blk = t.bytes.data() + i * bb;
        std::memcpy(dpl.bytes.data() + 2 * i, blk, 2);
        if (t.fmt == FMT_Q4_1) {
            std::memcpy(mpl.bytes.data() + 2 * i, blk + 2, 2);
            std::memcpy(qs.bytes.data() + 16 * i, blk + 4, 16);
        } else {
            std::memcpy(qs.bytes.data() + qb * i, blk + 2, qb);
        }
    }
}

}  // namespace emb
