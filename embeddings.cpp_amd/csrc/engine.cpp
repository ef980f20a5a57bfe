// Per-GPU engine: the model's device image (built once on the host from the repack.h
// layouts), the replica that uploads it, its workspace, live per-kernel timing and
// graph cache.  The forward itself is forward.cpp; see kernels.h for the HBM layouts.
#include "engine.h"
#include "hip_check.h"
#include "repack.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

namespace emb {

const char *kclass_name(int k)
{
    static const char *names[K_NUM_CLASSES] = {"embed_ln", "gemm_qkv", "attention", "gemm_attn_out",
                                               "ln_stats", "gemm_ffn_up", "gemm_ffn_down", "pool_l2"};
    return (k >= 0 && k < K_NUM_CLASSES) ? names[k] : "?";
}

int hip_device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

ModelImage::~ModelImage()
{
    if (pinned_) (void)hipHostFree(pinned_);
}

void build_proj_image(const float *W, int dim, int d, std::vector<uint8_t> &bytes)
{
    const int width = proj_width_of(dim), NT = width / 16;
    bytes.assign((size_t)width * d * 2, 0);   // (f16 +0: the padding rows)
    uint16_t *o = (uint16_t *)bytes.data();
    for (int j = 0; j < dim; ++j)
        for (int k = 0; k < d; ++k) {
            const int kb = k / 32, g = (k % 32) / 8, e = k % 8, t = j / 16, f = j % 16;
            o[(((size_t)kb * NT + t) * 64 + 16 * g + f) * 8 + e] = f32_to_f16(W[(size_t)j * d + k]);
        }
}

bool build_model_image(const HostModel &m, ModelImage &img, std::string &err, bool pin, int act_mode)
{
    try {
        const HParams &hp = m.hp;
        const int d = hp.n_embd, f = hp.n_intermediate;
        if (hp.n_head <= 0 || d % 64 || d > 1024 || f % 64 || (d / hp.n_head != 32 && d / hp.n_head != 64)) {
            char buf[256];
            std::snprintf(buf, sizeof buf,
                          "unsupported shape n_embd=%d n_intermediate=%d n_head=%d (need n_embd %% 64 == 0, "
                          "n_embd <= 1024, head_dim 32 or 64)", d, f, hp.n_head);
            err = buf;
            return false;
        }
        if (fault_inject("image")) throw std::bad_alloc();
        img.hp = hp;
        img.wfmt = hp.ftype;
        // f32 files run the f32 chain (f32.hip) on the file's own f32 rows; the other
        // formats the lane-order layout of the MFMA f16 GEMMs
        img.f32 = img.wfmt == FMT_F32;
        // activation mode 1 (quantized files): the same lane-order weights under the
        // q8-activation chain (q8act.hip)
        img.q8 = act_mode_effective(img.wfmt, act_mode) == 1;
        std::vector<Piece> pieces;
        pieces.reserve(16 + 24 * (size_t)hp.n_layer);
        auto add = [&](Piece &&p) -> size_t { pieces.push_back(std::move(p)); return pieces.size() - 1; };
        auto vec = [&](const HostTensor &t) -> size_t { Piece p; p.bytes = t.bytes; return add(std::move(p)); };
        auto table = [&](const HostTensor &t) -> ModelImage::Tab {
            Piece q, dd, mm;
            repack_table(t, q, dd, mm);
            ModelImage::Tab r;
            r.fmt = t.fmt; r.rows = t.ne1; r.cols = t.ne0;
            r.q = add(std::move(q)); r.d = add(std::move(dd)); r.m = add(std::move(mm));
            return r;
        };
        auto linear = [&](std::vector<const HostTensor *> parts) -> ModelImage::Lin {
            Piece q, dd, mm;
            ModelImage::Lin r;
            repack_linear(parts, img.wfmt, q, dd, mm, r.N, r.K);
            r.q = add(std::move(q)); r.d = add(std::move(dd)); r.m = add(std::move(mm));
            return r;
        };
        img.word = table(m.word);
        img.type = table(m.ttype);
        img.pos = table(m.pos);
        // f32 and q8 chains: the era's fp16 GELU and exp tables, built on the host (libm)
        // as ggml built them, indexed on the device by the f16 bits of the input
        if (img.f32 || img.q8) {
            std::vector<uint16_t> tg, te;
            era_tables(tg, te);
            Piece pg, pe;
            pg.bytes.assign((const uint8_t *)tg.data(), (const uint8_t *)(tg.data() + tg.size()));
            pe.bytes.assign((const uint8_t *)te.data(), (const uint8_t *)(te.data() + te.size()));
            img.gelu = add(std::move(pg));
            img.exp = add(std::move(pe));
        }
        img.lnw = vec(m.ln_e_w);
        img.lnb = vec(m.ln_e_b);
        auto fold = [&](std::vector<const HostTensor *> parts, std::vector<const HostTensor *> bias,
                        const HostTensor &gamma, const HostTensor &beta, size_t &i1, size_t &i2) {
            Piece c1, c2;
            fold_ln(parts, bias, gamma, beta, c1, c2, img.wfmt == FMT_F32);
            i1 = add(std::move(c1));
            i2 = add(std::move(c2));
        };
        // f32 chain: the rows of the parts as f32 (concatenated along N)
        auto rows32 = [&](std::vector<const HostTensor *> parts) -> size_t {
            Piece p;
            for (const HostTensor *t : parts) {
                const size_t n0 = p.bytes.size();
                p.bytes.resize(n0 + (size_t)t->ne1 * t->ne0 * 4);
                for (int r = 0; r < t->ne1; ++r)
                    dequant_row(t->fmt, t->bytes.data() + fmt_row_bytes(t->fmt, t->ne0) * r,
                                (float *)(p.bytes.data() + n0) + (size_t)r * t->ne0, t->ne0);
            }
            return add(std::move(p));
        };
        // the head, one f32 form for every chain: the pooler rows dequantized once
        if (m.n_labels > 0) {
            img.n_labels = m.n_labels;
            img.head_wp = rows32({&m.pool_w});
            img.head_bp = vec(m.pool_b);
            img.head_wc = vec(m.cls_w);
            img.head_bc = vec(m.cls_b);
        }
        // the projection, one f16 image for every chain: the library's own dequantized rows
        if (m.proj_dim > 0) {
            std::vector<float> w32((size_t)m.proj_dim * d);
            for (int r = 0; r < m.proj_dim; ++r)
                dequant_row(m.proj_w.fmt, m.proj_w.bytes.data() + fmt_row_bytes(m.proj_w.fmt, d) * r,
                            w32.data() + (size_t)r * d, d);
            Piece p;
            build_proj_image(w32.data(), m.proj_dim, d, p.bytes);
            img.proj_dim = m.proj_dim;
            img.proj = add(std::move(p));
        }
        img.layers.assign((size_t)hp.n_layer, ModelImage::Layer());
        for (int l = 0; l < hp.n_layer; ++l) {
            const HostLayer &L = m.layers[(size_t)l];
            ModelImage::Layer &x = img.layers[(size_t)l];
            if (img.f32) {
                x.w32q = rows32({&L.q_w, &L.k_w, &L.v_w}); x.w32o = rows32({&L.o_w});
                x.w32u = rows32({&L.i_w}); x.w32d = rows32({&L.o2_w});
                x.bq = rows32({&L.q_b, &L.k_b, &L.v_b}); x.bu = vec(L.i_b);
                x.bo = vec(L.o_b); x.bdown = vec(L.o2_b);
                x.l1w = vec(L.ln_att_w); x.l1b = vec(L.ln_att_b); x.l2w = vec(L.ln_out_w); x.l2b = vec(L.ln_out_b);
                continue;
            }
            x.qkv = linear({&L.q_w, &L.k_w, &L.v_w});
            x.o = linear({&L.o_w});
            x.up = linear({&L.i_w});
            x.down = linear({&L.o2_w});
            if (img.q8) {
                // LayerNorm is a kernel of its own in this chain: the raw biases, no fold
                x.bq = rows32({&L.q_b, &L.k_b, &L.v_b}); x.bu = vec(L.i_b);
            } else {
                // the LN in front of QKV: the previous layer's output LN, or the embedding LN
                const HostTensor &gq = l ? m.layers[(size_t)l - 1].ln_out_w : m.ln_e_w;
                const HostTensor &bq = l ? m.layers[(size_t)l - 1].ln_out_b : m.ln_e_b;
                fold({&L.q_w, &L.k_w, &L.v_w}, {&L.q_b, &L.k_b, &L.v_b}, gq, bq, x.c1q, x.c2q);
                fold({&L.i_w}, {&L.i_b}, L.ln_att_w, L.ln_att_b, x.c1u, x.c2u);
            }
            x.bo = vec(L.o_b); x.bdown = vec(L.o2_b);
            x.l1w = vec(L.ln_att_w); x.l1b = vec(L.ln_att_b); x.l2w = vec(L.ln_out_w); x.l2b = vec(L.ln_out_b);
        }
        img.off.resize(pieces.size());
        img.len.resize(pieces.size());
        size_t total = 0;
        for (size_t i = 0; i < pieces.size(); ++i) {
            img.off[i] = total;
            img.len[i] = pieces[i].bytes.size();
            total += align_up(pieces[i].bytes.size(), 256);
        }
        img.total = total ? total : 256;
        // one contiguous image, page-locked when possible so each replica's upload is
        // one async copy on its own stream; pieces are freed as they are copied
        uint8_t *dst = nullptr;
        if (pin) {
            if (hipHostMalloc((void **)&img.pinned_, img.total, hipHostMallocPortable) != hipSuccess) {   // every device copies from it
                (void)hipGetLastError();
                img.pinned_ = nullptr;
                trace("build_model_image: page-locking %zu bytes failed, pageable uploads\n", img.total);
            }
        }
        if (img.pinned_) {
            dst = img.pinned_;
        } else {
            img.host_.assign(img.total, 0);
            dst = img.host_.data();
        }
        for (size_t i = 0; i < pieces.size(); ++i) {
            Piece &p = pieces[i];
            if (!p.bytes.empty()) std::memcpy(dst + img.off[i], p.bytes.data(), p.bytes.size());
            const size_t pad = align_up(p.bytes.size(), 256) - p.bytes.size();
            if (pad) std::memset(dst + img.off[i] + p.bytes.size(), 0, pad);
            std::vector<uint8_t>().swap(p.bytes);
        }
        return true;
    } catch (const std::bad_alloc &) {
        err = "out of host memory building the device image";
    } catch (const std::exception &ex) {
        err = std::string("building the device image failed: ") + ex.what();
    }
    return false;
}

// Order: every host allocation first (layers_, the only one that can throw), then
// stream, event and arena, then bind (pointer arithmetic on arena_, cannot throw),
// and the upload last.  An exception therefore leaves the constructor before
// anything is allocated on the device or in flight; after that point failures
// return with ok() false and the destructor releases what was made.
Device::Device(int ordinal, const ModelImage &img) : ordinal_(ordinal), hp_(img.hp)
{
    layers_.assign((size_t)hp_.n_layer, DevLayer());
    DeviceGuard g(ordinal);
    if (!g.ok() || hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&done_ev_, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        errorf("libbert: cannot initialise HIP device %d\n", ordinal);
        return;
    }
    if (hipMalloc((void **)&arena_, img.total) != hipSuccess) {
        (void)hipGetLastError();
        errorf("libbert: hipMalloc of %zu bytes of weights failed on device %d\n", img.total, ordinal_);
        arena_ = nullptr;
        return;
    }
    arena_size_ = img.total;
    bind(img);
    // page-locked image: one async copy on this replica's stream, so the uploads of
    // all replicas overlap although one thread issues them; pageable: a blocking copy
    const hipError_t e = img.pinned()
        ? hipMemcpyAsync(arena_, img.bytes(), img.total, hipMemcpyHostToDevice, stream_)
        : hipMemcpy(arena_, img.bytes(), img.total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        errorf("libbert: weight upload failed on device %d: %s\n", ordinal_, hipGetErrorString(e));
        return;
    }
    uploading_ = true;
}

bool Device::finish_load()
{
    if (!uploading_) return false;
    DeviceGuard g(ordinal_);
    if (!g.ok()) return false;
    const hipError_t e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        errorf("libbert: weight upload failed on device %d: %s\n", ordinal_, hipGetErrorString(e));
        return false;
    }
    uploading_ = false;
    ok_ = true;
    return true;
}

Device::~Device()
{
    DeviceGuard g(ordinal_);
    if (stream_ && uploading_) (void)hipStreamSynchronize(stream_);   // the image may still be in flight
    if (done_ev_ && any_forward_) (void)hipEventSynchronize(done_ev_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    drop_graphs();
    for (auto &p : pending_) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : free_events_) (void)hipEventDestroy(e);
    if (arena_) (void)hipFree(arena_);
    if (ws_) (void)hipFree(ws_);
    if (tok_out_) (void)hipFree(tok_out_);
    if (h_ids_) (void)hipHostFree(h_ids_);
    if (h_cu_) (void)hipHostFree(h_cu_);
    if (h_types_) (void)hipHostFree(h_types_);
    if (h_keys_) (void)hipHostFree(h_keys_);
    if (h_out_) (void)hipHostFree(h_out_);
    if (done_ev_) (void)hipEventDestroy(done_ev_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void Device::order_after_last(hipStream_t s)
{
    if (any_forward_ && last_stream_ != s) (void)hipStreamWaitEvent(s, done_ev_, 0);
}

void Device::mark_done(hipStream_t s)
{
    (void)hipEventRecord(done_ev_, s);
    last_stream_ = s;
    any_forward_ = true;
}

void Device::bind(const ModelImage &img)
{
    wfmt_ = img.wfmt;
    f32_ = img.f32;
    q8_ = img.q8;
    auto P = [&](size_t i) -> void * {
        return (i == ModelImage::kNone || img.len[i] == 0) ? nullptr : (void *)(arena_ + img.off[i]);
    };
    auto mk_table = [&](const ModelImage::Tab &x) {
        DevTable r;
        r.fmt = x.fmt; r.rows = x.rows; r.cols = x.cols;
        r.qs = P(x.q); r.d = (const uint16_t *)P(x.d); r.m = (const uint16_t *)P(x.m);
        return r;
    };
    if (f32_ || q8_) {
        gelu_tab_ = (const uint16_t *)P(img.gelu);
        exp_tab_ = (const uint16_t *)P(img.exp);
    }
    word_ = mk_table(img.word);
    type_ = mk_table(img.type);
    pos_ = mk_table(img.pos);
    ln_e_w_ = (float *)P(img.lnw);
    ln_e_b_ = (float *)P(img.lnb);
    n_labels_ = img.n_labels;
    head_wp_ = (const float *)P(img.head_wp); head_bp_ = (const float *)P(img.head_bp);
    head_wc_ = (const float *)P(img.head_wc); head_bc_ = (const float *)P(img.head_bc);
    proj_dim_ = img.proj_dim;
    proj_w_ = P(img.proj);
    auto mk_lin = [&](const ModelImage::Lin &x) {
        DevWeight w;
        w.fmt = wfmt_ == FMT_F32 ? FMT_F16 : wfmt_; w.N = x.N; w.K = x.K;
        w.kx = wfmt_ == FMT_F32 ? x.K / 2 : 0;
        w.qs = P(x.q); w.d = (const uint16_t *)P(x.d); w.m = (const uint16_t *)P(x.m);
        return w;
    };
    for (int l = 0; l < hp_.n_layer; ++l) {   // (layers_ was sized by the constructor)
        const ModelImage::Layer &x = img.layers[(size_t)l];
        DevLayer &D = layers_[(size_t)l];
        if (f32_) {
            D.w32_qkv = (const float *)P(x.w32q); D.w32_o = (const float *)P(x.w32o);
            D.w32_up = (const float *)P(x.w32u); D.w32_down = (const float *)P(x.w32d);
            D.b_qkv = (const float *)P(x.bq); D.b_up = (const float *)P(x.bu);
            D.b_o = (float *)P(x.bo); D.b_down = (float *)P(x.bdown);
            D.ln1_w = (float *)P(x.l1w); D.ln1_b = (float *)P(x.l1b); D.ln2_w = (float *)P(x.l2w); D.ln2_b = (float *)P(x.l2b);
            continue;
        }
        D.qkv = mk_lin(x.qkv); D.o = mk_lin(x.o); D.up = mk_lin(x.up); D.down = mk_lin(x.down);
        D.b_o = (float *)P(x.bo); D.b_down = (float *)P(x.bdown);
        D.b_qkv = (const float *)P(x.bq); D.b_up = (const float *)P(x.bu);   // (q8 chain; else absent)
        D.c1_qkv = (float *)P(x.c1q); D.c2_qkv = (float *)P(x.c2q); D.c1_up = (float *)P(x.c1u); D.c2_up = (float *)P(x.c2u);
        D.ln1_w = (float *)P(x.l1w); D.ln1_b = (float *)P(x.l1b); D.ln2_w = (float *)P(x.l2w); D.ln2_b = (float *)P(x.l2b);
    }
}

bool Device::reserve(int64_t tokens, int64_t seqs, int max_len)
{
    const int64_t pool_rows = seqs * pool_chunks(std::max(1, std::min(max_len, hp_.n_max_tokens)));
    if (tokens <= cap_tokens_ && seqs <= cap_seqs_ && pool_rows <= cap_pool_) return true;
    DeviceGuard g(ordinal_);
    HIP_OK(g.status());
    if (any_forward_) HIP_OK(hipEventSynchronize(done_ev_));   // the last forward may be on a caller stream
    HIP_OK(hipStreamSynchronize(stream_));
    const int64_t nt = std::max<int64_t>(align_up((size_t)std::max(tokens, cap_tokens_), 4096), 4096);
    const int64_t ns = std::max<int64_t>(align_up((size_t)std::max(seqs, cap_seqs_), 256), 256);
    // pool partials [n_seqs][chunks][d]: sized by the sentences' own max_len, not
    // n_max_tokens (a chunk of many short texts would otherwise reserve GBs)
    const int64_t np = std::max<int64_t>(align_up((size_t)std::max(pool_rows, cap_pool_), 256), 256);
    const int64_t rows = nt + GEMM_BM + 256;   // padding rows for tile overrun (kernels read, never trust)
    const int64_t d = hp_.n_embd, f = hp_.n_intermediate;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return o; };
    // f16 chain: Z, QKV, ATT, FFN f16 + statistics; f32 and q8 chains: X, Z, QKV, ATT,
    // FFN f32; q8 chain: the int8 input of a projection, its block scales and sums
    const bool c32 = f32_ || q8_;
    const int64_t r16 = c32 ? 0 : rows, r32 = c32 ? rows : 0, rq = q8_ ? rows : 0, kq = std::max(d, f);
    const size_t o_st = take(r16 * 8), o_z = take(r16 * d * 2), o_part = take(r16 * (d / 32) * 8);
    const size_t o_qkv = take(r16 * 3 * d * 2), o_att = take(r16 * d * 2), o_ffn = take(r16 * f * 2);
    const size_t o_x32 = take(r32 * d * 4), o_z32 = take(r32 * d * 4), o_qkv32 = take(r32 * 3 * d * 4);
    const size_t o_att32 = take(r32 * d * 4), o_ffn32 = take(r32 * f * 4);
    const size_t o_xq = take(rq * kq), o_xd = take(rq * (kq / 32) * 4), o_xs = take(rq * (kq / 32) * 4);
    const size_t o_ids = take(rows * 4), o_cu = take((ns + 1) * 4), o_out = take(ns * d * 4);
    const size_t o_types = take(rows * 4);
    const int64_t rh = n_labels_ > 0 ? ns : 0;   // the head's two row buffers
    const size_t o_hx = take(rh * d * 4), o_hp = take(rh * d * 4);
    const size_t o_pool = take((size_t)np * d * 4);
    // the pruned last layer of CLS pooling (f16 chain): one row per sentence, padded
    // to whole GEMM tiles as the token rows are
    const int64_t rows_c = ns + GEMM_BM + 256, rc16 = c32 ? 0 : rows_c;
    const size_t o_stc = take(rc16 * 8), o_zc = take(rc16 * d * 2), o_partc = take(rc16 * (d / 32) * 8);
    const size_t o_attc = take(rc16 * d * 2), o_ffnc = take(rc16 * f * 2);
    const size_t o_keys = take(ns * 4);   // the sentences' key counts (forward_host with counts)
    drop_graphs();   // captured graphs hold the old workspace pointers
    if (ws_) { (void)hipFree(ws_); ws_ = nullptr; }
    if (h_ids_) { (void)hipHostFree(h_ids_); h_ids_ = nullptr; }
    if (h_cu_) { (void)hipHostFree(h_cu_); h_cu_ = nullptr; }
    if (h_out_) { (void)hipHostFree(h_out_); h_out_ = nullptr; }
    if (h_types_) { (void)hipHostFree(h_types_); h_types_ = nullptr; }
    if (h_keys_) { (void)hipHostFree(h_keys_); h_keys_ = nullptr; }
    cap_tokens_ = cap_seqs_ = cap_pool_ = 0;
    HIP_OK(hipMalloc((void **)&ws_, off));
    // on the replica's own (non-blocking) stream: a null-stream memset would not
    // be ordered before the forward that follows on stream_
    HIP_OK(hipMemsetAsync(ws_, 0, off, stream_));
    HIP_OK(hipStreamSynchronize(stream_));
    st_ = (float2 *)(ws_ + o_st); z_ = (uint16_t *)(ws_ + o_z); part_ = (float2 *)(ws_ + o_part);
    rows_ = rows;
    qkv_ = (uint16_t *)(ws_ + o_qkv); att_ = (uint16_t *)(ws_ + o_att); ffn_ = (uint16_t *)(ws_ + o_ffn);
    d_ids_ = (int32_t *)(ws_ + o_ids); d_cu_ = (int32_t *)(ws_ + o_cu); d_out_ = (float *)(ws_ + o_out);
    pool_part_ = (float *)(ws_ + o_pool);
    d_types_ = (int32_t *)(ws_ + o_types);
    d_keys_ = (int32_t *)(ws_ + o_keys);
    head_x_ = (float *)(ws_ + o_hx); head_p_ = (float *)(ws_ + o_hp);
    stc_ = (float2 *)(ws_ + o_stc); zc_ = (uint16_t *)(ws_ + o_zc); partc_ = (float2 *)(ws_ + o_partc);
    attc_ = (uint16_t *)(ws_ + o_attc); ffnc_ = (uint16_t *)(ws_ + o_ffnc);
    rows_c_ = rows_c;
    x32_ = (float *)(ws_ + o_x32); z32_ = (float *)(ws_ + o_z32); qkv32_ = (float *)(ws_ + o_qkv32);
    att32_ = (float *)(ws_ + o_att32); ffn32_ = (float *)(ws_ + o_ffn32);
    xq_ = (int8_t *)(ws_ + o_xq); xd_ = (float *)(ws_ + o_xd); xs_ = (float *)(ws_ + o_xs);
    HIP_OK(hipHostMalloc((void **)&h_ids_, nt * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc((void **)&h_cu_, (ns + 1) * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc((void **)&h_types_, nt * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc((void **)&h_keys_, ns * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc((void **)&h_out_, ns * d * 4, hipHostMallocDefault));
    cap_tokens_ = nt;
    cap_seqs_ = ns;
    cap_pool_ = np;
    return true;
}

hipEvent_t Device::get_event()
{
    if (!free_events_.empty()) { hipEvent_t e = free_events_.back(); free_events_.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void Device::begin(int cls, hipStream_t s, hipEvent_t &a)
{
    (void)cls;
    a = nullptr;
    if (!profiling_) return;
    a = get_event();
    (void)hipEventRecord(a, s);
}

void Device::end(int cls, hipStream_t s, hipEvent_t a, double work)
{
    if (!profiling_ || !a) return;
    hipEvent_t b = get_event();
    (void)hipEventRecord(b, s);
    pending_.push_back({cls, a, b, work});
}

void Device::collect_stats()
{
    DeviceGuard g(ordinal_);
    for (auto &p : pending_) {
        (void)hipEventSynchronize(p.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            stats_[p.cls].launches += 1;
            stats_[p.cls].ms += ms;
            stats_[p.cls].work += p.work;
        }
        free_events_.push_back(p.a);
        free_events_.push_back(p.b);
    }
    pending_.clear();
}

void Device::reset_stats()
{
    collect_stats();
    for (auto &s : stats_) s = KStats();
}

void Device::drop_graphs()
{
    for (auto &g : graphs_) (void)hipGraphExecDestroy(g.exec);
    graphs_.clear();
    seen_once_.clear();
}

}  // namespace emb
