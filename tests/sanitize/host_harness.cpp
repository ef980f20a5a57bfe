// ASan/UBSan harness of libbert's host code (test infrastructure): the tokenizer
// (tokenizer.cpp), the model-file loader and quantizer (model_file.cpp), the
// converter (converter.cpp) and the weight layout code (repack.cpp), built with -fsanitize=address,undefined by
// tests/sanitize/Makefile and driven by tests/test_cpu_sanitize.py.
//   tok <vocab.bin> <texts.bin> <ids.bin>   vocab: u32 n, (u32 len, bytes)*n;
//                                          texts: u32 n, (i32 n_max, u32 len, bytes)*n;
//                                          ids: per text i32 count, then min(count, n_max) i32
//   load <model.bin>                       parse a model file, print hparams and tensor count
//   quant <in.bin> <out.bin> <itype>       the native quantizer
//   convert <hf_dir> <out.bin> <ftype>     the native converter
//   repack <model.bin> <dump.bin>          the weight layout code (repack.cpp); dump: cmd_repack
#include "host_common.h"
#include "repack.h"
#include "tokenizer.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace emb;

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

static int cmd_tok(const char *vf, const char *tf, const char *of)
{
    FILE *v = std::fopen(vf, "rb"), *t = std::fopen(tf, "rb"), *o = std::fopen(of, "wb");
    if (!v || !t || !o) return 2;
    uint32_t n = 0, len = 0;
    std::vector<std::string> vocab;
    if (!rd(v, &n, 4)) return 3;
    for (uint32_t i = 0; i < n; ++i) {
        if (!rd(v, &len, 4)) return 3;
        std::string s(len, '\0');
        if (!rd(v, &s[0], len)) return 3;
        vocab.push_back(s);
    }
    Vocab voc;
    voc.build(vocab);
    for (uint32_t i = 0; i < n; ++i)
        if (!voc.id_to_token((int32_t)i)) return 4;
    if (!rd(t, &n, 4)) return 3;
    for (uint32_t i = 0; i < n; ++i) {
        int32_t nmax = 0;
        if (!rd(t, &nmax, 4) || !rd(t, &len, 4)) return 3;
        // an exact-size heap buffer, so a read past the terminator is a reported error
        std::vector<char> text(len + 1);
        if (!rd(t, text.data(), len)) return 3;
        text[len] = 0;
        std::vector<int32_t> ids((size_t)(nmax > 0 ? nmax : 0));
        const int32_t cnt = voc.tokenize(text.data(), nmax, ids.data(), nmax > 0 ? nmax : 0);
        std::fwrite(&cnt, 4, 1, o);
        const int32_t w = cnt < nmax ? cnt : nmax;
        if (w > 0) std::fwrite(ids.data(), 4, (size_t)w, o);
    }
    std::fclose(v);
    std::fclose(t);
    std::fclose(o);
    return 0;
}

// repack: every layout function of repack.cpp over a model file, as build_model_image
// calls them (f32 files through the hi/lo path), then the dump of one linear weight
// with its LN fold: layer 0's fused QKV when it spans two 32-feature groups and two
// K-steps (3 n_embd >= 64, n_embd >= 128), else a synthetic [64][128] weight from a
// fixed LCG, in the file's format, as two parts of 32 rows.
static int cmd_repack(const char *mf, const char *of)
{
    HostModel m;
    std::string err;
    if (!load_model_file(mf, m, err, false)) {
        std::fprintf(stderr, "load failed: %s\n", err.c_str());
        return 5;
    }
    const int wfmt = m.hp.ftype;
    for (const HostTensor *t : {&m.word, &m.ttype, &m.pos}) {
        Piece q, d, mm;
        repack_table(*t, q, d, mm);
        if (q.bytes.empty()) return 6;
    }
    using Parts = std::vector<const HostTensor *>;
    for (size_t l = 0; l < m.layers.size(); ++l) {
        const HostLayer &L = m.layers[l];
        for (const Parts &parts : {Parts{&L.q_w, &L.k_w, &L.v_w}, Parts{&L.o_w}, Parts{&L.i_w}, Parts{&L.o2_w}}) {
            Piece q, d, mm;
            int N = 0, K = 0;
            repack_linear(parts, wfmt, q, d, mm, N, K);
            if (q.bytes.empty() || N <= 0 || K <= 0) return 6;
        }
        Piece c1, c2;
        const HostTensor &gq = l ? m.layers[l - 1].ln_out_w : m.ln_e_w, &bq = l ? m.layers[l - 1].ln_out_b : m.ln_e_b;
        fold_ln({&L.q_w, &L.k_w, &L.v_w}, {&L.q_b, &L.k_b, &L.v_b}, gq, bq, c1, c2, wfmt == FMT_F32);
        fold_ln({&L.i_w}, {&L.i_b}, L.ln_att_w, L.ln_att_b, c1, c2, wfmt == FMT_F32);
    }
    // the weight to dump: parts, bias parts, gamma, beta
    HostTensor sw[2], sb[2], sg, sbt;
    Parts parts, bias;
    const HostTensor *gamma = &m.ln_e_w, *beta = &m.ln_e_b;
    if (!m.layers.empty() && 3 * m.hp.n_embd >= 64 && m.hp.n_embd >= 128) {
        const HostLayer &L = m.layers[0];
        parts = {&L.q_w, &L.k_w, &L.v_w};
        bias = {&L.q_b, &L.k_b, &L.v_b};
    } else {
        const int N = 64, K = 128;
        uint32_t st = 2463534242u;
        auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) / 16777216.0f - 0.5f) * 0.25f; };
        auto vec = [&](HostTensor &t, int n, float off) {
            t.fmt = FMT_F32; t.ne0 = n; t.ne1 = 1;
            std::vector<float> v((size_t)n);
            for (float &x : v) x = off + rnd();
            t.bytes.assign((const uint8_t *)v.data(), (const uint8_t *)(v.data() + n));
        };
        std::vector<float> row((size_t)K);
        for (int p = 0; p < 2; ++p) {
            sw[p].fmt = wfmt; sw[p].ne0 = K; sw[p].ne1 = N / 2;
            sw[p].bytes.assign(fmt_row_bytes(wfmt, K) * (size_t)(N / 2), 0);
            for (int r = 0; r < N / 2; ++r) {
                for (float &x : row) x = rnd();
                quantize_row(wfmt, row.data(), sw[p].bytes.data() + fmt_row_bytes(wfmt, K) * (size_t)r, K);
            }
            vec(sb[p], N / 2, 0.0f);
            parts.push_back(&sw[p]);
            bias.push_back(&sb[p]);
        }
        vec(sg, K, 1.0f);
        vec(sbt, K, 0.0f);
        gamma = &sg;
        beta = &sbt;
    }
    Piece q, d, mm, c1, c2;
    int N = 0, K = 0;
    repack_linear(parts, wfmt, q, d, mm, N, K);
    fold_ln(parts, bias, *gamma, *beta, c1, c2, wfmt == FMT_F32);
    // dump: i32 {format, N, K of the file rows, bytes of qs, d, m, c1, c2}, then the file
    // rows, gamma [K], beta [K], bias [N] (f32) and the five planes
    FILE *o = std::fopen(of, "wb");
    if (!o) return 2;
    const int32_t hdr[8] = {wfmt, N, parts[0]->ne0, (int32_t)q.bytes.size(), (int32_t)d.bytes.size(),
                            (int32_t)mm.bytes.size(), (int32_t)c1.bytes.size(), (int32_t)c2.bytes.size()};
    std::fwrite(hdr, 4, 8, o);
    auto put = [&](const std::vector<uint8_t> &b) { if (!b.empty()) std::fwrite(b.data(), 1, b.size(), o); };
    for (const HostTensor *t : parts) put(t->bytes);
    put(gamma->bytes);
    put(beta->bytes);
    for (const HostTensor *t : bias) put(t->bytes);
    for (const Piece *p : {&q, &d, &mm, &c1, &c2}) put(p->bytes);
    std::fclose(o);
    std::printf("%d %d %d\n", wfmt, N, K);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    const std::string c = argv[1];
    if (c == "repack" && argc == 4) return cmd_repack(argv[2], argv[3]);
    if (c == "tok" && argc == 5) return cmd_tok(argv[2], argv[3], argv[4]);
    if (c == "load") {
        HostModel m;
        std::string err;
        if (!load_model_file(argv[2], m, err, false)) {
            std::fprintf(stderr, "load failed: %s\n", err.c_str());
            return 5;
        }
        std::vector<float> row;
        for (const HostLayer &L : m.layers) {   // every weight row dequantizes
            row.resize((size_t)L.i_w.ne0);
            for (int r = 0; r < L.i_w.ne1; ++r)
                dequant_row(L.i_w.fmt, L.i_w.bytes.data() + fmt_row_bytes(L.i_w.fmt, L.i_w.ne0) * r, row.data(),
                            L.i_w.ne0);
        }
        std::printf("%d %d %d %d %d %d %d %d\n", m.hp.n_vocab, m.hp.n_max_tokens, m.hp.n_embd, m.hp.n_intermediate,
                    m.hp.n_head, m.hp.n_layer, m.hp.ftype, m.n_tensors);
        return 0;
    }
    if (c == "quant" && argc == 5) return quantize_file(argv[2], argv[3], std::atoi(argv[4]), false);
    if (c == "convert" && argc == 5) return convert_hf_dir(argv[2], argv[3], std::atoi(argv[4]));
    return 1;
}
