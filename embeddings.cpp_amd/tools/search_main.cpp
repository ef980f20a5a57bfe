// search: the reference's sample client (examples/sample_dylib.py:84-94: embed a
// corpus, then print the k closest texts of every query) with the corpus resident on
// the GPU and the search fused there (bertx_index_*).
//
// usage: search -m MODEL -f CORPUS.txt [-k 3] [-t threads] [-s f16|int8|binary [-R f16|int8 [-B N]]]
//               [-r RERANK_MODEL [-c N] | -l [-c N | -a [-C N [-c N]]] | -L COLBERT_MODEL [-M] [-c N | -a [-C N [-c N]]]]
//               [-S f16|int8|res2|res4]
// One text per line of CORPUS.txt; queries from stdin, one per line, `q` or EOF ends.
// Per hit one line: rank<TAB>id<TAB>score<TAB>text.
// A stdin line `:del ID [ID ...]` removes those rows from the embedding index
// (bertx_index_remove; with -R from both indexes) and prints `deleted N`, N being the change
// of bertx_index_live; later queries no longer return them.  With -a there is no embedding
// index: the line is answered with a message and ignored.
// A stdin line `:drop ID [ID ...]` removes those documents from the token store (-l or -L,
// with or without -a; bertx_mvindex_remove) and prints `dropped N`, N being the change of
// bertx_mvindex_live: the full scan and the pruned search no longer return them, and as
// second-stage candidates they score -inf and are not printed.  Without a token store the
// line is answered with `no token store: nothing dropped` and ignored.
// -s: how the index stores its rows (bertx_index_create_ex): f16, the default, or int8
// with one scale per row, half the bytes and a less precise first stage, or binary: a row
// as its sign bits, one sixteenth of the bytes, searched by Hamming distance; the printed
// score is then d - 2 hamming, an integer (bert_hip.h "Binary storage").
// -R f16|int8: with -s binary, a second index of that kind is kept beside the binary one
// and every query goes through bertx_index_search_rescored_texts: the binary index picks
// -B candidates (default min(128, 4 K), K .. 128, K being k, or the -c value when a second
// stage follows), the second index scores them and the K best by its scores go on.  -R or
// -B without -s binary, and -B without -R, are usage errors.
// -r: a second stage.  Per query the N best of the index (default 4 k, at most the
// index's 128) are re-scored as (query, text) pairs by the cross-encoder RERANK_MODEL
// (a model file with a classification head, bertx_rerank) and the k best of those are
// printed, ordered by the reranker's first-label logit, which is the printed score.
// -l: late interaction as the second stage, instead of -r.  While indexing, every text's
// per-token vectors go into a token store beside the index (bertx_mvindex_*); per query
// the N best of the index are re-scored by MaxSim and the k best of those are printed,
// ordered by that score (equal scores by ascending id), which is the printed score.
// -L: late interaction from a second model file, as -r takes a second model: a ColBERT
// file (a model file with a linear.weight record).  The store is created at that model's
// bertx_proj_width and filled with bertx_mvindex_add_texts_colbert ([D] marker,
// punctuation rows dropped, doc_maxlen 180 capped at the model's n_max_tokens); the
// candidates are re-scored with bertx_mvindex_score_text_colbert ([Q] marker, [MASK]
// augmentation to query_maxlen 32).
// -M: with -L, no row of a query attends to its [MASK] rows (bertx_set_mask_keys(ctx, 0):
// ColBERT's attend_to_mask_tokens = false, as colbertv2.0 was trained).  -M without -L
// is a usage error.
// -a: with -l or -L, full-scan late interaction: no embedding index is created or
// consulted; every query goes through bertx_mvindex_search_texts (-l) or
// bertx_mvindex_search_texts_colbert (-L), which score every stored document by MaxSim
// on the GPU and keep the k best there.  The printed score is the MaxSim score.  -a
// without -l or -L, or together with -r, or with -c but without -C, is a usage error.
// -C N: with -a, the pruned search: after indexing, N centroids (a multiple of 16) are trained
// on the stored token rows (bertx_mvindex_train_centroids, 8 iterations) and every query goes
// through bertx_mvindex_search_pruned_texts: centroid interaction picks -c candidates (default
// min(128, 4 k), k .. 128), the MaxSim scorer ranks those.  -C without -a is a usage error.
// -S: with -l or -L, how the token store keeps its rows (bertx_mvindex_create_ex): f16,
// the default, or int8 with one f32 per token, half the bytes and a less precise
// similarity.  -s still speaks of the index alone.
// -S res2 | res4: with -a -C N, a residual-coded token store (bert_hip.h "Residual codes"):
// the corpus first fills a temporary f16 store, on which the N centroids and then the
// residual buckets are trained (bertx_mvindex_train_residual_buckets); the residual store
// gets those centroids (read back with bertx_mvindex_centroid) and buckets, the corpus is
// added to it, the f16 store is freed, and the queries go through the pruned search.
// -S res* without -C is a usage error.
#include "bert.h"
#include "bert_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char **argv)
{
    const char *model = nullptr, *corpus = nullptr, *rerank = nullptr, *colbert = nullptr;
    int k = 3, threads = 4, cand = 0, cents = 0, storage = BERTX_INDEX_F16, mv_storage = -1, res_storage = -1;
    int fine_storage = -1, bin_cand = 0;
    bool late = false, all = false, no_mask_keys = false;
    for (int i = 1; i < argc; ++i) {
        const bool has = i + 1 < argc;
        if (!std::strcmp(argv[i], "-m") && has) model = argv[++i];
        else if (!std::strcmp(argv[i], "-f") && has) corpus = argv[++i];
        else if (!std::strcmp(argv[i], "-k") && has) k = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "-t") && has) threads = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "-s") && has && !std::strcmp(argv[i + 1], "f16")) { storage = BERTX_INDEX_F16; ++i; }
        else if (!std::strcmp(argv[i], "-s") && has && !std::strcmp(argv[i + 1], "int8")) { storage = BERTX_INDEX_I8; ++i; }
        else if (!std::strcmp(argv[i], "-s") && has && !std::strcmp(argv[i + 1], "binary")) { storage = BERTX_INDEX_BIN; ++i; }
        else if (!std::strcmp(argv[i], "-R") && has && !std::strcmp(argv[i + 1], "f16")) { fine_storage = BERTX_INDEX_F16; ++i; }
        else if (!std::strcmp(argv[i], "-R") && has && !std::strcmp(argv[i + 1], "int8")) { fine_storage = BERTX_INDEX_I8; ++i; }
        else if (!std::strcmp(argv[i], "-B") && has) { bin_cand = std::atoi(argv[++i]); if (bin_cand < 1) bin_cand = -1; }
        else if (!std::strcmp(argv[i], "-S") && has && !std::strcmp(argv[i + 1], "f16")) { mv_storage = BERTX_INDEX_F16; ++i; }
        else if (!std::strcmp(argv[i], "-S") && has && !std::strcmp(argv[i + 1], "int8")) { mv_storage = BERTX_INDEX_I8; ++i; }
        else if (!std::strcmp(argv[i], "-S") && has && (!std::strcmp(argv[i + 1], "res2") || !std::strcmp(argv[i + 1], "res4"))) {
            // (the store that is filled first is the f16 one the centroids and buckets are trained on)
            mv_storage = BERTX_INDEX_F16;
            res_storage = argv[++i][3] == '2' ? BERTX_INDEX_RES2 : BERTX_INDEX_RES4;
        }
        else if (!std::strcmp(argv[i], "-r") && has) rerank = argv[++i];
        else if (!std::strcmp(argv[i], "-c") && has) cand = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "-C") && has) { cents = std::atoi(argv[++i]); if (cents < 1) cents = -1; }
        else if (!std::strcmp(argv[i], "-l")) late = true;
        else if (!std::strcmp(argv[i], "-a")) all = true;
        else if (!std::strcmp(argv[i], "-M")) no_mask_keys = true;
        else if (!std::strcmp(argv[i], "-L") && has) colbert = argv[++i];
        else { model = nullptr; break; }
    }
    const bool second = rerank || late || colbert;
    const bool bad_all = (all && ((!late && !colbert) || (cand != 0 && cents == 0))) || (cents != 0 && !all) || cents < 0 ||
                         cents % 16 || cents > 65536;
    if (second && (!all || cents) && cand == 0) cand = std::min(128, 4 * k);
    // the rescored first stage: what it is asked for (K) and how many binary candidates it takes
    const int first_k = second && !all ? cand : k;
    const bool bad_bin = ((fine_storage >= 0 || bin_cand != 0) && (storage != BERTX_INDEX_BIN || all)) ||
                         (bin_cand != 0 && fine_storage < 0);
    if (fine_storage >= 0 && bin_cand == 0) bin_cand = std::min(128, 4 * first_k);
    if (bad_bin || (fine_storage >= 0 && (bin_cand < first_k || bin_cand > 128)) || bad_all || !model || !corpus || k < 1 || k > 128 || threads < 1 || (int)(rerank != nullptr) + late + (colbert != nullptr) > 1 ||
        (second && (!all || cents) ? cand < k || cand > 128 : cand != 0) || (mv_storage >= 0 && !late && !colbert) ||
        (no_mask_keys && !colbert) || (res_storage >= 0 && cents == 0)) {
        std::fprintf(stderr, "usage: %s -m MODEL -f CORPUS.txt [-k 3 (1..128)] [-t threads] "
                             "[-s f16|int8|binary [-R f16|int8 (rescore the binary candidates) [-B N (K..128, default 4 K)]]] "
                             "[-r RERANK_MODEL [-c N (k..128, default 4 k)] | -l [-c N | -a [-C CENTROIDS [-c N]]] | "
                             "-L COLBERT_MODEL [-M] [-c N | -a [-C CENTROIDS [-c N]]]] "
                             "[-S f16|int8 (the token store of -l / -L) | res2|res4 (with -a -C)]\n",
                     argv[0]);
        return 2;
    }
    std::vector<std::string> texts;
    {
        std::ifstream in(corpus);
        if (!in) {
            std::fprintf(stderr, "search: cannot read '%s'\n", corpus);
            return 1;
        }
        for (std::string line; std::getline(in, line);) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (!line.empty()) texts.push_back(line);
        }
    }
    if (texts.empty()) {
        std::fprintf(stderr, "search: '%s' holds no text\n", corpus);
        return 1;
    }
    bert_ctx *ctx = bert_load_from_file(model);
    if (!ctx) {
        std::fprintf(stderr, "search: cannot load '%s'\n", model);
        return 1;
    }
    bert_ctx *rctx = nullptr;
    if (rerank) {
        rctx = bert_load_from_file(rerank);
        if (!rctx || bertx_n_labels(rctx) < 1) {
            std::fprintf(stderr, "search: '%s' %s\n", rerank, rctx ? "has no classification head" : "cannot be loaded");
            if (rctx) bert_free(rctx);
            bert_free(ctx);
            return 1;
        }
    }
    // -L: the ColBERT model (in rctx, the second model's place)
    int32_t doc_maxlen = 0, query_maxlen = 0;
    if (colbert) {
        rctx = bert_load_from_file(colbert);
        if (!rctx || bertx_proj_dim(rctx) < 1) {
            std::fprintf(stderr, "search: '%s' %s\n", colbert, rctx ? "has no projection record" : "cannot be loaded");
            if (rctx) bert_free(rctx);
            bert_free(ctx);
            return 1;
        }
        doc_maxlen = std::min<int32_t>(180, bert_n_max_tokens(rctx));
        query_maxlen = std::min<int32_t>(32, bert_n_max_tokens(rctx));
        if (no_mask_keys) bertx_set_mask_keys(rctx, 0);
    }
    if (mv_storage < 0) mv_storage = BERTX_INDEX_F16;
    bertx_index *idx = all ? nullptr : bertx_index_create_ex(ctx, 0, (int32_t)texts.size(), storage);
    bertx_index *fine = idx && fine_storage >= 0 ? bertx_index_create_ex(ctx, 0, (int32_t)texts.size(), fine_storage) : nullptr;
    if ((!idx && !all) || (fine_storage >= 0 && !fine)) {
        bertx_index_free(idx);
        if (rctx) bert_free(rctx);
        bert_free(ctx);
        return 1;
    }
    bertx_mvindex *mv = nullptr;
    if (late) {
        // the store's size: every text's token count, as bert_tokenize counts it
        const int32_t n_max = bert_n_max_tokens(ctx);
        std::vector<bert_vocab_id> tok((size_t)n_max);
        int64_t slots = 0;
        for (const std::string &t : texts) {
            int32_t n = 0;
            bert_tokenize(ctx, t.c_str(), tok.data(), &n, n_max);
            slots += (std::max(n, 1) + 15) / 16 * 16;
        }
        mv = bertx_mvindex_create_ex(ctx, 0, bert_n_embd(ctx), (int32_t)texts.size(), slots, mv_storage);
        if (!mv) {
            bertx_index_free(fine);
            bertx_index_free(idx);
            bert_free(ctx);
            return 1;
        }
    }
    if (colbert) {
        // the store's size: doc_maxlen slots bound every document (its kept rows are fewer)
        const int64_t slots = (int64_t)texts.size() * ((doc_maxlen + 15) / 16 * 16);
        mv = bertx_mvindex_create_ex(rctx, 0, bertx_proj_width(rctx), (int32_t)texts.size(), slots, mv_storage);
        if (!mv) {
            bertx_index_free(fine);
            bertx_index_free(idx);
            bert_free(rctx);
            bert_free(ctx);
            return 1;
        }
    }
    int rc = 0;
    // the corpus in batches (one encoder call each); `to`: the token store that takes them
    auto add_corpus = [&](bertx_index *ix, bertx_mvindex *to) {
        for (size_t i = 0; i < texts.size() && rc == 0; i += 256) {
            std::vector<const char *> p;
            for (size_t j = i; j < texts.size() && j < i + 256; ++j) p.push_back(texts[j].c_str());
            if (ix && (bertx_index_add_texts(ix, ctx, threads, (int32_t)p.size(), p.data()) < 0 ||
                       (fine && bertx_index_add_texts(fine, ctx, threads, (int32_t)p.size(), p.data()) < 0))) {
                std::fprintf(stderr, "search: indexing failed at text %zu\n", i);
                rc = 1;
            } else if (to && (colbert ? bertx_mvindex_add_texts_colbert(to, rctx, threads, (int32_t)p.size(), p.data(), doc_maxlen)
                                      : bertx_mvindex_add_texts(to, ctx, threads, (int32_t)p.size(), p.data())) < 0) {
                std::fprintf(stderr, "search: token indexing failed at text %zu\n", i);
                rc = 1;
            }
        }
    };
    add_corpus(idx, mv);
    if (rc == 0 && cents && bertx_mvindex_train_centroids(mv, cents, 8, 0) != 0) {
        std::fprintf(stderr, "search: training %d centroids failed\n", cents);
        rc = 1;
    }
    if (rc == 0 && res_storage >= 0) {
        // mv is the temporary f16 store: its centroids and the buckets trained on it go to the
        // residual store, which takes the corpus and mv's place
        const int32_t w = bertx_mvindex_dim(mv);
        std::vector<float> cent((size_t)cents * w), cuts(15), wts(16);
        for (int c = 0; c < cents && rc == 0; ++c)
            if (bertx_mvindex_centroid(mv, c, cent.data() + (size_t)c * w) != 0) rc = 1;
        if (rc == 0 && bertx_mvindex_train_residual_buckets(mv, res_storage == BERTX_INDEX_RES2 ? 2 : 4, cuts.data(),
                                                            wts.data()) != 0)
            rc = 1;
        bertx_mvindex *rs = rc ? nullptr
                               : bertx_mvindex_create_ex(colbert ? rctx : ctx, 0, w, bertx_mvindex_capacity_docs(mv),
                                                         bertx_mvindex_capacity_token_slots(mv), res_storage);
        bertx_mvindex_free(mv);
        mv = rs;
        if (!mv || bertx_mvindex_set_centroids(mv, cent.data(), cents) != 0 ||
            bertx_mvindex_set_residual_buckets(mv, cuts.data(), wts.data()) != 0)
            rc = 1;
        if (rc == 0) add_corpus(nullptr, mv);
        if (rc != 0) std::fprintf(stderr, "search: building the residual store failed\n");
    }
    const int kq = second && !all ? cand : k;   // what the index (-a: the token store) is asked for
    std::vector<float> scores((size_t)kq);
    std::vector<int32_t> ids((size_t)kq);
    for (std::string q; rc == 0 && std::getline(std::cin, q);) {
        if (!q.empty() && q.back() == '\r') q.pop_back();
        if (q == "q") break;
        if (q.empty()) continue;
        if (q.compare(0, 4, ":del") == 0 && (q.size() == 4 || q[4] == ' ' || q[4] == '\t')) {
            if (!idx) {
                std::printf("no embedding index (-a): nothing deleted\n");
                std::fflush(stdout);
                continue;
            }
            std::vector<int32_t> del;
            const char *p = q.c_str() + 4;
            for (char *end = nullptr;; p = end) {
                const long v = std::strtol(p, &end, 10);
                if (end == p) break;
                del.push_back(v < 0 || v > 0x7fffffffl ? -1 : (int32_t)v);
            }
            const int32_t before = bertx_index_live(idx);
            if (!del.empty() && (bertx_index_remove(idx, del.data(), (int32_t)del.size()) != 0 ||
                                 (fine && bertx_index_remove(fine, del.data(), (int32_t)del.size()) != 0))) {
                std::fprintf(stderr, "search: deleting failed\n");
                rc = 1;
                break;
            }
            std::printf("deleted %d\n", before - bertx_index_live(idx));
            std::fflush(stdout);
            continue;
        }
        if (q.compare(0, 5, ":drop") == 0 && (q.size() == 5 || q[5] == ' ' || q[5] == '\t')) {
            if (!mv) {
                std::printf("no token store: nothing dropped\n");
                std::fflush(stdout);
                continue;
            }
            std::vector<int32_t> drop;
            const char *p = q.c_str() + 5;
            for (char *end = nullptr;; p = end) {
                const long v = std::strtol(p, &end, 10);
                if (end == p) break;
                drop.push_back(v < 0 || v > 0x7fffffffl ? -1 : (int32_t)v);
            }
            const int32_t before = bertx_mvindex_live(mv);
            if (!drop.empty() && bertx_mvindex_remove(mv, drop.data(), (int32_t)drop.size()) != 0) {
                std::fprintf(stderr, "search: dropping failed\n");
                rc = 1;
                break;
            }
            std::printf("dropped %d\n", before - bertx_mvindex_live(mv));
            std::fflush(stdout);
            continue;
        }
        const char *qp = q.c_str();
        if (all) {
            // the full scan: the k best of every stored document by MaxSim, selected on the GPU
            // (-C: the same over the candidates of the centroid interaction only)
            const int32_t qrc =
                cents ? bertx_mvindex_search_pruned_texts(mv, colbert ? rctx : ctx, threads, 1, &qp, k, cand,
                                                          colbert ? query_maxlen : 0, scores.data(), ids.data())
                : colbert ? bertx_mvindex_search_texts_colbert(mv, rctx, threads, 1, &qp, query_maxlen, k, scores.data(),
                                                               ids.data())
                          : bertx_mvindex_search_texts(mv, ctx, threads, 1, &qp, k, scores.data(), ids.data());
            if (qrc != 0) {
                std::fprintf(stderr, "search: late-interaction search failed\n");
                rc = 1;
                break;
            }
            for (int j = 0; j < k && ids[(size_t)j] >= 0; ++j)
                std::printf("%d\t%d\t%.4f\t%s\n", j + 1, ids[(size_t)j], scores[(size_t)j], texts[(size_t)ids[(size_t)j]].c_str());
            std::fflush(stdout);
            continue;
        }
        if ((fine ? bertx_index_search_rescored_texts(idx, fine, ctx, threads, 1, &qp, kq, bin_cand, scores.data(), ids.data())
                  : bertx_index_search_texts(idx, ctx, threads, 1, &qp, kq, scores.data(), ids.data())) != 0) {
            std::fprintf(stderr, "search: query failed\n");
            rc = 1;
            break;
        }
        if (mv) {
            // the candidates re-scored by MaxSim (a -1 fill slot scores -inf and sorts last, as
            // does a document dropped from the token store, which is not printed)
            std::vector<float> ms((size_t)kq);
            if ((colbert ? bertx_mvindex_score_text_colbert(mv, rctx, qp, query_maxlen, ids.data(), kq, ms.data())
                         : bertx_mvindex_score_text(mv, ctx, qp, ids.data(), kq, ms.data())) != 0) {
                std::fprintf(stderr, "search: late-interaction scoring failed\n");
                rc = 1;
                break;
            }
            std::vector<int> ord((size_t)kq);
            for (int j = 0; j < kq; ++j) ord[(size_t)j] = j;
            std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
                return ms[(size_t)a] > ms[(size_t)b] || (ms[(size_t)a] == ms[(size_t)b] && ids[(size_t)a] < ids[(size_t)b]);
            });
            for (int j = 0; j < k && ids[(size_t)ord[(size_t)j]] >= 0; ++j) {
                const int c = ord[(size_t)j];
                if (ms[(size_t)c] == -INFINITY) break;
                std::printf("%d\t%d\t%.4f\t%s\n", j + 1, ids[(size_t)c], ms[(size_t)c], texts[(size_t)ids[(size_t)c]].c_str());
            }
            std::fflush(stdout);
            continue;
        }
        if (rctx) {
            // the candidates re-scored as (query, text) pairs; the k best by the first logit,
            // equal logits in the index's order
            int n = 0;
            while (n < kq && ids[(size_t)n] >= 0) ++n;
            const int nl = bertx_n_labels(rctx);
            std::vector<const char *> docs((size_t)n);
            for (int j = 0; j < n; ++j) docs[(size_t)j] = texts[(size_t)ids[(size_t)j]].c_str();
            std::vector<float> logits((size_t)n * nl);
            if (n && bertx_rerank(rctx, threads, qp, n, docs.data(), 1, logits.data()) != 0) {
                std::fprintf(stderr, "search: reranking failed\n");
                rc = 1;
                break;
            }
            std::vector<int> ord((size_t)n);
            for (int j = 0; j < n; ++j) ord[(size_t)j] = j;
            std::stable_sort(ord.begin(), ord.end(),
                             [&](int a, int b) { return logits[(size_t)a * nl] > logits[(size_t)b * nl]; });
            for (int j = 0; j < k && j < n; ++j) {
                const int c = ord[(size_t)j];
                std::printf("%d\t%d\t%.4f\t%s\n", j + 1, ids[(size_t)c], logits[(size_t)c * nl],
                            texts[(size_t)ids[(size_t)c]].c_str());
            }
            std::fflush(stdout);
            continue;
        }
        for (int j = 0; j < k && ids[(size_t)j] >= 0; ++j)
            std::printf("%d\t%d\t%.4f\t%s\n", j + 1, ids[(size_t)j], scores[(size_t)j], texts[(size_t)ids[(size_t)j]].c_str());
        std::fflush(stdout);
    }
    bertx_mvindex_free(mv);
    bertx_index_free(fine);
    bertx_index_free(idx);
    if (rctx) bert_free(rctx);
    bert_free(ctx);
    return rc;
}
