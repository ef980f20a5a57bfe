// search: the reference's sample client (examples/sample_dylib.py:84-94: embed a
// corpus, then print the k closest texts of every query) with the corpus resident on
// the GPU and the search fused there (bertx_index_*).
//
// usage: search -m MODEL -f CORPUS.txt [-k 3] [-t threads]
// One text per line of CORPUS.txt; queries from stdin, one per line, `q` or EOF ends.
// Per hit one line: rank<TAB>id<TAB>score<TAB>text.
#include "bert.h"
#include "bert_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char **argv)
{
    const char *model = nullptr, *corpus = nullptr;
    int k = 3, threads = 4;
    for (int i = 1; i < argc; ++i) {
        const bool has = i + 1 < argc;
        if (!std::strcmp(argv[i], "-m") && has) model = argv[++i];
        else if (!std::strcmp(argv[i], "-f") && has) corpus = argv[++i];
        else if (!std::strcmp(argv[i], "-k") && has) k = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "-t") && has) threads = std::atoi(argv[++i]);
        else { model = nullptr; break; }
    }
    if (!model || !corpus || k < 1 || k > 128 || threads < 1) {
        std::fprintf(stderr, "usage: %s -m MODEL -f CORPUS.txt [-k 3 (1..128)] [-t threads]\n", argv[0]);
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
    bertx_index *idx = bertx_index_create(ctx, 0, (int32_t)texts.size());
    if (!idx) {
        bert_free(ctx);
        return 1;
    }
    int rc = 0;
    // the corpus in batches (one encoder call each)
    for (size_t i = 0; i < texts.size() && rc == 0; i += 256) {
        std::vector<const char *> p;
        for (size_t j = i; j < texts.size() && j < i + 256; ++j) p.push_back(texts[j].c_str());
        if (bertx_index_add_texts(idx, ctx, threads, (int32_t)p.size(), p.data()) < 0) {
            std::fprintf(stderr, "search: indexing failed at text %zu\n", i);
            rc = 1;
        }
    }
    std::vector<float> scores((size_t)k);
    std::vector<int32_t> ids((size_t)k);
    for (std::string q; rc == 0 && std::getline(std::cin, q);) {
        if (!q.empty() && q.back() == '\r') q.pop_back();
        if (q == "q") break;
        if (q.empty()) continue;
        const char *qp = q.c_str();
        if (bertx_index_search_texts(idx, ctx, threads, 1, &qp, k, scores.data(), ids.data()) != 0) {
            std::fprintf(stderr, "search: query failed\n");
            rc = 1;
            break;
        }
        for (int j = 0; j < k && ids[(size_t)j] >= 0; ++j)
            std::printf("%d\t%d\t%.4f\t%s\n", j + 1, ids[(size_t)j], scores[(size_t)j], texts[(size_t)ids[(size_t)j]].c_str());
        std::fflush(stdout);
    }
    bertx_index_free(idx);
    bert_free(ctx);
    return rc;
}
