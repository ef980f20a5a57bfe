// How a call's sentences are cut into device forwards: one rule for the pooled and the
// per-token host forms (bert_abi.cpp run_forward, forward_rows) and the token store's
// add_texts (mvindex.cpp).  Plain C++, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>

namespace emb {

constexpr int64_t kChunkTokens = 1 << 17;   // tokens per device forward (workspace bound)
constexpr int kChunkSeqs = 4096;            // sentences per device forward (pool / output staging bound)

// The end of the chunk that begins at sentence `start` of n: at least one sentence, then
// further ones while the chunk's tokens stay <= max_tokens and it has fewer than max_seqs
// sentences.  len_at(i): the tokens of sentence i in the caller's order.
template <class LenAt>
inline size_t chunk_end(LenAt len_at, size_t start, size_t n, int64_t max_tokens = kChunkTokens, int max_seqs = kChunkSeqs)
{
    size_t i = start;
    int64_t tok = 0;
    while (i < n && (i == start || (tok + len_at(i) <= max_tokens && (int64_t)(i - start) < max_seqs))) tok += len_at(i++);
    return i;
}

}  // namespace emb
