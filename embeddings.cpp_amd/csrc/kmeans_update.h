// The host half of centroid training (bertx_mvindex_train_centroids, bert_hip.h "Centroid
// codes"): which token rows are sampled, and the update of the centroids from the sample's
// codes.  Host code only, no device and no library state, so that it can be compiled into a
// stand-alone program.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace emb {

// Of T valid token rows numbered in (document, token) order the sample is rows start,
// start + stride, ...: stride = max(1, ceil(T / 2^18)), start = seed % stride.
struct KmeansSample {
    int64_t stride = 1, start = 0, n = 0;
};

inline KmeansSample kmeans_sample(int64_t T, uint32_t seed)
{
    KmeansSample s;
    s.stride = T > (1ll << 18) ? (T + (1ll << 18) - 1) >> 18 : 1;
    s.start = (int64_t)(seed % (uint64_t)s.stride);
    s.n = T > s.start ? (T - s.start + s.stride - 1) / s.stride : 0;
    return s;
}

// The initial centroid c of C is sample row floor(c n / C).
inline int64_t kmeans_initial_row(int64_t c, int64_t n, int64_t C) { return c * n / C; }

// One update: centroid c becomes the sum of the sample rows whose code is c, in f64, added
// one after the other in ascending sample order, divided by their count and rounded to f32;
// a centroid without a member keeps its row.  sample f32 [n][w], codes [n] (each < C),
// cent f32 [C][w] in place.  Returns the number of centroids without a member.
inline int64_t kmeans_update(const float *sample, const uint16_t *codes, int64_t n, int w, int64_t C, float *cent)
{
    std::vector<double> sum((size_t)C * w, 0.0);
    std::vector<int64_t> cnt((size_t)C, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t c = codes[i];
        if (c >= C) continue;   // (never: a code is an index into the centroids)
        double *s = sum.data() + (size_t)c * w;
        const float *x = sample + (size_t)i * w;
        for (int e = 0; e < w; ++e) s[e] += (double)x[e];
        ++cnt[(size_t)c];
    }
    int64_t empty = 0;
    for (int64_t c = 0; c < C; ++c) {
        if (cnt[(size_t)c] == 0) {
            ++empty;
            continue;
        }
        const double m = (double)cnt[(size_t)c];
        for (int e = 0; e < w; ++e) cent[(size_t)c * w + e] = (float)(sum[(size_t)c * w + e] / m);
    }
    return empty;
}

}  // namespace emb
