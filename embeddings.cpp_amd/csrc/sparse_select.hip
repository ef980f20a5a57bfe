// Top-n term selection of the sparse index (bert_hip.h "Sparse index") and
// the pack of its output into postings.
//
// Selection.  rows f32 [S][V], non-negative; per row the min(n, number of weights > 0)
// terms of largest weight, equal weights by ascending term, written in ascending term.
// Non-negative floats order as their unsigned bits (sparse.hip's atomicMax rests on the
// same fact), so the kernel never does arithmetic on a value: key = the bits of a weight
// whose sign bit is clear, 0 otherwise (-0 and anything negative count as "not > 0").
//
// One workgroup of 16 waves per row, four reads of the row (L2 after the first):
//   passes 1-3  radix select of the n'-th largest key, n' = min(n, V): a histogram in LDS
//               (ds_add) over key bits 31..21, then 20..10, then 9..0 of the keys that match
//               the prefix chosen so far; after each histogram every thread owns two bins,
//               a suffix sum over the threads (shuffles in a wave, the 16 wave totals
//               through LDS) finds the bin that holds the n'-th largest and how many keys
//               lie above it.  The result: the threshold T = that key and `take` = the
//               keys == T still to be chosen (n' less the keys > T).  T == 0 means the row
//               has fewer than n' positive weights: every positive weight is chosen and
//               no zero is (take = 0).
//   pass 4      ordered compaction, 1,024 terms per step in ascending term: per wave a
//               ballot of key > T and one of key == T, lane prefixes by popcount, the wave
//               totals of the step through LDS in wave order (double-buffered: one barrier
//               per step).  A chosen term's slot is (keys > T before it) + min(keys == T
//               before it, take); a key == T is chosen while fewer than `take` precede it.
// No global atomics, no allocation: capturable.
#include "device_common.h"
#include "kernels.h"

namespace emb {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kBins = 2048;   // 11 bits; the last pass uses the lower 1,024

__device__ __forceinline__ uint32_t key_of(uint32_t bits) { return (int32_t)bits > 0 ? bits : 0u; }

// The bin that holds the r-th largest (r >= 1) of the keys counted in hist, and how many
// lie in the bins above it.  Every thread returns the same pair.
__device__ __forceinline__ uint2 find_bin(const uint32_t *hist, uint32_t r, uint32_t *wtot, uint32_t *sel, int tid)
{
    const int lane = tid & 63, wv = tid >> 6;
    const uint32_t h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
    uint32_t x = h0 + h1;   // -> the sum over this wave's lanes >= lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_down(x, o, 64);
        if (lane + o < 64) x += y;
    }
    if (lane == 0) wtot[wv] = x;
    lds_barrier();
    uint32_t excl = x - (h0 + h1);   // the keys in the bins above this thread's two
    for (int w = wv + 1; w < kWaves; ++w) excl += wtot[w];
    if (excl < r && excl + h1 >= r) {
        sel[0] = 2 * tid + 1;
        sel[1] = excl;
    } else if (excl + h1 < r && excl + h1 + h0 >= r) {
        sel[0] = 2 * tid;
        sel[1] = excl + h1;
    }
    lds_barrier();
    return uint2{sel[0], sel[1]};
}

__global__ __launch_bounds__(kThreads) void sparse_select_kernel(const uint32_t *__restrict__ rows, int V, int n,
                                                                 int32_t *__restrict__ terms,
                                                                 uint32_t *__restrict__ weights,
                                                                 int32_t *__restrict__ count)
{
    __shared__ uint32_t hist[kBins];
    __shared__ uint32_t wtot[kWaves], sel[2];
    __shared__ uint2 tot[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t *row = rows + (size_t)blockIdx.x * V;
    int32_t *ot = terms + (size_t)blockIdx.x * n;
    uint32_t *ow = weights + (size_t)blockIdx.x * n;

    uint32_t r = (uint32_t)min(n, V), prefix = 0;
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;       // the pass's digit
        const int hi = pass == 0 ? 32 : pass == 1 ? 21 : 10;         // the bits above it: the prefix
        const uint32_t mask = pass == 2 ? 0x3ffu : 0x7ffu;
        hist[2 * tid] = 0;
        hist[2 * tid + 1] = 0;
        lds_barrier();
        for (int i = tid; i < V; i += kThreads) {
            const uint32_t key = key_of(row[i]);
            if (pass == 0 || (key >> hi) == prefix) atomicAdd(&hist[(key >> shift) & mask], 1u);
        }
        lds_barrier();
        const uint2 f = find_bin(hist, r, wtot, sel, tid);
        prefix = (prefix << (pass == 2 ? 10 : 11)) | f.x;
        r -= f.y;
    }
    const uint32_t T = prefix, take = T ? r : 0u;

    uint32_t run_gt = 0, run_eq = 0;
    int par = 0;
    for (int base = 0; base < V; base += kThreads, par ^= 1) {
        const int i = base + tid;
        const uint32_t bits = i < V ? row[i] : 0u, key = key_of(bits);
        const bool gt = key > T, eq = T != 0 && key == T;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq), below = (1ull << lane) - 1ull;
        if (lane == 0) tot[par][wv] = uint2{(uint32_t)__popcll(bg), (uint32_t)__popcll(be)};
        lds_barrier();
        uint32_t gb = run_gt + (uint32_t)__popcll(bg & below), eb = run_eq + (uint32_t)__popcll(be & below);
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint2 t = tot[par][w];
            if (w < wv) { gb += t.x; eb += t.y; }
            run_gt += t.x;
            run_eq += t.y;
        }
        if (gt || (eq && eb < take)) {
            const uint32_t pos = gb + min(eb, take);
            if (pos < (uint32_t)n) {   // (always: at most min(n, V) terms are chosen)
                ot[pos] = i;
                ow[pos] = bits;
            }
        }
    }
    const int cnt = (int)min(run_gt + min(run_eq, take), (uint32_t)n);
    for (int j = cnt + tid; j < n; j += kThreads) {
        ot[j] = -1;
        ow[j] = 0u;
    }
    if (tid == 0) count[blockIdx.x] = cnt;
}

// The table entries of the m documents of one add chunk, d_used[0] the store's used units
// before the chunk: entry i = (first unit, postings), the units an exclusive prefix sum of
// ceil(count / 16) in document order.  One workgroup, m <= kThreads; the host never sees
// the counts.  d_used[0] advances by the chunk's units.
__global__ __launch_bounds__(kThreads) void sparse_offsets_kernel(const int32_t *__restrict__ count, int m,
                                                                  int2 *__restrict__ table, int32_t *__restrict__ d_used)
{
    __shared__ uint32_t wtot[kWaves];
    __shared__ int32_t base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base = d_used[0];   // the one read of it, by the thread that writes it
    const int c = tid < m ? count[tid] : 0;
    const uint32_t u = (uint32_t)(c + 15) >> 4;
    uint32_t x = u;   // -> the inclusive prefix over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wtot[wv] = x;
    lds_barrier();
    uint32_t before = x - u, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wv) before += wtot[w];
        total += wtot[w];
    }
    const int32_t used = base;
    if (tid < m) table[tid] = int2{used + (int32_t)before, c};
    if (tid == 0) d_used[0] = used + (int32_t)total;
}

// One workgroup per document of the chunk: posting j = term | f16(weight) << 16 for
// j < count, (term 0, +0) up to the unit's end.
__global__ __launch_bounds__(256) void sparse_pack_kernel(const int32_t *__restrict__ terms,
                                                          const float *__restrict__ weights, int n,
                                                          const int2 *__restrict__ table, uint32_t *__restrict__ store)
{
    const int2 e = table[blockIdx.x];
    const int padded = (e.y + 15) & ~15;
    uint32_t *dst = store + (size_t)e.x * 16;
    for (int j = threadIdx.x; j < padded; j += 256) {
        uint32_t p = 0;
        if (j < e.y) {
            const h16 w = (h16)weights[(size_t)blockIdx.x * n + j];
            p = (uint32_t)terms[(size_t)blockIdx.x * n + j] | (uint32_t)__builtin_bit_cast(uint16_t, w) << 16;
        }
        dst[j] = p;
    }
}

}  // namespace

int launch_sparse_select(const float *d_rows, int S, int V, int n, int32_t *d_terms, float *d_weights, int32_t *d_count,
                         hipStream_t s)
{
    if (!d_rows || !d_terms || !d_weights || !d_count || S < 1 || V < 1 || V > 65536 || n < 1 || n > 1024) return -1;
    sparse_select_kernel<<<(unsigned)S, kThreads, 0, s>>>((const uint32_t *)d_rows, V, n, d_terms, (uint32_t *)d_weights,
                                                          d_count);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_sparse_pack(const int32_t *d_terms, const float *d_weights, const int32_t *d_count, int m, int n,
                       void *d_table, int32_t *d_used, uint32_t *store, hipStream_t s)
{
    if (!d_terms || !d_weights || !d_count || !d_table || !d_used || !store || m < 1 || m > kSparseAddRows || n < 1 ||
        n > 1024)
        return -1;
    sparse_offsets_kernel<<<1, kThreads, 0, s>>>(d_count, m, (int2 *)d_table, d_used);
    if (hipGetLastError() != hipSuccess) return -3;
    sparse_pack_kernel<<<(unsigned)m, 256, 0, s>>>(d_terms, d_weights, n, (const int2 *)d_table, store);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
