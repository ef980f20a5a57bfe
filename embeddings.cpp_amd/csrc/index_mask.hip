// The row masks of the embedding index (bertx_index_remove / _live / _deleted, bert_hip.h
// "Deleting rows and filtered search"): the kernels that write and read the
// index's tombstones.  A mask packs 32 rows to a uint32_t word, row r = bit r % 32 of word
// r / 32 (np.packbits(x, bitorder="little") viewed as uint32); a tombstone bit of 1 means
// deleted.  The scans that consult the masks are search.hip, search_bin.hip and
// search_rescore.hip.
#include "device_common.h"
#include "kernels.h"

#include <algorithm>

namespace emb {
namespace {

constexpr int kThreads = 256;

// One thread per listed id: ids outside [0, n_rows) are ignored, repeated ids set the same
// bit.  The bit is set with an atomic OR on the word (global_atomic_or), so neither the
// order of the ids nor two removals in flight matter.
__global__ __launch_bounds__(kThreads) void index_remove_kernel(const int32_t *__restrict__ ids, int n, int n_rows,
                                                                uint32_t *__restrict__ tomb)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = (uint32_t)ids[i];
    if (id < (uint32_t)n_rows) atomicOr(tomb + (id >> 5), 1u << (id & 31));
}

// *count += the tombstones set among rows [0, n_rows): whole words by popcount, the last
// word masked to its rows below n_rows.  One atomic add per wave.
__global__ __launch_bounds__(kThreads) void index_count_deleted_kernel(const uint32_t *__restrict__ tomb, int n_rows,
                                                                       int32_t *__restrict__ count)
{
    const int words = (n_rows + 31) >> 5;
    int c = 0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < words; i += gridDim.x * kThreads) {
        uint32_t v = tomb[i];
        if (i == words - 1 && (n_rows & 31)) v &= (1u << (n_rows & 31)) - 1u;
        c += __popc(v);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// out[i] = the tombstone of row first + i, 0 or 1.
__global__ __launch_bounds__(kThreads) void index_deleted_flags_kernel(const uint32_t *__restrict__ tomb, int first, int n,
                                                                       uint8_t *__restrict__ out)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t r = (int64_t)first + i;
    out[i] = (uint8_t)((tomb[r >> 5] >> (r & 31)) & 1);
}

}  // namespace

int64_t index_mask_words(int64_t capacity_rows) { return (capacity_rows + 63) / 64 * 2; }

int launch_index_remove(const int32_t *d_ids, int n, int64_t n_rows, uint32_t *tomb, hipStream_t s)
{
    if (!d_ids || !tomb || n < 1 || n_rows < 0 || n_rows > 0x7ffffff0) return -1;
    index_remove_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(d_ids, n, (int)n_rows, tomb);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_index_count_deleted(const uint32_t *tomb, int64_t n_rows, int32_t *d_count, hipStream_t s)
{
    if (!tomb || !d_count || n_rows < 0 || n_rows > 0x7ffffff0) return -1;
    if (hipMemsetAsync(d_count, 0, 4, s) != hipSuccess) return -3;
    if (n_rows == 0) return 0;
    const int64_t words = (n_rows + 31) / 32;
    const unsigned blocks = (unsigned)std::min<int64_t>(1024, (words + kThreads - 1) / kThreads);
    index_count_deleted_kernel<<<blocks, kThreads, 0, s>>>(tomb, (int)n_rows, d_count);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_index_deleted_flags(const uint32_t *tomb, int64_t first, int n, uint8_t *d_out, hipStream_t s)
{
    if (!tomb || !d_out || first < 0 || n < 1 || first + n > 0x7ffffff0) return -1;
    index_deleted_flags_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(tomb, (int)first, n, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace emb
