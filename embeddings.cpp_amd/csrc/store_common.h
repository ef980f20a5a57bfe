// What the two device-resident stores share (index.cpp, mvindex.cpp): the ordering of a
// store's device operations, an owned device buffer, and the host loops that unpack the
// search kernels' fragment order (kernels.h) into rows.  Host code only.
#pragma once

#include "host_common.h"

#include <hip/hip_runtime.h>

namespace emb {

inline bool capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

// Every device operation on a store is ordered after the previous one: an operation on
// another stream first waits (on the device) for `done`.  The store creates and destroys
// the event; the fields are read and written under the store's mutex.
struct StoreOrder {
    hipEvent_t done = nullptr;          // completion of the last device operation on the store
    hipStream_t last_stream = nullptr;  // ... and the stream it ran on
    bool any = false;
    // the host waits for the last operation (before it reads the store with a blocking copy)
    hipError_t wait() const { return any ? hipEventSynchronize(done) : hipSuccess; }
};

// Orders an operation on `s` after the store's previous one and, on destruction, records
// it as the new previous one.  A capturing stream records and waits for nothing outside
// its graph: the captured operation is ordered by its stream alone.
struct Ordered {
    StoreOrder &o;
    hipStream_t s;
    const bool cap;
    Ordered(StoreOrder &ord, hipStream_t st) : o(ord), s(st), cap(capturing(st))
    {
        if (!cap && o.any && o.last_stream != s) (void)hipStreamWaitEvent(s, o.done, 0);
    }
    ~Ordered()
    {
        if (cap) return;
        (void)hipEventRecord(o.done, s);
        o.last_stream = s;
        o.any = true;
    }
};

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// The filters of one search (device memory): none (d null, n 0), one for every query
// (stride 0) or one per query, `stride` words apart.  A mask packs 32 units (rows of the
// embedding index, documents of the token store) to a uint32_t word.
struct Filters {
    const uint32_t *d = nullptr;
    int64_t stride = 0;
    Filters from(int64_t query) const
    {
        Filters f = *this;
        if (f.d) f.d += (size_t)query * (size_t)stride;
        return f;
    }
};

// What a filtered search accepts over a store of n units (the store locked): no filter as
// (NULL, 0), else 1 or B filters of at least ceil(n / 32) words.
inline bool filters_fit(int64_t n, const void *filters, int32_t n_filters, int32_t words, int32_t B)
{
    if (!filters || n_filters == 0) return !filters && n_filters == 0;
    return (n_filters == 1 || n_filters == B) && (int64_t)words >= (n + 31) / 32;
}

inline Filters filters_of(const uint32_t *d_filters, int32_t n_filters, int32_t words)
{
    Filters f;
    f.d = d_filters;
    f.stride = n_filters > 1 ? words : 0;
    return f;
}

// The filters of a host call, uint32 [n_filters][words], staged in a device buffer of the
// call's own (the store locked, its device current); the copy is ordered on the store's stream.
inline hipError_t stage_filters(hipStream_t stream, const uint32_t *filters, int32_t n_filters, int32_t words, DevBuf &buf)
{
    if (!filters) return hipSuccess;
    const size_t bytes = (size_t)n_filters * (size_t)words * 4;
    hipError_t e = hipMalloc(&buf.p, bytes > 4 ? bytes : 4);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(buf.p, filters, bytes, hipMemcpyHostToDevice, stream);
    return e;
}

// The unpackers.  image: a host copy of whole 16-row groups of width w, of which the
// first holds row image_first (a multiple of 16); rows first .. first + n - 1 of it go to
// out [n][w].  An int8 store's scales stay with the caller (the two stores index them
// differently).
inline void unpack_f16_rows(const uint16_t *image, int64_t image_first, int64_t first, int64_t n, int w, float *out)
{
    const int KB = w / 32;
    const size_t group_halfs = (size_t)16 * w;
    for (int64_t r = first; r < first + n; ++r) {
        const uint16_t *grp = image + (size_t)((r - image_first) / 16) * group_halfs;
        float *o = out + (size_t)(r - first) * w;
        for (int kb = 0; kb < KB; ++kb)
            for (int q = 0; q < 4; ++q)
                for (int j = 0; j < 8; ++j) o[32 * kb + 8 * q + j] = f16_to_f32(grp[((size_t)kb * 64 + 16 * q + (r & 15)) * 8 + j]);
    }
}

inline void unpack_i8_rows(const int8_t *image, int64_t image_first, int64_t first, int64_t n, int w, int8_t *out)
{
    const int KB = w / 64;
    const size_t group_bytes = (size_t)16 * w;
    for (int64_t r = first; r < first + n; ++r) {
        const int8_t *grp = image + (size_t)((r - image_first) / 16) * group_bytes;
        int8_t *o = out + (size_t)(r - first) * w;
        for (int kb = 0; kb < KB; ++kb)
            for (int g = 0; g < 4; ++g) std::memcpy(o + 64 * kb + 16 * g, grp + ((size_t)kb * 64 + 16 * g + (r & 15)) * 16, 16);
    }
}

// The binary index's bit order (bin_bits.h): image holds whole 64-row groups of
// ceil(w / 128) blocks, image_first a multiple of 64; element i of a row is bit i % 32 of
// dword (i % 128) / 32 of the row's 16-B chunk i / 128.  out uint8 [n][w / 8] in np.packbits
// order: element i is bit 7 - i % 8 of byte i / 8.
inline void unpack_bin_rows(const uint32_t *image, int64_t image_first, int64_t first, int64_t n, int w, uint8_t *out)
{
    const size_t group_words = (size_t)((w + 127) / 128) * 256;
    for (int64_t r = first; r < first + n; ++r) {
        const uint32_t *grp = image + (size_t)((r - image_first) / 64) * group_words;
        uint8_t *o = out + (size_t)(r - first) * (w / 8);
        std::memset(o, 0, (size_t)(w / 8));
        for (int i = 0; i < w; ++i) {
            const uint32_t word = grp[((size_t)(i / 128) * 64 + (size_t)(r & 63)) * 4 + (i % 128) / 32];
            if ((word >> (i % 32)) & 1) o[i / 8] |= (uint8_t)(0x80 >> (i % 8));
        }
    }
}

}  // namespace emb
