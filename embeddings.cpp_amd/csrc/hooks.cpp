// Per-kernel parity hooks and micro-benchmarks (bert_hip.h bertx_test_* /
// bertx_bench_*): one launch on device 0 over host buffers.  Test infrastructure
// inside the library; the forward never calls these.
#include "bert_hip.h"
#include "engine.h"
#include "hip_check.h"
#include "repack.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace emb {
namespace {

// Device buffers of one hook call, freed together.
struct HookBufs {
    std::vector<void *> p;
    bool bad = false;
    void *up(const void *h, size_t bytes, size_t alloc)
    {
        void *d = nullptr;
        alloc = std::max<size_t>(std::max(alloc, bytes), 16);
        if (hipMalloc(&d, alloc) != hipSuccess) { bad = true; return nullptr; }
        p.push_back(d);
        if (hipMemset(d, 0, alloc) != hipSuccess) bad = true;
        if (h && bytes && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) bad = true;
        return d;
    }
    // the same with every byte the host does not give set to 0xFF (NaN bits): a
    // buffer the kernel writes, so an element it left alone and a store behind the
    // rows it owns both show
    void *up_ff(const void *h, size_t bytes, size_t alloc)
    {
        void *d = up(nullptr, 0, std::max(alloc, bytes));
        if (!d) return nullptr;
        if (hipMemset(d, 0xff, std::max<size_t>(std::max(alloc, bytes), 16)) != hipSuccess) bad = true;
        if (h && bytes && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) bad = true;
        return d;
    }
    ~HookBufs() { for (void *d : p) (void)hipFree(d); }
};

// Rows behind the launched ones of every buffer a GEMM hook's kernels write (one
// 64-row tile), 0xFF before the launch and checked after it.
constexpr int HOOK_GUARD = 64;

// 0 when `bytes` device bytes at d still hold 0xFF, -5 when one was written, -1 on a copy error
int guard_intact(const void *d, size_t bytes)
{
    std::vector<uint8_t> h(bytes);
    if (hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (const uint8_t v : h)
        if (v != 0xff) return -5;
    return 0;
}

// Pad rows of a hook's inputs (rows M .. rows - 1, computed and stored as the
// forward's are): finite, non-zero, magnitudes in [0.25, 1.25) with both signs.
struct PadFill {
    uint32_t st = 2463534242u;
    float next()
    {
        st = st * 1664525u + 1013904223u;
        const float v = 0.25f + (float)(st >> 8) / 16777216.0f;
        return (st & 0x80u) ? -v : v;
    }
};

// f16 rows [M][cols] of the host (may be null with M == 0) -> [rows][cols] with the pad rows filled
std::vector<uint16_t> padded_h16(const uint16_t *h, int M, int rows, int cols, PadFill &pf)
{
    std::vector<uint16_t> v((size_t)rows * cols);
    if (h && M > 0) std::memcpy(v.data(), h, (size_t)M * cols * 2);
    for (size_t i = (size_t)M * cols; i < v.size(); ++i) v[i] = f32_to_f16(pf.next());
    return v;
}

// (mean, 1/sigma) pairs [M] -> [rows], pad rows (mean, 1/sigma) with 1/sigma > 0
std::vector<float> padded_stats(const float *h, int M, int rows, PadFill &pf)
{
    std::vector<float> v((size_t)rows * 2);
    std::memcpy(v.data(), h, (size_t)M * 8);
    for (int r = M; r < rows; ++r) {
        v[2 * (size_t)r] = pf.next();
        v[2 * (size_t)r + 1] = 0.5f + std::fabs(pf.next());
    }
    return v;
}

// The two events of a device-timed bench loop.
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t create()
    {
        const hipError_t e = hipEventCreate(&a);
        return e != hipSuccess ? e : hipEventCreate(&b);
    }
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// A per-thread test switch (g_gemm_cfg, g_att_variant) set for a scope.
struct ScopedSet {
    int &var;
    const int prev;
    ScopedSet(int &v, int value) : var(v), prev(v) { var = value; }
    ~ScopedSet() { var = prev; }
    ScopedSet(const ScopedSet &) = delete;
    ScopedSet &operator=(const ScopedSet &) = delete;
};

// The weight of a hook call in the device layout; t keeps the file-format rows.
bool hook_weight(int32_t fmt, int32_t N, int32_t K, const void *w_rows, HostTensor &t, DevWeight &W, HookBufs &B)
{
    t.fmt = fmt; t.ne0 = K; t.ne1 = N;
    t.bytes.assign((const uint8_t *)w_rows, (const uint8_t *)w_rows + fmt_row_bytes(fmt, K) * (size_t)N);
    Piece q, dd, mm;
    repack_linear({&t}, fmt, q, dd, mm, W.N, W.K);
    W.fmt = fmt == FMT_F32 ? FMT_F16 : fmt;
    W.kx = fmt == FMT_F32 ? W.K / 2 : 0;
    W.qs = B.up(q.bytes.data(), q.bytes.size(), 0);
    W.d = (const uint16_t *)(dd.bytes.empty() ? nullptr : B.up(dd.bytes.data(), dd.bytes.size(), 0));
    W.m = (const uint16_t *)(mm.bytes.empty() ? nullptr : B.up(mm.bytes.data(), mm.bytes.size(), 0));
    return !B.bad;
}

HostTensor vec_tensor(const float *v, int n)
{
    HostTensor t;
    t.fmt = FMT_F32; t.ne0 = n; t.ne1 = 1;
    t.bytes.assign((const uint8_t *)v, (const uint8_t *)(v + n));
    return t;
}

}  // namespace
}  // namespace emb

extern "C" int32_t bertx_test_gemm(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                   int32_t M, const uint16_t *x, int32_t epi, const void *res, void *out,
                                   int32_t cfg)
{
    return bertx_test_gemm_ln(fmt, N, K, w_rows, bias, M, x, nullptr, nullptr, nullptr, epi, (const uint16_t *)res,
                              nullptr, nullptr, nullptr, nullptr, (uint16_t *)out, nullptr, cfg);
}

extern "C" int32_t bertx_test_cu_count(void)
{
    using namespace emb;
    if (hip_device_count() == 0) return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    return device_cu_count();
}

// the M-row forms: the launch padded to the 256-row tile, the first M rows returned
extern "C" int32_t bertx_test_gemm_fold(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                        int32_t M, const uint16_t *x, const float *part, const float *in_g,
                                        const float *in_b, int32_t epi, uint16_t *out, float *st_out,
                                        float *st_kernel, int32_t cfg)
{
    using namespace emb;
    if (M <= 0 || N <= 0 || !out) return -1;
    const int rows = (int)align_up((size_t)M, GEMM_BM);
    std::vector<uint16_t> o((size_t)rows * N);
    std::vector<float> s((size_t)rows * 2), sk((size_t)rows * 2);
    const int rc = bertx_test_gemm_fold_rows(fmt, N, K, w_rows, bias, M, rows, x, part, in_g, in_b, epi, o.data(),
                                             s.data(), st_kernel ? sk.data() : nullptr, cfg);
    if (rc != 0) return rc;
    std::memcpy(out, o.data(), (size_t)M * N * 2);
    if (st_out) std::memcpy(st_out, s.data(), (size_t)M * 8);
    if (st_kernel) std::memcpy(st_kernel, sk.data(), (size_t)M * 8);
    return 0;
}

extern "C" int32_t bertx_test_gemm_fold_rows(int32_t fmt, int32_t N, int32_t K, const void *w_rows,
                                             const float *bias, int32_t M, int32_t rows, const uint16_t *x,
                                             const float *part, const float *in_g, const float *in_b, int32_t epi,
                                             uint16_t *out, float *st_out, float *st_kernel, int32_t cfg)
{
    using namespace emb;
    if (!fmt_valid(fmt) || K % 64 || N % 32 || M <= 0 || rows < M || rows % 64 || (epi != 0 && epi != 1) || !part ||
        !in_g || !in_b || !x || !out || hip_device_count() == 0)
        return -1;
    const int Mp = rows, G = K / 32;   // (X columns: K for every format)
    const int PS = Mp + HOOK_GUARD;     // rows of the guarded [row] buffers
    PadFill pf;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    HostTensor t;
    DevWeight W;
    if (!hook_weight(fmt, N, K, w_rows, t, W, B)) return -1;
    ScopedSet tile(g_gemm_cfg, cfg);
    if (!gemm_fold_ok(W, Mp, G)) return -2;
    const HostTensor hb = vec_tensor(bias, N), hg = vec_tensor(in_g, K), hbt = vec_tensor(in_b, K);
    Piece c1, c2;
    fold_ln({&t}, {&hb}, hg, hbt, c1, c2, fmt == FMT_F32);
    LnFold ln;
    // partials [G][M] on the host -> [G][Mp] on the device (stride Mp)
    // (the pad rows: a sum and a positive sum of squared deviations)
    std::vector<float> hp((size_t)G * Mp * 2);
    for (int g = 0; g < G; ++g) {
        float *row = &hp[(size_t)g * Mp * 2];
        std::memcpy(row, part + (size_t)g * M * 2, (size_t)M * 8);
        for (int r = M; r < Mp; ++r) {
            row[2 * r] = 32.0f * pf.next();
            row[2 * r + 1] = 16.0f + 16.0f * std::fabs(pf.next());
        }
    }
    ln.in_part = (const float2 *)B.up(hp.data(), hp.size() * 4, 0);
    ln.in_part_stride = Mp;
    ln.in_G = G;
    ln.st_out = (float2 *)B.up_ff(nullptr, 0, (size_t)PS * 8);
    ln.c1 = (const float *)B.up(c1.bytes.data(), c1.bytes.size(), 0);
    const float *dbias = (const float *)B.up(c2.bytes.data(), c2.bytes.size(), 0);
    const std::vector<uint16_t> hx = padded_h16(x, M, Mp, K, pf);
    void *dx = B.up(hx.data(), hx.size() * 2, 0);
    void *dout = B.up_ff(nullptr, 0, (size_t)PS * N * 2);
    if (B.bad) return -1;
    const int rc = launch_gemm(W, (const uint16_t *)dx, Mp, dbias, epi, nullptr, dout, nullptr, ln);
    if (rc != 0) return rc;
    HIP_RC(hipGetLastError());
    HIP_RC(hipDeviceSynchronize());
    HIP_RC(hipMemcpy(out, dout, (size_t)Mp * N * 2, hipMemcpyDeviceToHost));
    if (st_out) HIP_RC(hipMemcpy(st_out, ln.st_out, (size_t)Mp * 8, hipMemcpyDeviceToHost));
    if (const int g = guard_intact((const uint16_t *)dout + (size_t)Mp * N, (size_t)HOOK_GUARD * N * 2)) return g;
    if (const int g = guard_intact(ln.st_out + Mp, (size_t)HOOK_GUARD * 8)) return g;
    if (st_kernel) {
        // the same partials through the statistics kernel (the launch form)
        float2 *dk = (float2 *)B.up_ff(nullptr, 0, (size_t)PS * 8);
        if (B.bad || launch_ln_stats(ln.in_part, G, Mp, Mp, 32 * G, dk, nullptr) != 0) return -1;
        HIP_RC(hipDeviceSynchronize());
        HIP_RC(hipMemcpy(st_kernel, dk, (size_t)Mp * 8, hipMemcpyDeviceToHost));
        if (const int g = guard_intact(dk + Mp, (size_t)HOOK_GUARD * 8)) return g;
    }
    return 0;
}

extern "C" int32_t bertx_test_gemm_ln(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                      int32_t M, const uint16_t *x, const float *in_stats, const float *in_g,
                                      const float *in_b, int32_t epi, const uint16_t *res, const float *res_stats,
                                      const float *res_g, const float *res_b, const float *g_next, uint16_t *out,
                                      float *st_out, int32_t cfg)
{
    using namespace emb;
    if (M <= 0 || N <= 0 || !out) return -1;
    const int rows = (int)align_up((size_t)M, GEMM_BM);
    std::vector<uint16_t> o((size_t)rows * N);
    std::vector<float> s((size_t)rows * 2);
    const int rc = bertx_test_gemm_rows(fmt, N, K, w_rows, bias, M, rows, x, in_stats, in_g, in_b, epi, res, res_stats,
                                        res_g, res_b, g_next, 0, o.data(), st_out ? s.data() : nullptr, nullptr, cfg);
    if (rc != 0) return rc;
    std::memcpy(out, o.data(), (size_t)M * N * 2);
    if (st_out && g_next) std::memcpy(st_out, s.data(), (size_t)M * 8);
    return 0;
}

extern "C" int32_t bertx_test_gemm_rows(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                        int32_t M, int32_t rows, const uint16_t *x, const float *in_stats,
                                        const float *in_g, const float *in_b, int32_t epi, const uint16_t *res,
                                        const float *res_stats, const float *res_g, const float *res_b,
                                        const float *g_next, int32_t out_of_place, uint16_t *out, float *st_out,
                                        float *part_out, int32_t cfg)
{
    using namespace emb;
    if (!fmt_valid(fmt) || K % 64 || N % 32 || M <= 0 || rows < M || rows % 64 || epi < 0 || epi > 2 || !x || !out ||
        hip_device_count() == 0)
        return -1;
    if (g_next && N > 1024) return -1;   // the statistics kernel combines at most 32 partials per row
    if ((in_stats && (!in_g || !in_b || epi == EPI_BIAS_RES)) || (epi == EPI_BIAS_RES && !res) ||
        (res_stats && (!res_g || !res_b)) || (g_next && epi != EPI_BIAS_RES))
        return -1;
    const int Mp = rows;
    const int PS = Mp + HOOK_GUARD;   // rows of the guarded [row] buffers (and the partials' stride)
    PadFill pf;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    HostTensor t;
    DevWeight W;
    if (!hook_weight(fmt, N, K, w_rows, t, W, B)) return -1;
    LnFold ln;
    const float *dbias = (const float *)B.up(bias, (size_t)N * 4, 0);
    if (in_stats) {
        // the LN fold of the input: c1 = W gamma, c2 = bias + W beta
        const HostTensor hb = vec_tensor(bias, N), hg = vec_tensor(in_g, K), hbt = vec_tensor(in_b, K);
        Piece c1, c2;
        fold_ln({&t}, {&hb}, hg, hbt, c1, c2, fmt == FMT_F32);
        const std::vector<float> hs = padded_stats(in_stats, M, Mp, pf);
        ln.in_stats = (const float2 *)B.up(hs.data(), hs.size() * 4, 0);
        ln.c1 = (const float *)B.up(c1.bytes.data(), c1.bytes.size(), 0);
        dbias = (const float *)B.up(c2.bytes.data(), c2.bytes.size(), 0);
    }
    const std::vector<uint16_t> hx = padded_h16(x, M, Mp, K, pf);
    void *dx = B.up(hx.data(), hx.size() * 2, 0);
    void *dout = nullptr;
    const void *dres = nullptr;
    float2 *dst = nullptr;
    const int NG = N / 32;
    if (epi == EPI_BIAS_RES) {
        const std::vector<uint16_t> hr = padded_h16(res, M, Mp, N, pf);
        if (out_of_place) {
            dres = B.up(hr.data(), hr.size() * 2, 0);
            dout = B.up_ff(nullptr, 0, (size_t)PS * N * 2);
        } else {
            // in place, as the forward runs it
            dout = B.up_ff(hr.data(), hr.size() * 2, (size_t)PS * N * 2);
            dres = dout;
        }
        if (res_stats) {
            const std::vector<float> hs = padded_stats(res_stats, M, Mp, pf);
            ln.res_stats = (const float2 *)B.up(hs.data(), hs.size() * 4, 0);
            ln.res_g = (const float *)B.up(res_g, (size_t)N * 4, 0);
            ln.res_b = (const float *)B.up(res_b, (size_t)N * 4, 0);
        }
        if (g_next) {
            ln.g_next = (const float *)B.up(g_next, (size_t)N * 4, 0);
            ln.part = (float2 *)B.up_ff(nullptr, 0, (size_t)PS * NG * 8);
            ln.part_stride = PS;
            dst = (float2 *)B.up_ff(nullptr, 0, (size_t)PS * 8);
        }
    } else {
        dout = B.up_ff(nullptr, 0, (size_t)PS * N * 2);
    }
    if (B.bad) return -1;
    ScopedSet tile(g_gemm_cfg, cfg);
    const int rc = launch_gemm(W, (const uint16_t *)dx, Mp, dbias, epi, dres, dout, nullptr, ln);
    if (rc != 0) return rc;
    HIP_RC(hipGetLastError());
    HIP_RC(hipDeviceSynchronize());
    if (dst) {
        // the partials as the epilogue left them: every group's guard rows, then the copy
        std::vector<float> hp((size_t)PS * NG * 2);
        HIP_RC(hipMemcpy(hp.data(), ln.part, hp.size() * 4, hipMemcpyDeviceToHost));
        for (int g = 0; g < NG; ++g) {
            const uint8_t *gb = (const uint8_t *)&hp[((size_t)g * PS + Mp) * 2];
            for (size_t i = 0; i < (size_t)HOOK_GUARD * 8; ++i)
                if (gb[i] != 0xff) return -5;
            if (part_out) std::memcpy(part_out + (size_t)g * Mp * 2, &hp[(size_t)g * PS * 2], (size_t)Mp * 8);
        }
        if (launch_ln_stats(ln.part, NG, PS, Mp, N, dst, nullptr) != 0) return -1;
        HIP_RC(hipGetLastError());
        HIP_RC(hipDeviceSynchronize());
        if (st_out) HIP_RC(hipMemcpy(st_out, dst, (size_t)Mp * 8, hipMemcpyDeviceToHost));
        if (const int g = guard_intact(dst + Mp, (size_t)HOOK_GUARD * 8)) return g;
    }
    HIP_RC(hipMemcpy(out, dout, (size_t)Mp * N * 2, hipMemcpyDeviceToHost));
    return guard_intact((const uint16_t *)dout + (size_t)Mp * N, (size_t)HOOK_GUARD * N * 2);
}

extern "C" int32_t bertx_test_gemm_ran(void) { return emb::g_gemm_ran; }

// f32 chain GEMM (f32.hip) on host buffers: w f32 [N][K], x f32 [M][K], res/out f32 [M][N]
extern "C" int32_t bertx_test_gemm_f32(int32_t N, int32_t K, const float *w, const float *bias, int32_t M,
                                       const float *x, int32_t epi, const float *res, float *out)
{
    using namespace emb;
    if (N <= 0 || K % 32 || K <= 0 || M <= 0 || epi < 0 || epi > 2 || (epi == 2 && !res) || hip_device_count() == 0)
        return -1;
    const int Mp = (int)align_up((size_t)M, 64);
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const float *dw = (const float *)B.up(w, (size_t)N * K * 4, 0);
    const float *db = (const float *)B.up(bias, (size_t)N * 4, 0);
    const float *dx = (const float *)B.up(x, (size_t)M * K * 4, (size_t)Mp * K * 4);
    const float *dr = epi == 2 ? (const float *)B.up(res, (size_t)M * N * 4, (size_t)Mp * N * 4) : nullptr;
    float *dout = (float *)B.up(nullptr, 0, (size_t)Mp * N * 4);
    std::vector<uint16_t> tg, te;
    era_tables(tg, te);
    const uint16_t *dg = (const uint16_t *)B.up(tg.data(), tg.size() * 2, 0);
    if (B.bad) return -1;
    if (launch_f32_gemm(dx, Mp, dw, N, K, db, epi, dr, dout, nullptr, dg) != 0) return -1;
    HIP_RC(hipGetLastError());
    HIP_RC(hipDeviceSynchronize());
    HIP_RC(hipMemcpy(out, dout, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// q8-activation chain (q8act.hip): the activation quantizer on host buffers; the
// device's block-major scale planes [K/32][Mp] come back as [M][K/32]
extern "C" int32_t bertx_test_quantize_act(int32_t kind, int32_t M, int32_t K, const float *x, int8_t *q, float *d,
                                           float *s)
{
    using namespace emb;
    if ((kind != 0 && kind != 1) || M <= 0 || K <= 0 || K % 32 || !x || !q || !d || (kind == 1 && !s) ||
        hip_device_count() == 0)
        return -1;
    const int Mp = (int)align_up((size_t)M, 64), nb = K / 32;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const float *dx = (const float *)B.up(x, (size_t)M * K * 4, 0);
    int8_t *dq = (int8_t *)B.up(nullptr, 0, (size_t)Mp * K);
    float *dd = (float *)B.up(nullptr, 0, (size_t)Mp * nb * 4), *ds = (float *)B.up(nullptr, 0, (size_t)Mp * nb * 4);
    if (B.bad) return -1;
    if (launch_q8_quantize(dx, M, Mp, K, kind, dq, dd, ds, nullptr) != 0) return -1;
    HIP_RC(hipGetLastError());
    HIP_RC(hipDeviceSynchronize());
    HIP_RC(hipMemcpy(q, dq, (size_t)M * K, hipMemcpyDeviceToHost));
    std::vector<float> pl((size_t)Mp * nb);
    for (int pass = 0; pass < (kind == 1 ? 2 : 1); ++pass) {
        HIP_RC(hipMemcpy(pl.data(), pass ? ds : dd, pl.size() * 4, hipMemcpyDeviceToHost));
        float *o = pass ? s : d;
        for (int r = 0; r < M; ++r)
            for (int b = 0; b < nb; ++b) o[(size_t)r * nb + b] = pl[(size_t)b * Mp + r];
    }
    return 0;
}

// q8-activation chain: one projection as the forward runs it (quantize, then the
// block-integer GEMM): x f32 [M][K], res / out f32 [M][N]
extern "C" int32_t bertx_test_gemm_q8(int32_t fmt, int32_t N, int32_t K, const void *w_rows, const float *bias,
                                      int32_t M, const float *x, int32_t epi, const float *res, float *out)
{
    using namespace emb;
    if ((fmt != FMT_Q4_0 && fmt != FMT_Q4_1 && fmt != FMT_Q8_0) || K <= 0 || K % 64 || N <= 0 || N % 32 || M <= 0 ||
        epi < 0 || epi > 2 || (epi == 2 && !res) || !w_rows || !bias || !x || !out || hip_device_count() == 0)
        return -1;
    const int Mp = gemm_rows(M), nb = K / 32;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    HostTensor t;
    DevWeight W;
    if (!hook_weight(fmt, N, K, w_rows, t, W, B)) return -1;
    const float *db = (const float *)B.up(bias, (size_t)N * 4, 0);
    const float *dx = (const float *)B.up(x, (size_t)M * K * 4, 0);
    const float *dr = epi == 2 ? (const float *)B.up(res, (size_t)M * N * 4, (size_t)Mp * N * 4) : nullptr;
    float *dout = (float *)B.up(nullptr, 0, (size_t)Mp * N * 4);
    int8_t *dq = (int8_t *)B.up(nullptr, 0, (size_t)Mp * K);
    float *dd = (float *)B.up(nullptr, 0, (size_t)Mp * nb * 4), *ds = (float *)B.up(nullptr, 0, (size_t)Mp * nb * 4);
    std::vector<uint16_t> tg, te;
    era_tables(tg, te);
    const uint16_t *dg = (const uint16_t *)B.up(tg.data(), tg.size() * 2, 0);
    if (B.bad) return -1;
    if (launch_q8_quantize(dx, M, Mp, K, fmt == FMT_Q4_1 ? 1 : 0, dq, dd, ds, nullptr) != 0) return -1;
    if (launch_q8_gemm(W, dq, dd, ds, Mp, db, epi, dr, dout, nullptr, dg) != 0) return -1;
    HIP_RC(hipGetLastError());
    HIP_RC(hipDeviceSynchronize());
    HIP_RC(hipMemcpy(out, dout, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------
// GEMM micro-benchmark (bert_hip.h): device-timed launches on random operands,
// in the forward's own forms (LN fold on the input of epi 0/1; residual with
// its LN, the next gamma and the partial statistics for epi 2)
// ---------------------------------------------------------------------------
extern "C" int32_t bertx_bench_gemm(int32_t fmt, int32_t N, int32_t K, int32_t M, int32_t epi, int32_t cfg,
                                    int32_t iters, float *avg_us)
{
    using namespace emb;
    if (!fmt_valid(fmt) || K % 64 || N % 32 || M <= 0 || iters <= 0 || epi < 0 || epi > 2 ||
        hip_device_count() == 0)
        return -1;
    const int Mp = (int)align_up((size_t)M, GEMM_BM);
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (st >> 8) / 16777216.0f; };
    // random weights in the file format, quantized by the native quantizer's rows
    std::vector<float> wrow((size_t)K);
    std::vector<uint8_t> rows(fmt_row_bytes(fmt, K) * (size_t)N);
    for (int n = 0; n < N; ++n) {
        for (auto &v : wrow) v = (rnd() - 0.5f) * 0.1f;
        quantize_row(fmt, wrow.data(), rows.data() + fmt_row_bytes(fmt, K) * (size_t)n, K);
    }
    std::vector<uint16_t> hx((size_t)Mp * K);
    for (auto &v : hx) v = f32_to_f16(rnd() - 0.5f);
    std::vector<float> hb((size_t)N), hg((size_t)std::max(N, K)), hbt((size_t)std::max(N, K)), hs((size_t)Mp * 2);
    for (auto &v : hb) v = (rnd() - 0.5f) * 0.1f;
    for (auto &v : hg) v = 1.0f + (rnd() - 0.5f) * 0.2f;
    for (auto &v : hbt) v = (rnd() - 0.5f) * 0.1f;
    for (size_t i = 0; i < hs.size(); i += 2) { hs[i] = 0.01f; hs[i + 1] = 1.0f + rnd() * 0.1f; }
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    HostTensor t;
    DevWeight W;
    if (!hook_weight(fmt, N, K, rows.data(), t, W, B)) return -1;
    LnFold ln;
    const float *dbias = (const float *)B.up(hb.data(), hb.size() * 4, 0);
    void *dx = B.up(hx.data(), hx.size() * 2, 0);
    void *dout = B.up(nullptr, 0, (size_t)Mp * N * 2);
    const bool plain = cfg & 0x100;   // A/B: the same GEMM without the LN fold
    cfg &= 0xff;
    if (plain) {
    } else if (epi == EPI_BIAS_RES) {
        ln.res_stats = (const float2 *)B.up(hs.data(), hs.size() * 4, 0);
        ln.res_g = (const float *)B.up(hg.data(), (size_t)N * 4, 0);
        ln.res_b = (const float *)B.up(hbt.data(), (size_t)N * 4, 0);
        ln.g_next = ln.res_g;
        ln.part = (float2 *)B.up(nullptr, 0, (size_t)Mp * (N / 32) * 8);
        ln.part_stride = Mp;
    } else {
        ln.in_stats = (const float2 *)B.up(hs.data(), hs.size() * 4, 0);
        ln.c1 = (const float *)B.up(hg.data(), (size_t)N * 4, 0);
    }
    if (B.bad) return -1;
    ScopedSet tile(g_gemm_cfg, cfg);
    int lrc = 0;
    auto launch = [&]() { lrc |= launch_gemm(W, (const uint16_t *)dx, Mp, dbias, epi, dout, dout, nullptr, ln); };
    for (int i = 0; i < 3; ++i) launch();
    if (lrc != 0) return -1;
    EventPair ev;
    HIP_RC(ev.create());
    HIP_RC(hipEventRecord(ev.a, nullptr));
    for (int i = 0; i < iters; ++i) launch();
    HIP_RC(hipEventRecord(ev.b, nullptr));
    HIP_RC(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIP_RC(hipEventElapsedTime(&ms, ev.a, ev.b));
    *avg_us = ms * 1000.0f / (float)iters;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// attention micro-benchmark (bert_hip.h): n_seqs sentences of `len` tokens,
// random Q/K/V, device-timed launches of variant `variant`
// ---------------------------------------------------------------------------
// n_keys: one key count for every sentence, or 0 for the plain launch
static int32_t bench_attention(int32_t n_seqs, int32_t len, int32_t n_keys, int32_t n_head, int32_t dh,
                               int32_t variant, int32_t iters, float *avg_us)
{
    using namespace emb;
    if (n_seqs <= 0 || len <= 0 || iters <= 0 || hip_device_count() == 0) return -1;
    const int d = n_head * dh;
    const size_t T = (size_t)n_seqs * len, rows = T + 256;
    std::vector<uint16_t> hq(rows * 3 * d);
    uint32_t st = 777u;
    for (auto &v : hq) { st = st * 1664525u + 1013904223u; v = f32_to_f16(((st >> 8) / 16777216.0f - 0.5f) * 2.0f); }
    std::vector<int32_t> hcu((size_t)n_seqs + 1);
    for (int i = 0; i <= n_seqs; ++i) hcu[(size_t)i] = i * len;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const uint16_t *dq = (const uint16_t *)B.up(hq.data(), hq.size() * 2, 0);
    const int32_t *dcu = (const int32_t *)B.up(hcu.data(), hcu.size() * 4, 0);
    uint16_t *dout = (uint16_t *)B.up(nullptr, 0, rows * d * 2);
    const std::vector<int32_t> hk((size_t)n_seqs, n_keys);
    const int32_t *dk = n_keys ? (const int32_t *)B.up(hk.data(), hk.size() * 4, 0) : nullptr;
    if (B.bad) return -1;
    ScopedSet var(g_att_variant, variant);
    for (int i = 0; i < 3; ++i) launch_attention(dq, dcu, n_seqs, len, n_head, d, dout, nullptr, dk);
    EventPair ev;
    HIP_RC(ev.create());
    HIP_RC(hipEventRecord(ev.a, nullptr));
    for (int i = 0; i < iters; ++i) launch_attention(dq, dcu, n_seqs, len, n_head, d, dout, nullptr, dk);
    HIP_RC(hipEventRecord(ev.b, nullptr));
    HIP_RC(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIP_RC(hipEventElapsedTime(&ms, ev.a, ev.b));
    *avg_us = ms * 1000.f / (float)iters;
    return 0;
}

extern "C" int32_t bertx_bench_attention(int32_t n_seqs, int32_t len, int32_t n_head, int32_t dh, int32_t variant,
                                         int32_t iters, float *avg_us)
{
    return bench_attention(n_seqs, len, 0, n_head, dh, variant, iters, avg_us);
}

extern "C" int32_t bertx_bench_attention_kv(int32_t n_seqs, int32_t len, int32_t n_keys, int32_t n_head, int32_t dh,
                                            int32_t variant, int32_t iters, float *avg_us)
{
    if (n_keys < 1 || n_keys > len) return -1;
    return bench_attention(n_seqs, len, n_keys, n_head, dh, variant, iters, avg_us);
}

namespace emb {
namespace {

struct IndexHolder {
    bertx_index *ix = nullptr;
    ~IndexHolder() { bertx_index_free(ix); }
};

// An index of N unit rows on device 0, filled by device-form adds of kFill rows from
// a staging buffer of hashed values, all on stream s; fill_ms (if not null): the adds' device time.
constexpr int64_t kFill = 65536;
int bench_index(int32_t d, int32_t N, int32_t storage, HookBufs &B, IndexHolder &H, hipStream_t s, float *fill_ms)
{
    H.ix = index_create_on(0, d, N, storage);
    if (!H.ix) return -1;
    const int64_t chunk = std::min<int64_t>(kFill, N);
    float *rows = (float *)B.up(nullptr, 0, (size_t)chunk * d * 4);
    if (B.bad) return -1;
    EventPair ev;
    HIP_RC(ev.create());
    float total = 0.f;
    for (int64_t i = 0; i < N; i += chunk) {
        const int64_t m = std::min<int64_t>(chunk, N - i);
        if (launch_unit_rows(rows, m, d, 12345u + (uint32_t)i, s) != 0) return -1;
        HIP_RC(hipEventRecord(ev.a, s));
        if (bertx_index_add_device(H.ix, rows, (int32_t)m, s) < 0) return -1;
        HIP_RC(hipEventRecord(ev.b, s));
        HIP_RC(hipEventSynchronize(ev.b));
        float ms = 0.f;
        HIP_RC(hipEventElapsedTime(&ms, ev.a, ev.b));
        total += ms;
    }
    if (fill_ms) *fill_ms = total;
    return 0;
}

}  // namespace
}  // namespace emb

namespace emb {
namespace {
struct StreamHolder {
    hipStream_t s = nullptr;
    ~StreamHolder()
    {
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    }
};
}  // namespace
}  // namespace emb

extern "C" int32_t bertx_bench_search(int32_t d, int32_t N, int32_t B, int32_t k, int32_t iters, float *avg_us)
{
    return bertx_bench_search_ex(d, N, B, k, BERTX_INDEX_F16, iters, avg_us);
}

extern "C" int32_t bertx_bench_search_ex(int32_t d, int32_t N, int32_t B, int32_t k, int32_t storage, int32_t iters,
                                         float *avg_us)
{
    using namespace emb;
    if (N <= 0 || B <= 0 || iters <= 0 || !avg_us || hip_device_count() == 0) return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs bufs;
    IndexHolder H;
    StreamHolder S;   // destroyed (after a synchronise) before the index and the buffers
    HIP_RC(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
    if (bench_index(d, N, storage, bufs, H, S.s, nullptr) != 0) return -1;
    float *q = (float *)bufs.up(nullptr, 0, (size_t)B * d * 4);
    float *sc = (float *)bufs.up(nullptr, 0, (size_t)B * 128 * 4);
    int32_t *id = (int32_t *)bufs.up(nullptr, 0, (size_t)B * 128 * 4);
    if (bufs.bad || launch_unit_rows(q, B, d, 777u, S.s) != 0) return -1;
    for (int i = 0; i < 3; ++i)
        if (bertx_index_search_device(H.ix, q, B, k, sc, id, S.s) != 0) return -1;
    EventPair ev;
    HIP_RC(ev.create());
    HIP_RC(hipEventRecord(ev.a, S.s));
    for (int i = 0; i < iters; ++i)
        if (bertx_index_search_device(H.ix, q, B, k, sc, id, S.s) != 0) return -1;
    HIP_RC(hipEventRecord(ev.b, S.s));
    HIP_RC(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIP_RC(hipEventElapsedTime(&ms, ev.a, ev.b));
    *avg_us = ms * 1000.f / (float)iters;
    return 0;
}

extern "C" int32_t bertx_bench_search_add_rate(int32_t d, int32_t N, double *add_rows_per_s)
{
    return bertx_bench_search_add_rate_ex(d, N, BERTX_INDEX_F16, add_rows_per_s);
}

extern "C" int32_t bertx_bench_search_add_rate_ex(int32_t d, int32_t N, int32_t storage, double *add_rows_per_s)
{
    using namespace emb;
    if (N <= 0 || !add_rows_per_s || hip_device_count() == 0) return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs bufs;
    IndexHolder H;
    StreamHolder S;
    HIP_RC(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
    float ms = 0.f;
    if (bench_index(d, N, storage, bufs, H, S.s, &ms) != 0 || ms <= 0.f) return -1;
    *add_rows_per_s = (double)N / (ms * 1e-3);
    return 0;
}

extern "C" int32_t bertx_bench_search_rescored(int32_t d, int32_t N, int32_t B, int32_t k, int32_t n_cand, int32_t fine,
                                               int32_t iters, float *avg_us)
{
    using namespace emb;
    if (N <= 0 || B <= 0 || iters <= 0 || !avg_us || k < 1 || k > n_cand || n_cand > 128 || hip_device_count() == 0 ||
        (fine != BERTX_INDEX_F16 && fine != BERTX_INDEX_I8))
        return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs bufs;
    IndexHolder H, F;
    StreamHolder S;   // destroyed (after a synchronise) before the indexes and the buffers
    HIP_RC(hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
    // the same rows in both: bench_index's rows depend on the position alone
    if (bench_index(d, N, BERTX_INDEX_BIN, bufs, H, S.s, nullptr) != 0 || bench_index(d, N, fine, bufs, F, S.s, nullptr) != 0)
        return -1;
    float *q = (float *)bufs.up(nullptr, 0, (size_t)B * d * 4);
    float *sc = (float *)bufs.up(nullptr, 0, (size_t)B * 128 * 4);
    int32_t *id = (int32_t *)bufs.up(nullptr, 0, (size_t)B * 128 * 4);
    float *cs = (float *)bufs.up(nullptr, 0, (size_t)B * 128 * 4);
    int32_t *ci = (int32_t *)bufs.up(nullptr, 0, (size_t)B * 128 * 4);
    if (bufs.bad || launch_unit_rows(q, B, d, 777u, S.s) != 0) return -1;
    EventPair ev;
    HIP_RC(ev.create());
    for (int what = 0; what < 3; ++what) {
        auto call = [&]() -> int32_t {
            if (what == 0) return bertx_index_search_rescored_device(H.ix, F.ix, q, B, k, n_cand, sc, id, S.s);
            if (what == 1) return bertx_index_score_ids_device(F.ix, q, B, ci, n_cand, sc, S.s);
            return bertx_index_search_device(H.ix, q, B, n_cand, cs, ci, S.s);
        };
        // (the ids the scorer is timed on are the binary search's: it runs once before any timing)
        if (what == 0 && bertx_index_search_device(H.ix, q, B, n_cand, cs, ci, S.s) != 0) return -1;
        for (int i = 0; i < 3; ++i)
            if (call() != 0) return -1;
        HIP_RC(hipEventRecord(ev.a, S.s));
        for (int i = 0; i < iters; ++i)
            if (call() != 0) return -1;
        HIP_RC(hipEventRecord(ev.b, S.s));
        HIP_RC(hipEventSynchronize(ev.b));
        float ms = 0.f;
        HIP_RC(hipEventElapsedTime(&ms, ev.a, ev.b));
        avg_us[what] = ms * 1000.f / (float)iters;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Row-kernel parity hooks (norm.hip, f32.hip, table_read.h): one launch over host
// buffers.  The caller's output buffers (out_rows rows, at least the rows the
// kernel writes) are uploaded before the launch and copied back whole after it,
// so a sentinel the caller put there shows which rows the kernel touched.  -1: bad
// arguments or the launcher's own refusal; -3: the launch was refused by the
// runtime (hipGetLastError); -4: the synchronise after it reported an error.
// ---------------------------------------------------------------------------
namespace emb {
namespace {

// launch error / execution error of the launch just made
int hook_finish()
{
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        errorf("libbert: test hook: launch refused: %s\n", hipGetErrorString(le));
        return -3;
    }
    const hipError_t se = hipDeviceSynchronize();
    if (se != hipSuccess) {
        errorf("libbert: test hook: synchronise failed: %s\n", hipGetErrorString(se));
        return -4;
    }
    return 0;
}

// cu[0] == 0, ascending, every sentence of 1 .. max_len tokens
bool hook_cu_ok(const int32_t *cu, int32_t n_seqs, int32_t max_len)
{
    if (!cu || n_seqs <= 0 || max_len <= 0 || cu[0] != 0) return false;
    for (int i = 0; i < n_seqs; ++i)
        if (cu[i + 1] <= cu[i] || cu[i + 1] - cu[i] > max_len) return false;
    return true;
}

// An embedding table from its file-format rows, through repack_table as the engine loads it.
bool hook_table(int32_t fmt, int32_t rows, int32_t cols, const void *bytes, DevTable &T, HookBufs &B)
{
    HostTensor t;
    t.fmt = fmt; t.ne0 = cols; t.ne1 = rows;
    t.bytes.assign((const uint8_t *)bytes, (const uint8_t *)bytes + fmt_row_bytes(fmt, cols) * (size_t)rows);
    Piece q, dd, mm;
    repack_table(t, q, dd, mm);
    T.fmt = fmt; T.rows = rows; T.cols = cols;
    T.qs = B.up(q.bytes.data(), q.bytes.size(), 0);
    T.d = (const uint16_t *)(dd.bytes.empty() ? nullptr : B.up(dd.bytes.data(), dd.bytes.size(), 0));
    T.m = (const uint16_t *)(mm.bytes.empty() ? nullptr : B.up(mm.bytes.data(), mm.bytes.size(), 0));
    return !B.bad;
}

bool hook_width_ok(int32_t d) { return d >= 64 && d <= 1024 && d % 64 == 0; }

}  // namespace
}  // namespace emb

extern "C" int32_t bertx_test_embed_ln(int32_t mode, int32_t fmt_word, int32_t fmt_type, int32_t fmt_pos,
                                       int32_t rows_word, int32_t rows_pos, int32_t d, const void *word_rows,
                                       const void *type_rows, const void *pos_rows, const float *ln_w,
                                       const float *ln_b, const int32_t *ids, const int32_t *cu, int32_t n_seqs,
                                       int32_t max_len, void *out, float *stats, int32_t out_rows)
{
    return bertx_test_embed_ln_types(mode, fmt_word, fmt_type, fmt_pos, rows_word, rows_pos, d, word_rows, type_rows,
                                     pos_rows, ln_w, ln_b, ids, nullptr, cu, n_seqs, max_len, out, stats, out_rows);
}

extern "C" int32_t bertx_test_embed_ln_types(int32_t mode, int32_t fmt_word, int32_t fmt_type, int32_t fmt_pos,
                                             int32_t rows_word, int32_t rows_pos, int32_t d, const void *word_rows,
                                             const void *type_rows, const void *pos_rows, const float *ln_w,
                                             const float *ln_b, const int32_t *ids, const int32_t *types,
                                             const int32_t *cu, int32_t n_seqs, int32_t max_len, void *out,
                                             float *stats, int32_t out_rows)
{
    using namespace emb;
    if (mode < 0 || mode > 2 || !fmt_valid(fmt_word) || !fmt_valid(fmt_type) || !fmt_valid(fmt_pos) ||
        rows_word <= 0 || rows_pos <= 0 || !hook_width_ok(d) || !word_rows || !type_rows || !pos_rows || !ln_w ||
        !ln_b || !ids || !out || (mode == 0 && !stats) || !hook_cu_ok(cu, n_seqs, max_len) || max_len > rows_pos ||
        hip_device_count() == 0)
        return -1;
    const int T = cu[n_seqs];
    if (out_rows < T) return -1;
    for (int t = 0; t < T; ++t)
        if (ids[t] < 0 || ids[t] >= rows_word || (types && types[t] != 0 && types[t] != 1)) return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    DevTable word, type, pos;
    if (!hook_table(fmt_word, rows_word, d, word_rows, word, B) || !hook_table(fmt_type, 2, d, type_rows, type, B) ||
        !hook_table(fmt_pos, rows_pos, d, pos_rows, pos, B))
        return -1;
    const float *dg = (const float *)B.up(ln_w, (size_t)d * 4, 0), *db = (const float *)B.up(ln_b, (size_t)d * 4, 0);
    const int32_t *dids = (const int32_t *)B.up(ids, (size_t)T * 4, 0);
    const int32_t *dcu = (const int32_t *)B.up(cu, ((size_t)n_seqs + 1) * 4, 0);
    const int32_t *dty = types ? (const int32_t *)B.up(types, (size_t)T * 4, 0) : nullptr;
    const size_t ob = (size_t)out_rows * d * (mode == 0 ? 2 : 4);
    void *dout = B.up(out, ob, 0);
    float2 *dst = mode == 0 ? (float2 *)B.up(stats, (size_t)out_rows * 8, 0) : nullptr;
    if (B.bad) return -1;
    if (mode == 0) launch_embed_ln(word, type, pos, dg, dids, dcu, n_seqs, max_len, d, (uint16_t *)dout, dst, nullptr, dty);
    else launch_f32_embed_ln(word, type, pos, dg, db, dids, dcu, n_seqs, max_len, d, (float *)dout, nullptr, mode == 2, dty);
    if (const int rc = hook_finish()) return rc;
    HIP_RC(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
    if (dst) HIP_RC(hipMemcpy(stats, dst, (size_t)out_rows * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int32_t bertx_test_head(const float *x, int32_t n, int32_t d, const float *wp, const float *bp,
                                   const float *wc, const float *bc, int32_t n_labels, float *out, int32_t out_rows)
{
    using namespace emb;
    if (!x || !wp || !bp || !wc || !bc || !out || n <= 0 || out_rows < n || !hook_width_ok(d) || n_labels < 1 ||
        n_labels > HEAD_MAX_LABELS || hip_device_count() == 0)
        return -1;
    constexpr size_t GUARD = 16;   // rows of NaN bits behind the caller's out_rows
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const float *dx = (const float *)B.up(x, (size_t)n * d * 4, 0);
    const float *dwp = (const float *)B.up(wp, (size_t)d * d * 4, 0), *dbp = (const float *)B.up(bp, (size_t)d * 4, 0);
    const float *dwc = (const float *)B.up(wc, (size_t)n_labels * d * 4, 0);
    const float *dbc = (const float *)B.up(bc, (size_t)n_labels * 4, 0);
    const size_t ob = (size_t)out_rows * n_labels * 4, gb = GUARD * n_labels * 4;
    float *dout = (float *)B.up(out, ob, ob + gb);
    float *dp = (float *)B.up(nullptr, 0, ((size_t)n + GUARD) * d * 4);
    if (B.bad) return -1;
    HIP_RC(hipMemset((char *)dout + ob, 0xff, gb));
    HIP_RC(hipMemset(dp, 0xff, ((size_t)n + GUARD) * d * 4));
    const int lrc = launch_head(dx, n, d, dwp, dbp, dwc, dbc, n_labels, dp, dout, nullptr);
    if (const int rc = hook_finish()) return rc;
    if (lrc != 0) return -1;
    HIP_RC(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
    std::vector<uint32_t> g1(GUARD * n_labels), g2(GUARD * d);
    HIP_RC(hipMemcpy(g1.data(), (char *)dout + ob, gb, hipMemcpyDeviceToHost));
    HIP_RC(hipMemcpy(g2.data(), dp + (size_t)n * d, GUARD * d * 4, hipMemcpyDeviceToHost));
    for (const uint32_t v : g1) if (v != 0xffffffffu) return -5;
    for (const uint32_t v : g2) if (v != 0xffffffffu) return -5;   // the pooler stored past row n
    return 0;
}

extern "C" int32_t bertx_test_ln_stats(const float *part, int32_t G, int32_t stride, int32_t rows, int32_t d,
                                       float *stats, int32_t stats_rows)
{
    using namespace emb;
    if (!part || !stats || G <= 0 || G > 64 || rows <= 0 || stride < rows || stats_rows < rows ||
        hip_device_count() == 0)
        return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const float2 *dp = (const float2 *)B.up(part, (size_t)G * stride * 8, 0);
    float2 *dst = (float2 *)B.up(stats, (size_t)stats_rows * 8, 0);
    if (B.bad) return -1;
    const int lrc = launch_ln_stats(dp, G, stride, rows, d, dst, nullptr);
    if (const int rc = hook_finish()) return rc;
    HIP_RC(hipMemcpy(stats, dst, (size_t)stats_rows * 8, hipMemcpyDeviceToHost));
    return lrc;
}

extern "C" int32_t bertx_test_pool(int32_t kind, const uint16_t *z, const float *stats, const float *ln_w,
                                   const float *ln_b, const int32_t *cu, int32_t n_seqs, int32_t max_len, int32_t T,
                                   int32_t d, float *out, int32_t out_rows)
{
    using namespace emb;
    if (kind < 0 || kind > 3 || !z || !stats || !ln_w || !ln_b || !out || T <= 0 || !hook_width_ok(d) ||
        hip_device_count() == 0)
        return -1;
    if (kind == 0 || kind == 1) {
        if (!hook_cu_ok(cu, n_seqs, kind == 0 ? max_len : T) || cu[n_seqs] > T) return -1;
    }
    if (kind == 2 && (n_seqs <= 0 || n_seqs > T)) return -1;
    if (out_rows < (kind == 3 ? T : n_seqs)) return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const uint16_t *dz = (const uint16_t *)B.up(z, (size_t)T * d * 2, 0);
    const float2 *dst = (const float2 *)B.up(stats, (size_t)T * 8, 0);
    const float *dg = (const float *)B.up(ln_w, (size_t)d * 4, 0), *db = (const float *)B.up(ln_b, (size_t)d * 4, 0);
    const int32_t *dcu = kind < 2 ? (const int32_t *)B.up(cu, ((size_t)n_seqs + 1) * 4, 0) : nullptr;
    float *dout = (float *)B.up(out, (size_t)out_rows * d * 4, 0);
    float *dpart = kind == 0 ? (float *)B.up(nullptr, 0, (size_t)n_seqs * pool_chunks(max_len) * d * 4) : nullptr;
    if (B.bad) return -1;
    if (kind == 0) launch_pool_l2(dz, dst, dg, db, dcu, n_seqs, max_len, d, dpart, dout, nullptr);
    else if (kind == 3) launch_tokens_f32(dz, dst, dg, db, T, d, dout, nullptr);
    else launch_cls_l2(dz, dst, dg, db, dcu, n_seqs, d, dout, nullptr);
    if (const int rc = hook_finish()) return rc;
    HIP_RC(hipMemcpy(out, dout, (size_t)out_rows * d * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int32_t bertx_test_f32_rows(int32_t kind, const float *x, const int32_t *cu, int32_t n, int32_t d,
                                       const float *g, const float *b, int32_t flag, float *out, int32_t out_rows)
{
    using namespace emb;
    if (kind < 0 || kind > 2 || !x || !out || n <= 0 || out_rows < n || !hook_width_ok(d) ||
        (kind == 0 && (!g || !b)) || hip_device_count() == 0)
        return -1;
    if (kind != 0 && !hook_cu_ok(cu, n, INT32_MAX)) return -1;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    float *dout = (float *)B.up(out, (size_t)out_rows * d * 4, 0);
    if (kind == 0) {
        // in place over the first n rows of the caller's buffer
        const float *dg = (const float *)B.up(g, (size_t)d * 4, 0), *db = (const float *)B.up(b, (size_t)d * 4, 0);
        if (B.bad) return -1;
        HIP_RC(hipMemcpy(dout, x, (size_t)n * d * 4, hipMemcpyHostToDevice));
        launch_f32_ln(dout, n, d, dg, db, nullptr, flag != 0);
    } else {
        const float *dx = (const float *)B.up(x, (size_t)cu[n] * d * 4, 0);
        const int32_t *dcu = (const int32_t *)B.up(cu, ((size_t)n + 1) * 4, 0);
        if (B.bad) return -1;
        if (kind == 1) launch_f32_pool(dx, dcu, n, d, dout, nullptr, flag != 0);
        else launch_f32_cls(dx, dcu, n, d, dout, nullptr);
    }
    if (const int rc = hook_finish()) return rc;
    HIP_RC(hipMemcpy(out, dout, (size_t)out_rows * d * 4, hipMemcpyDeviceToHost));
    return 0;
}

// host key counts of a hook: each within 1 .. the sentence's length (cu already checked)
static bool hook_keys_ok(const int32_t *keys, const int32_t *cu, int32_t n_seqs)
{
    for (int i = 0; i < n_seqs; ++i)
        if (keys[i] < 1 || keys[i] > cu[i + 1] - cu[i]) return false;
    return true;
}

extern "C" int32_t bertx_test_attention_f32_kv(const float *qkv, const int32_t *cu, const int32_t *keys,
                                               int32_t n_seqs, int32_t max_len, int32_t n_head, int32_t d,
                                               int32_t era, float *out, int32_t out_rows)
{
    using namespace emb;
    if (!qkv || !out || n_head <= 0 || d <= 0 || d % n_head || !hook_cu_ok(cu, n_seqs, max_len) ||
        out_rows < cu[n_seqs] || hip_device_count() == 0)
        return -1;
    if (keys && !hook_keys_ok(keys, cu, n_seqs)) return -1;
    const size_t T = (size_t)cu[n_seqs];
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const float *dq = (const float *)B.up(qkv, T * 3 * d * 4, 0);
    const int32_t *dcu = (const int32_t *)B.up(cu, ((size_t)n_seqs + 1) * 4, 0);
    float *dout = (float *)B.up(out, (size_t)out_rows * d * 4, 0);
    std::vector<uint16_t> tg, te;
    era_tables(tg, te);
    const uint16_t *de = (const uint16_t *)B.up(te.data(), te.size() * 2, 0);
    const int32_t *dk = keys ? (const int32_t *)B.up(keys, (size_t)n_seqs * 4, 0) : nullptr;
    if (B.bad) return -1;
    const int lrc = launch_f32_attention(dq, dcu, n_seqs, max_len, n_head, d, dout, nullptr, de, era != 0, dk);
    if (const int rc = hook_finish()) return rc;
    HIP_RC(hipMemcpy(out, dout, (size_t)out_rows * d * 4, hipMemcpyDeviceToHost));
    return lrc;
}

extern "C" int32_t bertx_test_attention_f32(const float *qkv, const int32_t *cu, int32_t n_seqs, int32_t max_len,
                                            int32_t n_head, int32_t d, int32_t era, float *out, int32_t out_rows)
{
    return bertx_test_attention_f32_kv(qkv, cu, nullptr, n_seqs, max_len, n_head, d, era, out, out_rows);
}

// ---------------------------------------------------------------------------
// The f16 attention kernels (attention.hip, attention_cls.hip).  Every output
// buffer starts as NaN bits (0xffff), so a row the kernel did not write, and a
// write past the rows it owns, both show.
// ---------------------------------------------------------------------------
extern "C" int32_t bertx_test_attention_kv(const uint16_t *qkv, const int32_t *cu, const int32_t *keys,
                                           int32_t n_seqs, int32_t n_head, int32_t d, int32_t variant, uint16_t *out)
{
    using namespace emb;
    if (!qkv || !cu || !out || n_seqs <= 0 || n_head <= 0 || d % n_head || hip_device_count() == 0) return -1;
    const int dh = d / n_head;
    if (dh != 64 && dh != 32) return -1;
    int max_len = 0;
    for (int i = 0; i < n_seqs; ++i) {
        if (cu[i + 1] < cu[i]) return -1;
        max_len = std::max(max_len, cu[i + 1] - cu[i]);
    }
    if (keys && !hook_keys_ok(keys, cu, n_seqs)) return -1;
    const size_t T = (size_t)cu[n_seqs];
    // Rows behind the T packed ones.  qkv: the widest over-read of any kernel
    // launched here is the streaming kernel's, which loads the Q rows of all ATT_QT
    // queries of a tile that holds one query of the last sentence before it masks
    // them, so up to row T + ATT_QT - 2; every other kernel clamps its rows to the
    // sentence (min(row, len - 1)).  The forward's workspace has GEMM_BM + 256 spare
    // rows for the same read.  out: as many sentinel rows, which no kernel may touch.
    constexpr size_t PAD = ATT_QT;
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const uint16_t *dq = (const uint16_t *)B.up(qkv, T * 3 * d * 2, (T + PAD) * 3 * d * 2);
    const int32_t *dcu = (const int32_t *)B.up(cu, ((size_t)n_seqs + 1) * 4, 0);
    uint16_t *dout = (uint16_t *)B.up(nullptr, 0, (T + PAD) * d * 2);
    const int32_t *dk = keys ? (const int32_t *)B.up(keys, (size_t)n_seqs * 4, 0) : nullptr;
    if (B.bad) return -1;
    HIP_RC(hipMemset(dout, 0xff, (T + PAD) * d * 2));
    ScopedSet var(g_att_variant, variant);
    // variant -1: the streaming kernel, reached by claiming a length past the LDS form
    launch_attention(dq, dcu, n_seqs, variant == -1 ? std::max(max_len, ATT_LDS_MAX + 1) : max_len, n_head, d, dout,
                     nullptr, dk);
    if (const int rc = hook_finish()) return rc;
    HIP_RC(hipMemcpy(out, dout, T * d * 2, hipMemcpyDeviceToHost));
    std::vector<uint16_t> pad(PAD * d);
    HIP_RC(hipMemcpy(pad.data(), dout + T * d, pad.size() * 2, hipMemcpyDeviceToHost));
    for (const uint16_t v : pad)
        if (v != 0xffff) return -5;   // a store past the last sentence
    return 0;
}

extern "C" int32_t bertx_test_attention(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs, int32_t n_head,
                                        int32_t d, int32_t variant, uint16_t *out)
{
    return bertx_test_attention_kv(qkv, cu, nullptr, n_seqs, n_head, d, variant, out);
}

extern "C" int32_t bertx_test_attention_ran(void) { return emb::g_att_ran; }

extern "C" int32_t bertx_test_attention_cls_gather(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs,
                                                   int32_t n_head, int32_t d, int32_t Mc, uint16_t *out,
                                                   const uint16_t *z, const float *st, uint16_t *zc, float *stc)
{
    using namespace emb;
    if (!qkv || !cu || !out || n_seqs <= 0 || Mc < n_seqs || n_head <= 0 || d % n_head || hip_device_count() == 0)
        return -1;
    if ((z != nullptr) != (st != nullptr) || (z != nullptr) != (zc != nullptr) || (z != nullptr) != (stc != nullptr))
        return -1;
    const int dh = d / n_head;
    if (dh != 64 && dh != 32) return -1;
    for (int i = 0; i < n_seqs; ++i)
        if (cu[i + 1] < cu[i]) return -1;
    const size_t T = (size_t)cu[n_seqs];
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const uint16_t *dq = (const uint16_t *)B.up(qkv, T * 3 * d * 2, 0);
    const int32_t *dcu = (const int32_t *)B.up(cu, ((size_t)n_seqs + 1) * 4, 0);
    uint16_t *dout = (uint16_t *)B.up(nullptr, 0, (size_t)Mc * d * 2);
    const uint16_t *dz = z ? (const uint16_t *)B.up(z, T * d * 2, 0) : nullptr;
    const float2 *dst = z ? (const float2 *)B.up(st, T * 8, 0) : nullptr;
    uint16_t *dzc = z ? (uint16_t *)B.up(nullptr, 0, (size_t)Mc * d * 2) : nullptr;
    float2 *dstc = z ? (float2 *)B.up(nullptr, 0, (size_t)Mc * 8) : nullptr;
    if (B.bad) return -1;
    // the compact buffers start as NaN bits, so the zeros of the padding rows are the kernel's
    HIP_RC(hipMemset(dout, 0xff, (size_t)Mc * d * 2));
    if (z) {
        HIP_RC(hipMemset(dzc, 0xff, (size_t)Mc * d * 2));
        HIP_RC(hipMemset(dstc, 0xff, (size_t)Mc * 8));
    }
    if (launch_attention_cls(dq, dcu, n_seqs, n_head, d, Mc, dout, dz, dst, dzc, dstc, nullptr) != 0) return -1;
    if (const int rc = hook_finish()) return rc;
    HIP_RC(hipMemcpy(out, dout, (size_t)Mc * d * 2, hipMemcpyDeviceToHost));
    if (z) {
        HIP_RC(hipMemcpy(zc, dzc, (size_t)Mc * d * 2, hipMemcpyDeviceToHost));
        HIP_RC(hipMemcpy(stc, dstc, (size_t)Mc * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int32_t bertx_test_attention_cls(const uint16_t *qkv, const int32_t *cu, int32_t n_seqs, int32_t n_head,
                                            int32_t d, uint16_t *out)
{
    using namespace emb;
    if (!out || n_seqs <= 0 || d <= 0) return -1;
    const int Mc = gemm_rows(n_seqs);
    std::vector<uint16_t> h((size_t)Mc * d);
    if (const int rc = bertx_test_attention_cls_gather(qkv, cu, n_seqs, n_head, d, Mc, h.data(), nullptr, nullptr,
                                                       nullptr, nullptr))
        return rc;
    for (size_t i = (size_t)n_seqs * d; i < h.size(); ++i)
        if (h[i] != 0) return -5;   // a padding row the kernel did not clear
    std::memcpy(out, h.data(), (size_t)n_seqs * d * 2);
    return 0;
}

extern "C" int32_t bertx_test_project(int32_t mode, const void *src, const float *stats, const float *g, const float *b,
                                      int32_t T, int32_t d, const float *W, int32_t dim, const int32_t *rows,
                                      int32_t n_out, float *out, int32_t out_rows)
{
    using namespace emb;
    if ((mode != 0 && mode != 1) || !src || (mode == 0 && (!stats || !g || !b)) || !W || !out || T <= 0 ||
        !hook_width_ok(d) || dim % 32 || dim < kProjMinDim || dim > kProjMaxDim || hip_device_count() == 0)
        return -1;
    if (!rows) n_out = T;
    if (n_out <= 0 || out_rows < n_out) return -1;
    for (int i = 0; rows && i < n_out; ++i)
        if (rows[i] < 0 || rows[i] >= T) return -1;
    constexpr size_t GUARD = 16;   // rows of NaN bits behind the caller's out_rows
    const size_t width = (size_t)proj_width_of(dim);
    std::vector<uint8_t> img;
    build_proj_image(W, dim, d, img);
    DeviceGuard guard(0);
    HIP_RC(guard.status());
    HookBufs B;
    const void *dsrc = B.up(src, (size_t)T * d * (mode == 0 ? 2 : 4), 0);
    const float2 *dst = mode == 0 ? (const float2 *)B.up(stats, (size_t)T * 8, 0) : nullptr;
    const float *dg = mode == 0 ? (const float *)B.up(g, (size_t)d * 4, 0) : nullptr;
    const float *db = mode == 0 ? (const float *)B.up(b, (size_t)d * 4, 0) : nullptr;
    const void *dw = B.up(img.data(), img.size(), 0);
    const int32_t *dr = rows ? (const int32_t *)B.up(rows, (size_t)n_out * 4, 0) : nullptr;
    const size_t ob = (size_t)out_rows * width * 4, gb = GUARD * width * 4;
    float *dout = (float *)B.up(out, ob, ob + gb);
    if (B.bad) return -1;
    HIP_RC(hipMemset((char *)dout + ob, 0xff, gb));
    const int lrc = mode == 0 ? launch_project((const uint16_t *)dsrc, dst, dg, db, nullptr, d, dw, dim, dr, n_out, dout, nullptr)
                              : launch_project(nullptr, nullptr, nullptr, nullptr, (const float *)dsrc, d, dw, dim, dr, n_out,
                                               dout, nullptr);
    if (const int rc = hook_finish()) return rc;
    if (lrc != 0) return -1;
    HIP_RC(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
    std::vector<uint32_t> gd(GUARD * width);
    HIP_RC(hipMemcpy(gd.data(), (char *)dout + ob, gb, hipMemcpyDeviceToHost));
    for (const uint32_t v : gd) if (v != 0xffffffffu) return -5;
    return 0;
}

// Projector micro-benchmark (bert_hip.h): device 0, no context, the f16-chain form.
extern "C" int32_t bertx_bench_project(int32_t d, int32_t dim, int32_t T, int32_t iters, float *avg_us)
{
    using namespace emb;
    if (!hook_width_ok(d) || dim % 32 || dim < kProjMinDim || dim > kProjMaxDim || T < 1 || iters < 1 || !avg_us ||
        hip_device_count() == 0)
        return -1;
    try {
        // hashed operands: z in about [-2, 2), statistics near (0, 1), gamma near 1, W about 1 / sqrt(d)
        auto h01 = [](uint32_t x) {
            x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
            return (float)(x >> 8) * (1.0f / 16777216.0f);
        };
        const size_t width = (size_t)proj_width_of(dim);
        std::vector<uint16_t> z((size_t)T * d);
        for (size_t i = 0; i < z.size(); ++i) z[i] = f32_to_f16(4.0f * h01((uint32_t)i + 1u) - 2.0f);
        std::vector<float> st((size_t)T * 2), gam((size_t)d), bet((size_t)d), W((size_t)dim * d);
        for (int t = 0; t < T; ++t) { st[2 * (size_t)t] = 0.1f * h01(77u + (uint32_t)t); st[2 * (size_t)t + 1] = 0.5f + h01(991u + (uint32_t)t); }
        for (int k = 0; k < d; ++k) { gam[(size_t)k] = 0.75f + 0.5f * h01(5u + (uint32_t)k); bet[(size_t)k] = 0.2f * h01(3001u + (uint32_t)k) - 0.1f; }
        const float ws = 2.0f / std::sqrt((float)d);
        for (size_t i = 0; i < W.size(); ++i) W[i] = ws * (h01(0x9e3779b9u + (uint32_t)i) - 0.5f);
        std::vector<uint8_t> img;
        build_proj_image(W.data(), dim, d, img);
        DeviceGuard guard(0);
        HIP_RC(guard.status());
        HookBufs B;
        const uint16_t *dz = (const uint16_t *)B.up(z.data(), z.size() * 2, 0);
        const float2 *dst = (const float2 *)B.up(st.data(), st.size() * 4, 0);
        const float *dg = (const float *)B.up(gam.data(), gam.size() * 4, 0), *db = (const float *)B.up(bet.data(), bet.size() * 4, 0);
        const void *dw = B.up(img.data(), img.size(), 0);
        float *dout = (float *)B.up(nullptr, 0, (size_t)T * width * 4);
        if (B.bad) return -1;
        struct Ev {
            hipStream_t s = nullptr;
            hipEvent_t a = nullptr, b = nullptr;
            ~Ev()
            {
                if (s) (void)hipStreamSynchronize(s);
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
                if (s) (void)hipStreamDestroy(s);
            }
        } E;
        HIP_RC(hipStreamCreateWithFlags(&E.s, hipStreamNonBlocking));
        HIP_RC(hipEventCreate(&E.a));
        HIP_RC(hipEventCreate(&E.b));
        auto run = [&] { return launch_project(dz, dst, dg, db, nullptr, d, dw, dim, nullptr, T, dout, E.s); };
        for (int i = 0; i < 3; ++i)
            if (run() != 0) return -1;
        HIP_RC(hipEventRecord(E.a, E.s));
        for (int i = 0; i < iters; ++i)
            if (run() != 0) return -1;
        HIP_RC(hipEventRecord(E.b, E.s));
        HIP_RC(hipEventSynchronize(E.b));
        float ms = 0.f;
        HIP_RC(hipEventElapsedTime(&ms, E.a, E.b));
        *avg_us = ms * 1000.f / (float)iters;
        return 0;
    } catch (const std::exception &ex) {
        emb::errorf("bertx_bench_project: %s\n", ex.what());
        return -1;
    }
}
