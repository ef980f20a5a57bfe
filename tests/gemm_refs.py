"""Inputs, float64 references, numpy float32/float16 restatements and per-element error bounds
of the fused-dequant GEMM (gemm.hip through bertx_test_gemm_rows / bertx_test_gemm_fold_rows),
shared by test_gpu_gemm_kernels.py (the kernels against them) and test_cpu_gemm_refs.py (the
restatements against the references, and planted mutations of the restatements against the
bounds, before a GPU is involved).

The weight a kernel multiplies is taken from the file-format bytes (`Weights`): q4_0 f16((q-8) d),
q4_1 f16(q d + m) with one rounding (the packed fma), q8_0 f16(q d), f16 as stored, f32 files
(fmt 0) the pair hi = f16(w), lo = f16(w - hi) as one row of 2K that reads X twice.  The LN-fold
constants c1 = W gamma, c2 = bias + W beta are the host's (repack.cpp fold_ln): summed in double
over f16(the f32 dequantization) -- for q4_1 formally a second rounding the kernel's weight does
not have (`Weights.fold` keeps it; with d and m of like size q d + m is exact in f32, and none of
7e6 quantized random weights differed) -- or over the f32 weight itself for fmt 0.

The bound, counted from the operations and never from the output.  With A the sum of the
magnitudes of every term that enters the f32 value and U = 2^-24,

  |got - ref| <= 2 (Ke + n_epi) U A + half an f16 step at (|ref| + that)

  Ke     the products of one output: K, or 2K for fmt 0.  The order in which an MFMA adds its 32
         products is not established, so every product counts as one addition; the factor 2 allows
         an MFMA that truncates (the convention of attention_refs.py).
  n_epi  the f32 operations of the epilogue (gemm.hip, the `!RES` / `RES` branches):
         plain epi 0/1   v + bias                                                  1
         plain epi 2     z + bias, v + that                                        2
         input LN        st0 = -mean r, fma(st0, c1, c2), fma(r, v, .) and the
                         roundings of c1 (one) and c2 (the sum, then + bias) to f32  6
                         A = |r| sum |z w| + |r mean c1| + sum |w beta| + |bias|
         residual LN     st0, bias + beta, fma(st0, gamma, .), fma(r, z, .), v + . 5
                         A = sum |x w| + |r z| + |r mean gamma| + |beta| + |bias|
         ... * g_next    one more, and the whole f32 part times |g_next|
  The per-group partials of the residual form, (s, q) = (sum, sum (y' - s / 32)^2) of 32 values
  y' each within e = 2 (Ke + 5) U A of its reference: |s - s_ref| <= sum e + 32 U sum |y'|
  (15 additions in the lane, one across the halves); u = y' - s / 32 is within du = e + ds / 32 +
  U |u| of its reference and q within sum (2 |u| du + du^2) + 32 U sum (|u| + du)^2.
  `stats_bound` carries both through ln_row_stats (device_common.h) to (mean, 1/sigma).

At K <= 448 the bound is mostly the f16 step (median bound / |ref| 4e-4 at K 64, 1.2e-3 at K 448);
at K 3072 it is 1.9e-2, so the long K loop is checked by the exact kinds instead: `integers`
(every partial sum a multiple of 1/4 below 2^13, so the f32 sum is exact in any order and the f16
output is known bit for bit) and `onehot` (the output is one weight, bit for bit).
"""
import ctypes
import functools

import numpy as np

F, D, H = np.float32, np.float64, np.float16
U = 2.0 ** -24
LOG2E = 1.4426950408889634

FMTS = {0: "f32", 1: "f16", 2: "q4_0", 3: "q4_1", 8: "q8_0"}
BLOCK = {2: 18, 3: 20, 8: 34}
# the shipped tile configs (gemm.hip): row tile, column tile; two workgroups per CU each
CONFIGS = (2, 3, 4, 11, 16)
ROW_TILE = {2: 256, 11: 256, 3: 128, 4: 64, 16: 64}
COL_TILE = {2: 128, 11: 128, 3: 128, 4: 64, 16: 64}
OCC = 2
KINDS = ("random", "wcol", "xrow")          # plain; one outlier weight column; one scaled X row
N_EPI = {"plain0": 1, "plain2": 2, "inln": 6, "resln": 5}


def half_step_f16(x):
    """Half the f16 spacing at |x| (f64 array), taken at the next f16 value at or above it."""
    x = np.abs(np.asarray(x, D))
    h = x.astype(H)
    h = np.where(h.astype(D) < x, np.nextafter(h, H(np.inf)), h).astype(H)
    return np.spacing(h).astype(D) / 2


def worst_ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, D) - ref) / bound).max())


def f16_ord(h):
    """f16 values as integers in value order (-0 and +0 both 0): differences count f16 steps."""
    b = np.ascontiguousarray(h, H).view(np.int16).astype(np.int32)
    return np.where(b < 0, -(b & 0x7fff), b)


# ---------------------------------------------------------------- weights

def parse_blocks(fmt, wb, N, K):
    """The file blocks of a weight [N][K]: integer values wq [N][K/32][32] as the block dot
    uses them (nibble - 8, nibble, byte), f16 scales wd and mins wm as float64 [N][K/32]."""
    nb = K // 32
    raw = np.frombuffer(wb, np.uint8).reshape(N, nb, BLOCK[fmt])
    wd = raw[:, :, 0:2].copy().view(np.float16)[:, :, 0].astype(np.float64)
    wm = np.zeros((N, nb))
    if fmt == 8:
        wq = raw[:, :, 2:].copy().view(np.int8).astype(np.int64)
    else:
        o = 4 if fmt == 3 else 2
        if fmt == 3:
            wm = raw[:, :, 2:4].copy().view(np.float16)[:, :, 0].astype(np.float64)
        nib = raw[:, :, o:]
        wq = np.concatenate([nib & 15, nib >> 4], axis=2).astype(np.int64) - (8 if fmt == 2 else 0)
    return wq, wd, wm


def build_blocks(fmt, wq, wd, wm=None):
    """The inverse of parse_blocks: file bytes of a weight with chosen integers wq [N][nb][32]
    (the values the dot uses: -8..7, 0..15, -128..127), scales wd and mins wm [N][nb] (f16
    values).  The oracle quantizer cannot be told its scale."""
    N, nb, _ = wq.shape
    raw = np.zeros((N, nb, BLOCK[fmt]), np.uint8)
    raw[:, :, 0:2] = np.ascontiguousarray(wd, H).reshape(N, nb, 1).view(np.uint8)
    if fmt == 8:
        assert wq.min() >= -128 and wq.max() <= 127
        raw[:, :, 2:] = wq.astype(np.int8).view(np.uint8)
    else:
        o = 4 if fmt == 3 else 2
        if fmt == 3:
            raw[:, :, 2:4] = np.ascontiguousarray(wm, H).reshape(N, nb, 1).view(np.uint8)
        nib = (wq + (8 if fmt == 2 else 0)).astype(np.int64)
        assert nib.min() >= 0 and nib.max() <= 15
        raw[:, :, o:] = (nib[:, :, :16] | (nib[:, :, 16:] << 4)).astype(np.uint8)
    return raw.tobytes()


class Weights:
    """A weight [N][K] in file format `fmt`: wb the bytes the hooks take; w float64 [N][Ke] as
    the kernel multiplies it (Ke = K, or the 2K row [hi | lo] of fmt 0); fold float64 [N][K] as
    fold_ln sums it."""

    def __init__(self, fmt, wb, N, K):
        self.fmt, self.wb, self.N, self.K = fmt, wb, N, K
        self.Ke = 2 * K if fmt == 0 else K
        if fmt == 0:
            w32 = np.frombuffer(wb, F).reshape(N, K)
            hi = w32.astype(H)
            lo = (w32 - hi.astype(F)).astype(F).astype(H)
            self.hi, self.lo = hi.astype(D), lo.astype(D)
            self.w = np.concatenate([self.hi, self.lo], axis=1)
            self.fold = w32.astype(D)
        elif fmt == 1:
            self.w = np.frombuffer(wb, H).reshape(N, K).astype(D)
            self.fold = self.w
        else:
            wq, wd, wm = parse_blocks(fmt, wb, N, K)
            v = wq * wd[:, :, None] + wm[:, :, None]              # exact in float64 for f16 d, m of like size
            self.w = v.astype(H).astype(D).reshape(N, K)
            # dequant_row's f32 value, then fold_ln's f16 rounding of it
            self.fold = v.astype(F).astype(H).astype(D).reshape(N, K)

    def x_cols(self, x):
        """X [M][K] as the Ke-long product reads it (twice for fmt 0)."""
        return np.concatenate([x, x], axis=1) if self.fmt == 0 else x

    def value(self):
        """The weight as one number per (n, k): hi + lo for fmt 0."""
        return self.hi + self.lo if self.fmt == 0 else self.w


def weights_from_rows(fmt, W):
    """Random rows W f32 [N][K] in format fmt: the oracle quantizer's bytes for q4_0 / q4_1 / q8_0."""
    N, K = W.shape
    if fmt == 0:
        return Weights(0, np.ascontiguousarray(W, F).tobytes(), N, K)
    if fmt == 1:
        return Weights(1, W.astype(H).tobytes(), N, K)
    import oracle_lib
    L = oracle_lib.lib()
    rows = []
    for n in range(N):
        buf = ctypes.create_string_buffer(K // 32 * BLOCK[fmt])
        x = np.ascontiguousarray(W[n], F)
        L.oracle_quantize_row(fmt, x.ctypes.data, buf, K)
        rows.append(buf.raw)
    return Weights(fmt, b"".join(rows), N, K)


def integer_weights(fmt, N, K, rng):
    """Weights that are multiples of 1/4 (the `integers` kind): q4_0 (q - 8) d, q4_1 q d + m,
    q8_0 q in [-16, 16) times d with d, |m| in {1/4, 1/2, 1}; f16 and f32 multiples of 1/4 in
    [-2, 2]."""
    nb = K // 32
    if fmt in (0, 1):
        W = rng.integers(-8, 9, (N, K)) / 4.0
        return Weights(fmt, W.astype(F if fmt == 0 else H).tobytes(), N, K)
    d = rng.choice([0.25, 0.5, 1.0], (N, nb))
    m = rng.choice([0.25, 0.5, 1.0], (N, nb)) * rng.choice([-1.0, 1.0], (N, nb))
    lo, hi = {2: (-8, 8), 3: (0, 16), 8: (-16, 16)}[fmt]
    q = rng.integers(lo, hi, (N, nb, 32))
    return Weights(fmt, build_blocks(fmt, q, d, m), N, K)


# ---------------------------------------------------------------- inputs

def random_weights(fmt, N, K, rng, kind="random"):
    W = rng.standard_normal((N, K)).astype(F) * F(0.05)
    if kind in ("wcol", "legacy"):
        W[:, 5] *= 20.0                       # an asymmetric outlier column: a transposed map shows
    return weights_from_rows(fmt, W)


def random_x(M, K, rng, kind="random"):
    X = rng.standard_normal((M, K)).astype(F)
    if kind in ("xrow", "legacy") and M > 7:
        X[7] *= 3.0
    return np.ascontiguousarray(X.astype(H))


def ln_stats64(y):
    """ggml_norm's (mean, 1/sigma), eps 1e-5, two passes in float64."""
    y = np.asarray(y, D)
    mean = y.mean(axis=1)
    return mean, 1.0 / np.sqrt(((y - mean[:, None]) ** 2).mean(axis=1) + 1e-5)


def ln_stream(M, d, rng, legacy=False):
    """A LayerNorm'd stream as the forward stores it: rows y, gamma, beta, z = f16(y gamma) and
    the rows' (mean, 1/sigma) as f32 pairs.  No outlier channel: the largest |reference| is not
    inflated, so a relative error on a small output is seen (legacy: the outlier channels of
    test_gpu_kernels.py's LN-fold test, for the comparison with its criterion)."""
    y = rng.standard_normal((M, d)) * 2.0 + rng.standard_normal((M, 1)) * (3.0 if legacy else 1.0)
    g = (1.0 + rng.standard_normal(d) * 0.3).astype(F)
    be = (rng.standard_normal(d) * 0.1).astype(F)
    if legacy:
        y[:, 7] += 80.0
        y[:, 300 % d] -= 150.0
        g[7] = 0.3
    mean, r = ln_stats64(y)
    stats = np.ascontiguousarray(np.stack([mean, r], axis=1), F)
    z = np.ascontiguousarray((y * g).astype(H))
    return y, g, be, z, stats


def group_partials(y):
    """The residual GEMM's partials of rows y [M][32 G] in float32: [G][M][2] (sum, squared
    deviations from the group mean)."""
    M, d = y.shape
    yg = np.asarray(y, F).reshape(M, d // 32, 32)
    sg = yg.sum(axis=2, dtype=F)
    q = ((yg - (sg / F(32))[:, :, None]) ** 2).sum(axis=2, dtype=F)
    return np.ascontiguousarray(np.stack([sg.T, q.T], axis=2), F)


def integer_x(M, K, rng):
    """x in {-1, 0, 1} with P(x != 0) = 1/4."""
    return np.ascontiguousarray((rng.choice([-1.0, 1.0], (M, K)) * (rng.random((M, K)) < 0.25)).astype(H))


def integer_case(fmt, N, K, M, seed, res=False):
    """The `integers` kind: (Weights, x f16, integer bias f32, integer residual f16 or None, the
    exact float64 output).  `integer_condition` is what makes it a bit-for-bit check."""
    rng = np.random.default_rng(seed)
    wt = integer_weights(fmt, N, K, rng)
    x = integer_x(M, K, rng)
    bias = rng.integers(-8, 9, N).astype(F)
    r = np.ascontiguousarray(rng.integers(-63, 64, (M, N)).astype(H)) if res else None
    want = x.astype(D) @ wt.value().T + bias + (r.astype(D) if res else 0.0)
    return wt, x, bias, r, want


# the battery of exact-integer launches: one K-step, one unrolled triple, bge-base's longest loop;
# every launched row count of the small-batch forward (the tile fallbacks among them)
INTEGER_KS = (64, 192, 3072)
INTEGER_ROWS = (64, 128, 192, 256, 320)


def ran_cfg(cfg, rows):
    """pick_cfg's fallbacks for a config asked for by number: a row tile that does not divide the
    launched rows gives way to the next smaller one."""
    if cfg in (2, 11) and rows % 256:
        cfg = 3
    if cfg == 3 and rows % 128:
        cfg = 4
    return cfg


def integer_battery(fmt):
    """(cfg, rows, N, K, res, seed) of every exact-integer launch of format fmt."""
    for cfg in CONFIGS:
        for rows in INTEGER_ROWS:
            for K in INTEGER_KS:
                for res in ((False, True) if K == 64 else (False,)):      # (the epilogue does not depend on K)
                    yield cfg, rows, COL_TILE[cfg] + 32, K, res, ((fmt * 32 + cfg) * 8 + rows // 64) * 8192 + 2 * K + res


def integer_condition(wt, x, bias, r, want):
    """Every term is a multiple of 1/4 and the magnitudes sum below 2^13, so every partial sum in
    any order is exact in f32 (lo is zero for fmt 0); returns the share of outputs with |want| <
    512, where f16 holds every multiple of 1/4 and so hides nothing."""
    v = wt.value()
    assert np.array_equal(v * 4, np.round(v * 4)) and np.array_equal(x.astype(D), np.round(x.astype(D)))
    if wt.fmt == 0:
        assert not wt.lo.any()
    mag = np.abs(x.astype(D)) @ np.abs(v).T + np.abs(bias) + (np.abs(r.astype(D)) if r is not None else 0.0)
    assert mag.max() < 2.0 ** 13, mag.max()
    assert np.abs(want).max() < 65504
    return float(np.mean(np.abs(want) < 512))


def onehot_map(K):
    """pi(m) for M = K rows: rows of the 64-row tile t read the k of tile t + 1 (cyclically),
    reversed inside it on even tiles and rotated by 33 on odd ones: a permutation of 0 .. K-1
    that crosses K-steps, block halves and row tiles."""
    m = np.arange(K)
    t, i = m // 64, m % 64
    T = K // 64
    return 64 * ((t + 1) % T) + np.where(t % 2 == 0, 63 - i, (i + 33) % 64)


def onehot_x(K):
    X = np.zeros((K, K), H)
    X[np.arange(K), onehot_map(K)] = 1.0
    return X


# ---------------------------------------------------------------- references and bounds

def _finish(ref, e):
    return ref, e + half_step_f16(np.abs(ref) + e)


def acc_terms(wt, x):
    """float64 x W^T and sum |x w| over the Ke products [M][N]."""
    xe = wt.x_cols(np.asarray(x, D))
    return xe @ wt.w.T, np.abs(xe) @ np.abs(wt.w).T


def plain_f32(wt, x, bias, res=None):
    """(reference, A, n_epi) of acc + bias (+ res) before the f16 rounding."""
    acc, mag = acc_terms(wt, x)
    b = np.asarray(bias, D)
    if res is None:
        return acc + b, mag + np.abs(b), N_EPI["plain0"]
    r = np.asarray(res, D)
    return acc + b + r, mag + np.abs(b) + np.abs(r), N_EPI["plain2"]


def plain(wt, x, bias, res=None):
    """x W^T + bias (+ res): (reference, bound)."""
    ref, A, n = plain_f32(wt, x, bias, res)
    return _finish(ref, 2 * (wt.Ke + n) * U * A)


def fold_constants(wt, g, be, bias):
    """fold_ln's c1 = W gamma and c2 = bias + W beta in float64, and sum |w beta| + |bias|."""
    g, be, b = np.asarray(g, D), np.asarray(be, D), np.asarray(bias, D)
    return wt.fold @ g, wt.fold @ be + b, np.abs(wt.fold) @ np.abs(be) + np.abs(b)


def input_ln_f32(wt, z, stats, g, be, bias):
    acc, mag = acc_terms(wt, z)
    mean, r = (np.asarray(stats, D)[:, i:i + 1] for i in (0, 1))
    c1, c2, c2mag = fold_constants(wt, g, be, bias)
    return r * (acc - mean * c1) + c2, np.abs(r) * mag + np.abs(r * mean * c1) + c2mag, N_EPI["inln"]


def input_ln(wt, z, stats, g, be, bias):
    """LN(y) W^T + bias as the fold computes it, r (z W^T - mean c1) + c2, on the f16 z and the
    f32 statistics the kernel is given: (reference, bound)."""
    ref, A, n = input_ln_f32(wt, z, stats, g, be, bias)
    return _finish(ref, 2 * (wt.Ke + n) * U * A)


class ResidualLn:
    """The residual form: y' = acc + r z - r mean gamma + beta + bias, out = f16(y' g_next), and
    the per-group partials of y'.  ref / bound [M][N]; s, q, s_bound, q_bound [N/32][M]."""

    def __init__(self, wt, x, bias, z, stats, g, be, gn):
        acc, mag = acc_terms(wt, x)
        mean, r = (np.asarray(stats, D)[:, i:i + 1] for i in (0, 1))
        zz, g, be, b, gn = (np.asarray(a, D) for a in (z, g, be, bias, gn))
        self.y2 = acc + r * zz - r * mean * g + be + b
        A = mag + np.abs(r * zz) + np.abs(r * mean * g) + np.abs(be) + np.abs(b)
        n = N_EPI["resln"]
        self.e = 2 * (wt.Ke + n) * U * A                          # of y' itself
        self.ref, self.bound = _finish(self.y2 * gn, 2 * (wt.Ke + n + 1) * U * A * np.abs(gn))
        M, N = self.y2.shape
        yg, eg = self.y2.reshape(M, N // 32, 32), self.e.reshape(M, N // 32, 32)
        s = yg.sum(axis=2)
        ds = eg.sum(axis=2) + 32 * U * np.abs(yg).sum(axis=2)
        u = yg - s[:, :, None] / 32
        du = eg + ds[:, :, None] / 32 + U * np.abs(u)
        q = (u * u).sum(axis=2)
        dq = (2 * np.abs(u) * du + du * du).sum(axis=2) + 32 * U * ((np.abs(u) + du) ** 2).sum(axis=2)
        self.s, self.q, self.s_bound, self.q_bound = s.T, q.T, ds.T, dq.T

    def stats(self):
        """Two-pass float64 (mean, 1/sigma) of y' [M][2] and the bound on ln_row_stats of
        partials within (s_bound, q_bound): see stats_bound."""
        mean, r = ln_stats64(self.y2)
        return np.stack([mean, r], axis=1), stats_bound(self.s, self.q, self.s_bound, self.q_bound)


def stats_bound(s, q, ds, dq):
    """ln_row_stats on partials [G][M] within (ds, dq) of (s, q): the bound [M][2] on (mean,
    1/sigma) against the exact combination.  mean = (sum_g s_g) / d: G additions and the
    division; dm_g = s_g - 32 mean; m2 = sum_g (dm_g^2 / 32 + q_g); var = m2 / d + eps;
    1/sigma = 1 / sqrt(var): every f32 operation one U of its result."""
    G, M = s.shape
    d = 32.0 * G
    mean = s.sum(axis=0) / d
    dmean = (ds.sum(axis=0) + G * U * np.abs(s).sum(axis=0)) / d + U * np.abs(mean)
    dm = s - 32 * mean
    ddm = ds + 32 * dmean + U * (np.abs(dm) + ds + 32 * dmean)
    term = dm * dm / 32 + q
    dterm = (2 * np.abs(dm) * ddm + ddm * ddm) / 32 + dq + 3 * U * (term + dq + (np.abs(dm) + ddm) ** 2 / 32)
    m2 = term.sum(axis=0)
    dm2 = dterm.sum(axis=0) + G * U * (m2 + dterm.sum(axis=0))
    var = m2 / d + 1e-5
    dvar = dm2 / d + 2 * U * (var + dm2 / d)
    r = 1 / np.sqrt(var)
    dr = r * (0.5 * dvar / (var - dvar) + 4 * U)
    return np.stack([dmean, dr], axis=1)


def ln_row_stats_f32(part, d):
    """ln_row_stats (device_common.h) in numpy float32, op for op: part [G][M][2] -> [M][2]."""
    f = F
    G, M = part.shape[0], part.shape[1]
    s = np.zeros(M, f)
    for g in range(G):
        s = (s + part[g, :, 0]).astype(f)
    mean = (s / f(d)).astype(f)
    m2 = np.zeros(M, f)
    for g in range(G):
        dm = (part[g, :, 0] - (f(32) * mean).astype(f)).astype(f)
        q = (dm * dm).astype(f)
        m2 = (m2 + ((q / f(32)).astype(f) + part[g, :, 1]).astype(f)).astype(f)
    r = (f(1) / np.sqrt(((m2 / f(d)).astype(f) + f(1e-5)).astype(f)).astype(f)).astype(f)
    return np.stack([mean, r], axis=1).astype(f)


# ---------------------------------------------------------------- the GELU epilogue

@functools.lru_cache(maxsize=None)
def era_gelu_table():
    """The era fp16 GELU table over all 65536 f16 inputs, from the oracle (oracle_gelu)."""
    import oracle_lib
    L = oracle_lib.lib()
    xs = np.arange(65536, dtype=np.uint16).view(H).astype(F)
    t = np.array([L.oracle_gelu(float(x)) for x in xs], F).astype(H)
    t.setflags(write=False)
    return t


def gelu_restated(x16, cubic=True, flush_negative=False):
    """gelu2_era / gelu8_era (device_common.h) in numpy f16, operation for operation: x x, the
    packed fma with c1 and c0 (one rounding), times x, exp2, + 1, reciprocal, times x, each
    rounded to f16 once, with a correctly rounded exp2 and reciprocal (the device's are within
    one f16 ulp).  cubic / flush_negative: the planted mutations of test_cpu_gemm_refs.py."""
    k = F(F(-2.0) * F(LOG2E)) * F(0.7978845608028654)
    c0 = D(H(F(k)))
    c1 = D(H(F(F(k) * F(0.044715)))) if cubic else 0.0
    x = np.asarray(x16, H).astype(D)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        t = (x * x).astype(H).astype(D)
        t = (t * c1 + c0).astype(H).astype(D)
        z = (t * x).astype(H).astype(D)
        e = np.exp2(z).astype(H).astype(D)
        d = (e + 1.0).astype(H).astype(D)
        r = (1.0 / d).astype(H).astype(D)
        out = (x * r).astype(H)
    if flush_negative:
        out = np.where(out < 0, H(-0.0), out).astype(H)
    return out


FINITE16 = np.arange(65536, dtype=np.uint16).view(H)
FINITE16 = FINITE16[np.isfinite(FINITE16)]
GELU_FLOOR = 2.0 ** -13                      # below it in |T|: an absolute bound of the same size


def gelu_distance(got, x16):
    """(worst f16 steps from the era table where |T| >= 2^-13, worst |got - T| below that) of
    got = gelu(x16), f16 arrays."""
    T = era_gelu_table()[np.ascontiguousarray(x16, H).view(np.uint16)]
    big = np.abs(T.astype(D)) >= GELU_FLOOR
    steps = np.abs(f16_ord(got) - f16_ord(T))
    err = np.abs(np.asarray(got, D) - T.astype(D))
    return int(steps[big].max(initial=0)), float(err[~big].max(initial=0.0))


# gelu_restated over every finite f16 input against the era table (test_cpu_gemm_refs.py asserts
# these are what the restatement gives): the worst distance in f16 steps where |T| >= 2^-13, and
# the device may be two more per v_exp_f16 / v_rcp_f16 being within one ulp each
GELU_STEPS_RESTATED = 15
GELU_STEPS_DEVICE = GELU_STEPS_RESTATED + 4


def gelu_input_launch():
    """The launch that feeds the GELU epilogue every normal f16 value exactly: f16 weights
    W[n][0] = the n-th mantissa in [1, 2), X row m = +-2^e at k 0 (e = -14 .. 15, 60 rows of 64),
    K = 64, bias 0.  Returns (W f32 [1024][64], X f16 [64][64], acc f16 [64][1024])."""
    W = np.zeros((1024, 64), F)
    W[:, 0] = 1.0 + np.arange(1024) / 1024.0
    X = np.zeros((64, 64), H)
    e = np.arange(-14, 16)
    X[:30, 0] = 2.0 ** e
    X[30:60, 0] = -(2.0 ** e)
    acc = (X[:, :1].astype(D) * W[None, :, 0].astype(D)).astype(H)
    assert np.array_equal(acc.astype(D), X[:, :1].astype(D) * W[None, :, 0])
    return W, X, acc


# ---------------------------------------------------------------- float32 restatement

ORDERS = ("seq", "tree", "block")


def chain_f32(wt, x, order="seq", w=None):
    """The kernel's sum restated in numpy float32: a chain over 32-k blocks in ascending k (for
    fmt 0 the hi half, then the lo half), the 32 exact f16 x f16 products of a block added in one
    of three internal orders -- seq: one by one into the accumulator; tree: pairwise among
    themselves, then into the accumulator; block: exactly, one rounding into the accumulator.
    `w` replaces the weights (the planted mutations)."""
    w = wt.w if w is None else w
    xe = wt.x_cols(np.asarray(x, D))
    M, N = xe.shape[0], w.shape[0]
    acc = np.zeros((M, N), F)
    for b in range(w.shape[1] // 32):
        k = slice(32 * b, 32 * b + 32)
        P = xe[:, None, k] * w[None, :, k]                        # exact: 22-bit products
        if order == "block":
            acc = (acc.astype(D) + P.sum(axis=2)).astype(F)
        elif order == "tree":
            t = P.astype(F)
            while t.shape[2] > 1:
                t = (t[:, :, 0::2] + t[:, :, 1::2]).astype(F)
            acc = (acc + t[:, :, 0]).astype(F)
        else:
            p = P.astype(F)
            for j in range(32):
                acc = (acc + p[:, :, j]).astype(F)
    return acc


def fma32(a, b, c):
    """fmaf on float32 arrays: the float64 product of two f32 is exact, and the double rounding of
    the sum through float64 differs from one rounding only at ties no input here sits on."""
    return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)


def to_f16(v, gelu=False, **mut):
    h = np.asarray(v, F).astype(H)
    return gelu_restated(h, **mut) if gelu else h


def epi_plain(acc, bias, res=None, gelu=False, **mut):
    b = np.asarray(bias, F)[None, :]
    if res is None:
        return to_f16((acc + b).astype(F), gelu, **mut)
    return to_f16((acc + (np.asarray(res, H).astype(F) + b).astype(F)).astype(F))


def fold_f32(wt, g, be, bias):
    """fold_ln's constants as it stores them: c1 rounded to f32; c2 the rounded sum, + bias in
    double, rounded again."""
    c1, _, _ = fold_constants(wt, g, be, bias)
    s2 = (wt.fold @ np.asarray(be, D)).astype(F).astype(D)
    return c1.astype(F), (s2 + np.asarray(bias, D)).astype(F)


def epi_input_ln(wt, acc, stats, g, be, bias, gelu=False, stats_rows=None, **mut):
    """fma(r, acc, fma(st0, c1, c2)), st0 = -mean r.  stats_rows: the row whose statistics each
    row's st0 c1 term uses (the planted mutation; None: its own)."""
    c1, c2 = fold_f32(wt, g, be, bias)
    st = np.asarray(stats, F)
    sr = st[:, 1:2]
    st0 = (-st[:, 0:1] * st[:, 1:2]).astype(F)
    if stats_rows is not None:
        st0 = st0[stats_rows]
    return to_f16(fma32(sr, acc, fma32(st0, c1[None, :], c2[None, :])), gelu, **mut)


def epi_residual_ln(acc, bias, z, stats, g, be, gn, beta=True, gnext_first=False, group_shift=0):
    """The residual form's epilogue: (out f16 [M][N], part f32 [N/32][M][2]).  beta / gnext_first
    / group_shift: the planted mutations."""
    st = np.asarray(stats, F)
    sr = st[:, 1:2]
    st0 = (-st[:, 0:1] * st[:, 1:2]).astype(F)
    bb = (np.asarray(bias, F) + (np.asarray(be, F) if beta else F(0))).astype(F)[None, :]
    v = (acc + fma32(sr, np.asarray(z, H).astype(F), fma32(st0, np.asarray(g, F)[None, :], bb))).astype(F)
    gnf = np.asarray(gn, F)[None, :]
    if gnext_first:
        v = (v * gnf).astype(F)
    M, N = v.shape
    vg = v.reshape(M, N // 32, 32)
    s = np.zeros((M, N // 32), F)
    for j in range(32):
        s = (s + vg[:, :, j]).astype(F)
    mg = (s * F(1.0 / 32.0)).astype(F)
    q = np.zeros((M, N // 32), F)
    for j in range(32):
        u = (vg[:, :, j] - mg).astype(F)
        q = fma32(u, u, q)
    part = np.ascontiguousarray(np.stack([s.T, q.T], axis=2), F)
    if group_shift:
        part = np.roll(part, group_shift, axis=0)
    out = v if gnext_first else (v * gnf).astype(F)
    return out.astype(H), part
