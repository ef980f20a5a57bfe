"""Inputs, float64 references, numpy-float32 restatements and error bounds of the row
kernels (norm.hip, f32.hip, table_read.h), shared by test_gpu_row_kernels.py (the
kernels against them) and test_cpu_row_kernel_refs.py (the restatements against the
references, so every bound is shown reachable before a GPU is involved).

Bounds are per element, c * U * (sum of the magnitudes of the terms that were added),
with c counted from the kernel's operation sequence (written beside each count) and
never from a kernel's output.  U is the f32 unit roundoff 2^-24 times 1.001: the
factor covers the 1 / (1 - c U) of the standard summation bound for every c < 8000.
"""
import ctypes

import numpy as np

import oracle_lib
from test_gpu_kernels import BLOCK, ln_ref, ln_row_stats_f32   # noqa: F401 (re-exported)

F = np.float32
D = np.float64
U = 2.0 ** -24 * 1.001

WIDTHS = [64, 384, 768, 1024]
# the 4- and 8-row workgroup edges of the embed kernels, the 64-token pool chunk and the
# one-launch / two-launch switch at 4 chunks; the last sentence ends inside a workgroup
# of every kernel (257 = 4 * 64 + 1 = 8 * 32 + 1), so a write past it lands on a sentinel row
LENS = [512, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130, 256, 257]
# the 16-query group and the 64-key tile; the last sentence ends inside a 16-query group
ATT_LENS = [512, 1, 15, 16, 17, 63, 64, 65, 130]
FMTS = {0: "f32", 1: "f16", 2: "q4_0", 3: "q4_1", 8: "q8_0"}
POS_ROWS = 520     # more rows than max_len: position rows run 0 .. max_len - 1
WORD_ROWS = 37
SENT = F(-12345.678)          # f32 sentinel
SENT16 = np.float16(777.0)    # f16 sentinel
PAD = 16                      # sentinel rows behind every output


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def ptr(a):
    return None if a is None else a.ctypes.data


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def tie_distance(v):
    """Distance of the f64 values v from the nearest f32 rounding boundary (the midpoint of
    two neighbouring f32 values)."""
    v = np.asarray(v, D)
    f = v.astype(F)
    up = np.nextafter(f, F(np.inf)).astype(D)
    dn = np.nextafter(f, F(-np.inf)).astype(D)
    f = f.astype(D)
    return np.minimum(np.abs(v - (f + up) / 2), np.abs(v - (f + dn) / 2))


def exact_sum(a, axis):
    """Row sums in 80-bit extended precision where the platform has it: their error,
    n * 2^-64 * sum|a|, is 2^-11 of the f64 summation error the tie margins allow for."""
    if np.finfo(np.longdouble).nmant >= 63:
        return a.astype(np.longdouble).sum(axis=axis).astype(D)
    import math
    a = np.moveaxis(np.asarray(a, D), axis, -1)
    return np.array([math.fsum(r) for r in a.reshape(-1, a.shape[-1])]).reshape(a.shape[:-1])


# ---------------------------------------------------------------- tables

def make_table(fmt, rows, d, seed):
    """File-format bytes and the oracle's dequantized f32 values of a random table whose
    every quant block has its own scale (and, q4_1, its own minimum): a wrong block
    index, nibble half or plane offset moves a value by a large multiple of any tolerance."""
    rng = np.random.default_rng(seed)
    nb = d // 32
    scale = rng.uniform(0.25, 4.0, (rows, nb, 1))
    off = rng.uniform(-2.0, 2.0, (rows, nb, 1)) if fmt == 3 else 0.0
    vals = (rng.standard_normal((rows, nb, 32)) * scale + off).reshape(rows, d).astype(F)
    if fmt == 0:
        return vals.tobytes(), vals
    if fmt == 1:
        h = vals.astype(np.float16)
        return h.tobytes(), h.astype(F)
    L = oracle_lib.lib()
    raw = []
    deq = np.zeros((rows, d), F)
    for n in range(rows):
        buf = ctypes.create_string_buffer(nb * BLOCK[fmt])
        L.oracle_quantize_row(fmt, vals[n].ctypes.data, buf, d)
        L.oracle_dequantize_row(fmt, buf, deq[n].ctypes.data, d)
        raw.append(buf.raw)
    return b"".join(raw), deq


def decode_table_f32(fmt, raw, rows, d):
    """The table readers' decode in numpy float32: q * d (+ m), one f32 product and one
    f32 sum (exact: 4- or 8-bit integers times an 11-bit significand)."""
    if fmt == 0:
        return np.frombuffer(raw, F).reshape(rows, d).copy()
    if fmt == 1:
        return np.frombuffer(raw, np.float16).reshape(rows, d).astype(F)
    nb = d // 32
    a = np.frombuffer(raw, np.uint8).reshape(rows, nb, BLOCK[fmt])
    dd = a[:, :, 0:2].copy().view(np.float16).astype(F)                 # [rows][nb][1]
    if fmt == 8:
        q = a[:, :, 2:].copy().view(np.int8).astype(F)
        return (q * dd).astype(F).reshape(rows, d)
    qs = a[:, :, (4 if fmt == 3 else 2):].astype(np.int32)
    # element j < 16: low nibble of byte j; element j >= 16: high nibble of byte j - 16
    q = np.concatenate([qs & 15, qs >> 4], axis=2)
    if fmt == 2:
        return ((q - 8).astype(F) * dd).astype(F).reshape(rows, d)
    mm = a[:, :, 2:4].copy().view(np.float16).astype(F)
    return ((q.astype(F) * dd).astype(F) + mm).astype(F).reshape(rows, d)


class EmbedCase:
    """Three tables, LayerNorm weights, a ragged batch and its ids: row 0, the last row
    and repeated rows of the word table; position rows 0 .. len - 1."""

    def __init__(self, fmts, d, lens=LENS, seed=0):
        self.fmts, self.d, self.lens = fmts, d, list(lens)
        self.cu = cu_of(lens)
        self.T = int(self.cu[-1])
        self.max_len = max(lens)
        rng = np.random.default_rng(1000 + seed)
        rows = (WORD_ROWS, 2, POS_ROWS)
        tabs = [make_table(f, r, d, 7000 + 10 * seed + k) for k, (f, r) in enumerate(zip(fmts, rows))]
        self.raw = [t[0] for t in tabs]
        self.word, self.type, self.pos = (t[1] for t in tabs)
        ids = rng.integers(0, WORD_ROWS, self.T).astype(np.int32)
        ids[self.cu[:-1]] = 0                       # row 0
        ids[self.cu[1:] - 1] = WORD_ROWS - 1        # the last row
        ids[5:9] = 11                               # a repeated row inside one workgroup
        self.ids = ids
        self.pos_idx = np.concatenate([np.arange(n) for n in lens])
        self.g = (1.0 + rng.standard_normal(d) * 0.3).astype(F)
        self.g[7] = F(0.3)
        self.b = (rng.standard_normal(d) * 0.1).astype(F)

    def sum_f32(self):
        """pos + (type[0] + word[id]), each sum one f32 add: the kernels' bits."""
        return (self.pos[self.pos_idx] + (self.type[0][None, :] + self.word[self.ids]).astype(F)).astype(F)

    def as_f32_tables(self):
        """The same values as three f32 tables (the reference of the mixed-format form)."""
        c = EmbedCase.__new__(EmbedCase)
        c.__dict__.update(self.__dict__)
        c.fmts = (0, 0, 0)
        c.raw = [np.ascontiguousarray(t, F).tobytes() for t in (self.word, self.type, self.pos)]
        return c


def embed_z_bits(y, g):
    """z = f16(f32(y) * gamma): one f32 product, one rounding to f16."""
    return bits((y * g[None, :]).astype(F).astype(np.float16))


def embed_stats_f32(y):
    """embed_ln_kernel's statistics in numpy float32, in its order: lane l holds columns
    32 l .. 32 l + 31, sums them in fours, the 32 lanes combine by an xor butterfly."""
    T, d = y.shape
    G = d // 32
    v = np.zeros((T, 32, 32), F)
    v[:, :G, :] = y.reshape(T, G, 32)

    def butterfly(s):
        for o in (16, 8, 4, 2, 1):
            s = (s + s[:, np.arange(32) ^ o]).astype(F)
        return s[:, 0]
    s = np.zeros((T, 32), F)
    for e in range(0, 32, 4):
        s = (s + ((v[:, :, e] + v[:, :, e + 1]) + (v[:, :, e + 2] + v[:, :, e + 3]))).astype(F)
    mean = (butterfly(s) / F(d)).astype(F)
    s2 = np.zeros((T, 32), F)
    for e in range(32):
        u = (v[:, :, e] - mean[:, None]).astype(F)
        u[:, G:] = 0
        s2 = (s2 + u * u).astype(F)
    r = (F(1) / np.sqrt((butterfly(s2) / F(d) + F(1e-5)).astype(F))).astype(F)
    return np.stack([mean, r], axis=1)


def embed_stats_bound(y):
    """Bounds of embed_ln_kernel's (mean, 1/sigma) against ln_ref(y).
    mean: every value passes 2 adds of its group of four, at most 8 adds of the lane's
    running sum, 5 butterfly adds and the division: c = 16 on sum|y| / d.
    1/sigma: the variance is centred on the computed mean, which adds exactly dmean^2; its
    terms carry 2 (the rounded difference, squared) + 1 (the square) + 32 (the lane's running
    sum) + 5 (butterfly) + 1 (division) + 1 (+ eps) = 42 roundings, halved by the square
    root, plus the square root and the reciprocal: c = 21 + 2 = 23, relative."""
    y = y.astype(D)
    d = y.shape[1]
    mean, r = ln_ref(y)
    bm = 16 * U * np.abs(y).sum(axis=1) / d
    var = 1.0 / r ** 2
    return bm, r * (23 * U + 0.5 * bm ** 2 / var)


# ---------------------------------------------------------------- the LN-fold stream

def stream_rows(T, d, rng):
    """Rows as test_gemm_input_ln_fold builds them: a per-row mean of a few units and two
    outlier channels (where r z - r mean gamma + beta cancels)."""
    y = rng.standard_normal((T, d)) * 2.0 + rng.standard_normal((T, 1)) * 3.0
    y[:, 7] += 80.0
    y[:, 300 % d] -= 150.0
    g = (1.0 + rng.standard_normal(d) * 0.3).astype(F)
    g[7] = F(0.3)
    be = (rng.standard_normal(d) * 0.1).astype(F)
    return y, g, be


# two launches (8 chunks), one launch with 4 chunks, one chunk
POOL_BATCHES = ((LENS, 512), ([256, 1, 63, 64, 65, 130, 129, 200], 256), ([64, 1, 3, 17], 64))


class StreamCase:
    """z = f16(y gamma) and the f32 statistics of y for a ragged batch, followed by `pad`
    poisoned rows (a chunk that runs past its sentence's end reads them)."""

    def __init__(self, lens, d, seed, pad=64):
        self.lens, self.d = list(lens), d
        self.cu = cu_of(lens)
        self.T = int(self.cu[-1])
        rng = np.random.default_rng(seed)
        y, self.g, self.b = stream_rows(self.T, d, rng)
        mean, r = ln_ref(y)
        self.z = np.full((self.T + pad, d), 3.0e4, np.float16)
        self.z[:self.T] = (y * self.g).astype(np.float16)
        self.stats = np.full((self.T + pad, 2), 1.0e3, F)
        self.stats[:self.T] = np.stack([mean, r], axis=1)

    def terms(self):
        """LN(y) = r z - r mean gamma + beta in f64 from the values the kernels read, and
        the sum of the magnitudes of its three terms."""
        z = self.z[:self.T].astype(D)
        m, r = self.stats[:self.T, 0].astype(D)[:, None], self.stats[:self.T, 1].astype(D)[:, None]
        g, b = self.g.astype(D), self.b.astype(D)
        return r * z - r * m * g + b, np.abs(r * z) + np.abs(r * m * g) + np.abs(b)


def fma32(a, b, c):
    """fmaf in numpy: the f32 product is exact in f64 (not bit-exact where the f64 sum
    itself rounds, so used for bounds only, never for a bitwise assertion)."""
    return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)


def tokens_f32(case):
    """tokens_f32_kernel / cls_l2_kernel / pool_chunk_sum's per-token value in float32."""
    z = case.z[:case.T].astype(F)
    m, r = case.stats[:case.T, 0:1], case.stats[:case.T, 1:2]
    t0 = (-m * r).astype(F)
    return fma32(r, z, fma32(t0, case.g[None, :], case.b[None, :]))


# every output of these three kernels is fma(r, z, fma(t0, gamma, beta)) with t0 = -mean r:
# three roundings, each of a partial sum of the three terms: c = 3
C_TOKEN = 3


def normalize_bound(p, E, c_n):
    """Bound of o = p / ||p|| when p carries the per-element error E and the norm and the
    division carry c_n relative roundings: |do| <= E / ||p|| + |o| (||E|| / ||p|| + c_n U)."""
    n = np.linalg.norm(p, axis=-1, keepdims=True)
    return E / n + np.abs(p / n) * (np.linalg.norm(E, axis=-1, keepdims=True) / n + c_n * U)


# pool_normalize / cls_l2_kernel: squares (1) + at most 4 adds in the thread + 6 of the wave
# sum + 2 across the waves = 13 on the sum of squares, halved by the square root, + the
# square root + the division: 8.5, rounded up
C_NORM = 9


def pool_counts(d, max_len):
    """Adds a token's value passes in the mean pool: * wt with wt itself rounded (2), the
    thread's running sum over ceil(64 / TT) tokens, TT - 1 adds across the token lanes, and
    one add per chunk."""
    TT = 256 // (d // 8)
    return 2 + -(-64 // TT) + (TT - 1) + -(-max_len // 64)


def pool_ref(case, max_len):
    """f64 mean pool + L2 and its bound, per sentence."""
    v, mag = case.terms()
    c = C_TOKEN + pool_counts(case.d, max_len)
    p = np.stack([v[a:b].mean(axis=0) for a, b in zip(case.cu[:-1], case.cu[1:])])
    A = np.stack([mag[a:b].mean(axis=0) for a, b in zip(case.cu[:-1], case.cu[1:])])
    return p / np.linalg.norm(p, axis=1, keepdims=True), normalize_bound(p, c * U * A, C_NORM)


def pool_f32(case, max_len):
    """launch_pool_l2 in numpy float32 in the kernels' order (pool_chunk_sum, pool_normalize)."""
    v = tokens_f32(case)
    d = case.d
    TT = 256 // (d // 8)
    out = np.zeros((len(case.lens), d), F)
    for s, (a, b) in enumerate(zip(case.cu[:-1], case.cu[1:])):
        n = int(b - a)
        wt = F(1) / F(n)
        x = (v[a:b] * wt).astype(F)
        tot = np.zeros(d, F)
        for i0 in range(0, -(-max_len // 64) * 64, 64):
            i1 = min(n, i0 + 64)
            cs = np.zeros(d, F)
            for tl in range(TT):
                acc = np.zeros(d, F)
                for i in range(i0 + tl, i1, TT):
                    acc = (acc + x[i]).astype(F)
                cs = acc if tl == 0 else (cs + acc).astype(F)
            tot = (tot + cs).astype(F)
        out[s] = tot / np.sqrt(np.sum(tot * tot, dtype=F))
    return out


def cls_ref(case):
    v, mag = case.terms()
    rows = case.cu[:-1]
    return (v[rows] / np.linalg.norm(v[rows], axis=1, keepdims=True),
            normalize_bound(v[rows], C_TOKEN * U * mag[rows], C_NORM))


def cls_f32(case):
    v = tokens_f32(case)[case.cu[:-1]]
    return (v / np.sqrt(np.sum(v * v, axis=1, dtype=F))[:, None]).astype(F)


# ---------------------------------------------------------------- ln_stats

STATS_ROWS = [1, 64, 65, 13 * 64 - 5, 1000, 4096 + 70]
STATS_G = [2, 12, 16, 20, 24, 32]


def stats_parts(rows, G, seed, stride_pad=37):
    """The residual GEMM's partials of `rows` rows of width 32 G, each row with a different
    mean: part [G][stride][2] f32 (stride > rows; the padding holds a poison value)."""
    rng = np.random.default_rng(seed)
    d = 32 * G
    y = rng.standard_normal((rows, d)) * 2.0 + ((np.arange(rows) * 0.6180339887) % 1.0 * 12.0 - 6.0)[:, None]
    y[:, 7] += 80.0
    y[:, 300 % d] -= 150.0
    yg = y.reshape(rows, G, 32)
    sg = yg.sum(axis=2)
    q = ((yg - sg[:, :, None] / 32) ** 2).sum(axis=2)
    part = np.full((G, rows + stride_pad, 2), 1.0e30, F)
    part[:, :rows, 0] = sg.T
    part[:, :rows, 1] = q.T
    return part


def stats_ref(part, rows):
    """Chan's combination of the f32 partials in f64 (the operation ln_row_stats performs;
    = ln_ref of the rows the partials came from) and its bounds.
    mean: G adds and the division: c = G + 1 on sum|s_g| / d =: Em.
    M2 = sum_g t_g, t_g = dm_g^2 / 32 + q_g, dm_g = s_g - 32 mean (one fma): dm_g carries
    32 Em + U |dm_g|, its square twice that times |dm_g| plus (32 Em)^2 plus the square's own
    rounding, the fma U t_g, the G adds G U sum t_g; then / d, + eps (2 roundings, halved by
    the square root), the square root and the reciprocal: 3 U relative on 1/sigma."""
    p = part[:, :rows].astype(D)
    G = p.shape[0]
    d = 32 * G
    s, q = p[:, :, 0], p[:, :, 1]
    mean = s.sum(axis=0) / d
    dm = s - 32 * mean
    t = dm ** 2 / 32 + q
    var = t.sum(axis=0) / d + 1e-5
    r = 1 / np.sqrt(var)
    Em = (G + 1) * U * np.abs(s).sum(axis=0) / d
    E = ((2 * np.abs(dm) * 32 * Em + (32 * Em) ** 2 + 3 * U * dm ** 2) / 32 + U * t).sum(axis=0) + G * U * t.sum(axis=0)
    return np.stack([mean, r], axis=1), np.stack([Em, r * (0.5 * E / d / var + 3 * U)], axis=1)


# ---------------------------------------------------------------- the f32 chain: LayerNorm

def ln_exact_f32(x, g, b):
    """ln_row<EXACT> in numpy: f64 sums, f32 mean, f32 centred values, f32 squares summed in
    f64, f32 variance, 1 / sqrt(var + eps) in f32, then * scale, * gamma, + beta as three
    rounded f32 operations."""
    d = x.shape[1]
    mean = (x.astype(D).sum(axis=1) / d).astype(F)
    c = (x - mean[:, None]).astype(F)
    var = ((c * c).astype(F).astype(D).sum(axis=1) / d).astype(F)
    scale = (F(1) / np.sqrt((var + F(1e-5)).astype(F))).astype(F)
    return ((g[None, :] * (c * scale[:, None]).astype(F)).astype(F) + b[None, :]).astype(F)


def sum_tie_ratio(a, axis, div):
    """How safely the f32 rounding of (f64 sum of the f32 values a along axis) / div is the
    same for every summation order: inf where the sum is exact in any order (every value is
    a multiple of the row's smallest ulp q and sum|a| < 2^53 q, so every partial sum is
    representable), else the quotient's distance from an f32 rounding boundary over margin.
    An f64 sum of n terms is within n 2^-53 sum|a| of the exact one in any order (n 2^-63
    more for the extended-precision sum standing in for the exact one here) and the f64
    division adds 2^-53 relative: margin = n (2^-53 + 2^-63) sum|a| / div + 2^-52 |quotient|.
    A ratio > 1 means no tie."""
    a = np.asarray(a, F)
    n = a.shape[axis]
    mag = np.abs(a).astype(D).sum(axis=axis)
    q = np.where(a != 0, np.spacing(np.abs(a)), F(np.inf)).astype(D).min(axis=axis)
    v = exact_sum(a, axis) / div
    margin = n * (2.0 ** -53 + 2.0 ** -63) * mag / div + 2.0 ** -52 * np.abs(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mag < 2.0 ** 53 * q, np.inf, tie_distance(v) / margin), v


def ln_tie_ok(x):
    """The smallest sum_tie_ratio of ln_exact_f32's two f64 -> f32 roundings (the mean, and
    the variance given that mean) over the rows: > 1 means the restatement's bits do not
    depend on the order of the f64 sums."""
    d = x.shape[1]
    rm, m64 = sum_tie_ratio(x, 1, d)
    c = (x - m64.astype(F)[:, None]).astype(F)
    rv, _ = sum_tie_ratio((c * c).astype(F), 1, d)
    return min(rm.min(), rv.min())


def ln_ref_bound(x, g, b):
    """f64 LayerNorm and the bound of ln_row (either form).  With c = x - mean, r = 1/sigma:
    the f32 mean is off by U |mean| (its f64 sum by d 2^-53 sum|x| / d more), which moves
    every output by |gamma| r times that; c itself rounds once (1); the variance carries 2
    (c, squared) + 1 (the square) + 1 (to f32) + 1 (+ eps) = 5, halved, + the square root +
    the reciprocal = 4.5 on the scale; * scale and * gamma round once each (2): c = 7.5,
    rounded up to 8, on |gamma c r|; the final sum rounds once on |out|, at most
    |gamma c r| + |beta|."""
    x = x.astype(D)
    d = x.shape[1]
    mean, r = ln_ref(x)
    t = g.astype(D) * (x - mean[:, None]) * r[:, None]
    dm = U * np.abs(mean) + 2.0 ** -53 * np.abs(x).sum(axis=1)
    bound = np.abs(g.astype(D)) * (r * dm)[:, None] + 8 * U * np.abs(t) + U * (np.abs(t) + np.abs(b.astype(D)))
    return t + b.astype(D), bound


F32_LN_ROWS = 131


def f32_ln_case(d, seed=0):
    rng = np.random.default_rng(4000 + d + seed)
    y, g, b = stream_rows(F32_LN_ROWS, d, rng)
    return y.astype(F), g, b


# ---------------------------------------------------------------- the f32 chain: attention

_EXP = None


def era_exp_table():
    """The era fp16 exp table over all 65536 f16 inputs, from the oracle (oracle_exp), as
    era_gelu_table of test_gpu_kernels.py builds the GELU one."""
    global _EXP
    if _EXP is None:
        L = oracle_lib.lib()
        xs = np.arange(65536, dtype=np.uint16).view(np.float16).astype(F)
        _EXP = np.array([L.oracle_exp(float(x)) for x in xs], F).astype(np.float16)
    return _EXP


def attention_case(dh, lens=ATT_LENS, seed=0, n_head=2):
    """qkv f32 [T][3d]; the second-to-last sentence has sharp scores (Q x 4, keys growing
    along the sentence), as the f16 attention tests have."""
    d = n_head * dh
    cu = cu_of(lens)
    rng = np.random.default_rng(5000 + dh + seed)
    qkv = rng.standard_normal((int(cu[-1]), 3 * d)).astype(F)
    s0, s1 = cu[-3], cu[-2]
    qkv[s0:s1, :d] *= F(4.0)
    qkv[s0:s1, d:2 * d] *= np.linspace(0.2, 3.0, s1 - s0).astype(F)[:, None]
    return qkv, cu, n_head, d


def heads(qkv, cu, n_head, d):
    dh = d // n_head
    for s in range(len(cu) - 1):
        a, b = int(cu[s]), int(cu[s + 1])
        for h in range(n_head):
            c = slice(h * dh, (h + 1) * dh)
            yield a, b, c, qkv[a:b, c], qkv[a:b, d:2 * d][:, c], qkv[a:b, 2 * d:][:, c]


def attention_ref(qkv, cu, n_head, d):
    """f64 attention with the era softmax of f32.hip (row max, T(f16(s - max)), f64 sum,
    times 1 / sum) and its bound.
    Scores: an f32 chain of dh multiply-adds and the scale: c = dh + 1 on scale sum|q k| =:
    ds.  The argument a = s - max carries ds, the largest ds of its row (the max is taken
    over computed scores) and the difference's own rounding U |a|; both sides round it to an
    f16 table input, one input step apart at most: Da = da + ulp16(a).  The table's slope is
    exp <= exp(a + Da), and both entries are rounded to f16: de = exp(a + Da) Da + ulp16(e).
    p = e / sum: dp = de / sum + p (sum(de) / sum + 2 U) (the f32 reciprocal and the product).
    P V: an f32 chain of len multiply-adds: c = len on sum_k |p v|, plus sum_k dp |v|."""
    table = era_exp_table()
    dh = d // n_head
    out = np.zeros((qkv.shape[0], d), D)
    bound = np.zeros_like(out)
    for a, b, c, q, k, v in heads(qkv.astype(D), cu, n_head, d):
        n = b - a
        s = q @ k.T / np.sqrt(dh)
        ds = (dh + 1) * U * (np.abs(q) @ np.abs(k).T) / np.sqrt(dh)
        arg = s - s.max(axis=1, keepdims=True)
        da = ds + ds.max(axis=1, keepdims=True) + U * np.abs(arg)
        a16 = arg.astype(np.float16)
        Da = da + np.spacing(np.abs(a16)).astype(D)
        e = table[a16.view(np.uint16)].astype(D)
        de = np.exp(arg + Da) * Da + np.spacing(table[a16.view(np.uint16)]).astype(D)
        sm = e.sum(axis=1, keepdims=True)
        p = e / sm
        dp = de / sm + p * (de.sum(axis=1, keepdims=True) / sm + 2 * U)
        out[a:b, c] = p @ v
        bound[a:b, c] = dp @ np.abs(v) + n * U * (p @ np.abs(v))
    return out, bound


def era_lanes_sum(la):
    """((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) over axis -1, f32."""
    return (((la[..., 0] + la[..., 1]) + (la[..., 2] + la[..., 3])) +
            ((la[..., 4] + la[..., 5]) + (la[..., 6] + la[..., 7]))).astype(F)


def attention_era_f32(qkv, cu, n_head, d):
    """f32_attention_kernel<DH, true> in numpy float32, bit for bit: both dot products in
    the oracle's dot_f32 order (eight lanes i & 7, the product and the sum rounded
    separately, a pairwise horizontal sum); padded keys of P V add exact zeros."""
    table = era_exp_table()
    dh = d // n_head
    scale = F(1) / np.sqrt(F(dh))
    out = np.zeros((qkv.shape[0], d), F)
    for a, b, c, q, k, v in heads(qkv, cu, n_head, d):
        n = b - a
        la = np.zeros((n, n, 8), F)
        for e in range(0, dh, 8):
            la = (la + (k[None, :, e:e + 8] * q[:, None, e:e + 8]).astype(F)).astype(F)
        s = (era_lanes_sum(la) * scale).astype(F)
        arg = (s - s.max(axis=1, keepdims=True)).astype(F).astype(np.float16)
        e16 = table[arg.view(np.uint16)]
        inv = (1.0 / e16.astype(D).sum(axis=1, keepdims=True)).astype(F)      # (exact in any order)
        p = (e16.astype(F) * inv).astype(F)
        n8 = -(-n // 8) * 8
        pp = np.zeros((n, n8), F)
        pp[:, :n] = p
        vv = np.zeros((n8, dh), F)
        vv[:n] = v
        ol = np.zeros((n, dh, 8), F)
        for k0 in range(0, n8, 8):
            ol = (ol + (vv[k0:k0 + 8].T[None, :, :] * pp[:, None, k0:k0 + 8]).astype(F)).astype(F)
        out[a:b, c] = era_lanes_sum(ol)
    return out


# ---------------------------------------------------------------- the f32 chain: pool, CLS

def f32_pool_case(d, lens=LENS, seed=0):
    cu = cu_of(lens)
    rng = np.random.default_rng(6000 + d + seed)
    y, _, _ = stream_rows(int(cu[-1]), d, rng)
    return y.astype(F), cu


def f32_pool_ref(x, cu):
    """f64 mean pool + L2 and the bound of f32_pool_kernel (either order): wt = 1 / len
    rounds once and every token passes at most len multiply-adds: c = len + 1 on
    sum|x| wt.  The norm: the squares round once, the f64 sum to f32 once, both halved by the
    square root, + the square root + the division: c = 3."""
    x = x.astype(D)
    p = np.stack([x[a:b].mean(axis=0) for a, b in zip(cu[:-1], cu[1:])])
    A = np.stack([(b - a + 1) * U * np.abs(x[a:b]).mean(axis=0) for a, b in zip(cu[:-1], cu[1:])])
    return p / np.linalg.norm(p, axis=1, keepdims=True), normalize_bound(p, A, 3)


def f32_pool_era_f32(x, cu):
    """f32_pool_kernel<true> in numpy float32, bit for bit: the token sum in dot_f32's order
    (lane = token & 7), the sum of squares in f64.  Also returns, per sentence, the f64 sum
    of squares' sum_tie_ratio: > 1 means its f32 rounding does
    not depend on the summation order."""
    d = x.shape[1]
    out = np.zeros((len(cu) - 1, d), F)
    tie = np.zeros(len(cu) - 1)
    for s, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        n = int(b - a)
        wt = F(1) / F(n)
        n8 = -(-n // 8) * 8
        xx = np.zeros((n8, d), F)
        xx[:n] = (x[a:b] * wt).astype(F)
        la = np.zeros((d, 8), F)
        for i in range(0, n8, 8):
            la = (la + xx[i:i + 8].T).astype(F)
        acc = era_lanes_sum(la)
        sq = (acc * acc).astype(F)
        tie[s] = sum_tie_ratio(sq, 0, 1)[0]
        out[s] = acc / np.sqrt(F(sq.astype(D).sum()))
    return out, tie


def f32_cls_ref(x, cu):
    """f64 x[cu[b]] / ||.||; the kernel rounds the norm as f32_pool_kernel does and
    divides: c = 3 + 1, relative."""
    v = x.astype(D)[cu[:-1]]
    o = v / np.linalg.norm(v, axis=1, keepdims=True)
    return o, 4 * U * np.abs(o)


def f32_cls_f32(x, cu):
    v = x[cu[:-1]]
    return (v / np.sqrt((v * v).astype(F).astype(D).sum(axis=1).astype(F))[:, None]).astype(F)


def worst(err, bound):
    """max error / bound (bounds are positive wherever an error can be)."""
    err, bound = np.asarray(err, D), np.asarray(bound, D)
    return float(np.max(err / np.maximum(bound, 1e-300)))
