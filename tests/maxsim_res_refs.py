"""numpy restatement of the residual-coded token store (bert_hip.h "Residual codes";
maxsim_res.hip): the codec (bucket index, the one f16 addition, the exact sum of squares, u),
the canonical bit order, the quantile rule of the bucket trainer, the float64 MaxSim of the
decoded operands with its bound, and the inputs of the accuracy-ordering condition.
Everything stored is restated bit for bit; test_cpu_maxsim_res.py checks the restatement
itself, test_gpu_maxsim_res.py the device against it."""
import numpy as np

import maxsim_refs as M

NBITS = {"res2": 2, "res4": 4}
CENTROID_COUNTS = (16, 48)


# ---- the codec ----
def f16_weights(weights):
    """wt_k = f16(weights[k]), nearest even."""
    return np.asarray(weights, np.float32).astype(np.float16)


def encode(v, c, cutoffs, weights):
    """v, c f32 [n][w] holding f16 values (the twin's rows, the rows' centroids).  Returns
    (b uint8 [n][w], e float16 [n][w], u f32 [n])."""
    v, c = np.asarray(v, np.float32), np.asarray(c, np.float32)
    cut = np.asarray(cutoffs, np.float32)
    r = (v - c).astype(np.float32)                                      # one f32 subtraction
    b = (cut[None, None, :] < r[:, :, None]).sum(axis=2).astype(np.uint8)
    e = decode(c, b, weights)
    return b, e, unit_scale(e)


def decode(c, b, weights):
    """e = c + wt[b]: np.float16 + np.float16 (an f32 sum rounded once more: the same bits as
    one IEEE f16 addition, test_cpu_maxsim_res.py)."""
    return np.asarray(c, np.float32).astype(np.float16) + f16_weights(weights)[np.asarray(b)]


def unit_scale(e):
    """ss exactly (float64; every square is a multiple of 2^-48 and ss < 32), s = f32(ss),
    u = 1 / sqrtf(s): two f32 operations; 0 for ss == 0."""
    e64 = np.asarray(e, np.float16).astype(np.float64)
    ss = (e64 * e64).sum(axis=-1)
    s = ss.astype(np.float32)
    with np.errstate(divide="ignore"):
        u = (np.float32(1.0) / np.sqrt(s).astype(np.float32)).astype(np.float32)
    return np.where(ss > 0, u, np.float32(0.0)).astype(np.float32)


def encode_loops(v, c, cutoffs, weights):
    """The same, restated element by element."""
    v, c = np.asarray(v, np.float32), np.asarray(c, np.float32)
    wt = f16_weights(weights)
    n, w = v.shape
    b = np.zeros((n, w), np.uint8)
    e = np.zeros((n, w), np.float16)
    u = np.zeros(n, np.float32)
    for j in range(n):
        ss = 0.0
        for i in range(w):
            r = np.float32(v[j, i] - c[j, i])
            k = 0
            for cut in cutoffs:
                if np.float32(cut) < r:
                    k += 1
            b[j, i] = k
            e[j, i] = np.float16(np.float16(c[j, i]) + wt[k])
            ss += float(e[j, i]) * float(e[j, i])
        if ss > 0:
            u[j] = np.float32(1.0) / np.float32(np.sqrt(np.float32(ss)))
    return b, e, u


def pack_bits(b, nb):
    """The canonical bytes uint8 [n][w nb / 8]: element i in byte i nb / 8 at bit nb (i mod 8 / nb)."""
    b = np.asarray(b, np.uint8)
    per = 8 // nb
    out = np.zeros((b.shape[0], b.shape[1] // per), np.uint8)
    for j in range(per):
        out |= (b[:, j::per] << np.uint8(nb * j)).astype(np.uint8)
    return out


def unpack_bits(bits, nb):
    bits = np.asarray(bits, np.uint8)
    per = 8 // nb
    out = np.zeros((bits.shape[0], bits.shape[1] * per), np.uint8)
    for j in range(per):
        out[:, j::per] = (bits >> np.uint8(nb * j)) & np.uint8((1 << nb) - 1)
    return out


# ---- the trainer ----
def quantile_rule(residuals, nb):
    """(cutoffs [2^nb - 1], weights [2^nb]) of all residuals, sorted ascending, no interpolation."""
    s = np.sort(np.asarray(residuals, np.float32).reshape(-1))
    n, nw = len(s), 1 << nb
    cut = np.array([s[min(n - 1, k * n // nw)] for k in range(1, nw)], np.float32)
    wts = np.array([s[min(n - 1, (2 * k + 1) * n // (2 * nw))] for k in range(nw)], np.float32)
    return cut, wts


def sample_stride(T):
    return max(1, -(-T // (1 << 16)))


def train_buckets(rows, codes, cent, nb):
    """rows f32 [T][w] (the twin's _doc values in (document, token) order), their codes and
    the twin's _centroid values: the trainer's rule."""
    rows, cent = np.asarray(rows, np.float32), np.asarray(cent, np.float32)
    st = sample_stride(len(rows))
    r = (rows[::st] - cent[np.asarray(codes)[::st]]).astype(np.float32)
    return quantile_rule(r, nb)


# ---- scores ----
def maxsim(q16, e, u):
    """float64 sum_i max_j (q_i . e_j) u_j of the reproducible operands."""
    s = np.asarray(q16, np.float64) @ np.asarray(e, np.float16).astype(np.float64).T
    return float((s * np.asarray(u, np.float64)[None, :]).max(axis=1).sum())


def score_tol(Lq, w):
    """The f16 store's bound (|q16| and |e u| are unit to 2^-10) plus the one extra rounding
    of acc * u, at most 2^-24 for a similarity below 2 in magnitude, once per query row."""
    return M.score_tol(Lq, w) + Lq * 2.0 ** -24


# ---- the accuracy-ordering condition ----
def accuracy_case(w, sigma, seed=0):
    """(cent [16][w], rows [400][w], queries [32][w]): rows are one of 16 random unit centroids
    plus Gaussian noise of norm about sigma, unnormalised; queries are drawn the same way."""
    rng = np.random.default_rng(9000 + w + seed)
    cent = M.unit_rows(rng, 16, w)

    def draw(n):
        x = cent[rng.integers(0, 16, n)] + (sigma / np.sqrt(w)) * rng.standard_normal((n, w))
        return x.astype(np.float32)
    return cent, draw(400), draw(32)


def accuracy_errors(w, sigma):
    """The condition's three figures in float64 numpy for the reference's own codec: mean
    |sim - sim of the unit row| over all (query, row) pairs for RES4, RES2, centroid only.
    Rows, centroids and queries are rounded to f16 as the stores round them; codes are the
    nearest centroid by the exact cosine."""
    cent, rows, queries = accuracy_case(w, sigma)
    v = M.normalise(rows).astype(np.float16).astype(np.float32)
    c16 = M.normalise(cent).astype(np.float16).astype(np.float32)
    q = M.normalise(queries).astype(np.float16).astype(np.float64)
    codes = (v.astype(np.float64) @ c16.astype(np.float64).T).argmax(axis=1)
    c = c16[codes]
    base = q @ v.astype(np.float64).T
    out = []
    for nb in (4, 2):
        cut, wts = quantile_rule(v - c, nb)
        _, e, u = encode(v, c, cut, wts)
        out.append(float(np.abs(q @ (e.astype(np.float64) * u[:, None].astype(np.float64)).T - base).mean()))
    out.append(float(np.abs(q @ c.astype(np.float64).T - base).mean()))
    return tuple(out)
