"""numpy reference of the token store and its MaxSim scorer (bertx_mvindex_*, bert_hip.h):
the normaliser, the f16 view of a row, float64 MaxSim, the two tolerances of the
contract, an f32 emulation of the device arithmetic, and the fixed inputs the GPU tests
use (test_gpu_maxsim.py), so that test_cpu_maxsim_refs.py can check those very inputs."""
import numpy as np

WIDTHS = (64, 192, 768)
QUERY_LENS = (1, 16, 17, 64)
DOC_LENS = (1, 15, 16, 17, 31, 32, 33, 100, 512)
PACK_LENS = (1, 15, 16, 17, 33)


# ---- the contract's arithmetic ----
def normalise(x):
    """float64 x / |x| per row; a zero row stays zero."""
    x = np.asarray(x, np.float64)
    n = np.sqrt((x * x).sum(axis=-1, keepdims=True))
    return np.divide(x, n, out=np.zeros_like(x), where=n > 0)


def f16_view(x):
    """An f32 emulation of the stored row: ss summed sequentially in f32, rinv = 1 / sqrt(ss)
    as two f32 operations, f16(x * rinv); returned as f32.  (The device sums in another
    order; both are inside elem_tol.)"""
    x = np.asarray(x, np.float32)
    sq = x * x
    ss = np.zeros(x.shape[:-1], np.float32)
    for i in range(x.shape[-1]):
        ss = (ss + sq[..., i]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rinv = (np.float32(1.0) / np.sqrt(ss).astype(np.float32)).astype(np.float32)
    rinv = np.where(ss > 0, rinv, np.float32(0.0)).astype(np.float32)
    return (x * rinv[..., None]).astype(np.float32).astype(np.float16).astype(np.float32)


def maxsim(q16, doc16):
    """float64 sum_i max_j <q_i, c_j> of the f16 values q16 [Lq][w], doc16 [len][w]."""
    s = np.asarray(q16, np.float64) @ np.asarray(doc16, np.float64).T
    return float(s.max(axis=1).sum())


def maxsim_loops(q16, doc16):
    """The same, restated as three loops."""
    q16, doc16 = np.asarray(q16, np.float64), np.asarray(doc16, np.float64)
    total = 0.0
    for i in range(len(q16)):
        best = -np.inf
        for j in range(len(doc16)):
            dot = 0.0
            for k in range(q16.shape[1]):
                dot += q16[i, k] * doc16[j, k]
            best = max(best, dot)
        total += best
    return total


def maxsim_f32(q16, doc16):
    """An f32 emulation of the scorer: per (i, j) an f32 accumulator over ascending blocks
    of 32 elements (each block's dot taken in f32), the exact max, a sequential f32 sum."""
    q, c = np.asarray(q16, np.float32), np.asarray(doc16, np.float32)
    acc = np.zeros((len(q), len(c)), np.float32)
    for k in range(0, q.shape[1], 32):
        acc = (acc + (q[:, k:k + 32] @ c[:, k:k + 32].T).astype(np.float32)).astype(np.float32)
    s = np.float32(0.0)
    for v in acc.max(axis=1):
        s = np.float32(s + v)
    return float(s)


def elem_tol(v, w):
    """|stored - v| bound per element for the exact v = x_i / |x|: the f16 half-ulp, the f32
    norm, the subnormal spacing."""
    return np.abs(np.asarray(v, np.float64)) * (2.0 ** -11 + (w + 8) * 2.0 ** -24) + 2.0 ** -24


def score_tol(Lq, w):
    """|score - float64 MaxSim of the stored f16 values| bound: 2 w 2^-24 per similarity of
    unit vectors plus the f32 sum of Lq terms of magnitude <= 1."""
    return Lq * (2.0 * w + Lq) * 2.0 ** -24


# ---- inputs ----
def token_rows(rng, n, w):
    """n un-normalised token rows: normal values, each row scaled by 1e-3, 1 or 30, with
    three channels 20 times larger."""
    x = rng.standard_normal((n, w)).astype(np.float32)
    x[:, [1, w // 2, w - 1]] *= np.float32(20.0)
    scale = np.array([1e-3, 1.0, 30.0], np.float32)[rng.integers(0, 3, n)]
    return x * scale[:, None]


def unit_rows(rng, n, w):
    x = rng.standard_normal((n, w)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def pack_case(w):
    """Documents of PACK_LENS token rows; document 2 has a zero row at index 7."""
    rng = np.random.default_rng(1000 + w)
    docs = [token_rows(rng, n, w) for n in PACK_LENS]
    docs[2][7] = 0.0
    return docs


def parity_case(w):
    """(docs of DOC_LENS rows, {Lq: query rows}) of the score parity test."""
    rng = np.random.default_rng(2000 + w)
    docs = [token_rows(rng, n, w) for n in DOC_LENS]
    queries = {Lq: token_rows(rng, Lq, w) for Lq in QUERY_LENS}
    return docs, queries


def orthogonal_to(rng, n, basis):
    """n unit rows orthogonal to every row of basis (float64 Gram-Schmidt, then f32)."""
    b = np.linalg.qr(np.asarray(basis, np.float64).T)[0].T
    x = rng.standard_normal((n, basis.shape[1]))
    x -= (x @ b.T) @ b
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def planted_last(w, n):
    """(q [1][w], doc [n][w]): rows 0 .. n - 2 are orthogonal to the query, row n - 1 is the
    query itself: the score is 1 when the last row of the partly filled group counts and
    about 0 when it does not."""
    rng = np.random.default_rng(3000 + w + n)
    q = unit_rows(rng, 1, w)
    doc = np.concatenate([orthogonal_to(rng, n - 1, q), q])
    return q, doc


def planted_negative(w, Lq):
    """(q [Lq][w], doc [5][w]): every query token is one unit vector v and every document
    token is -v: each similarity is -1 and the score -Lq, where padding rows counted as 0
    would give 0."""
    rng = np.random.default_rng(4000 + w + Lq)
    v = unit_rows(rng, 1, w)
    return np.repeat(v, Lq, axis=0), np.repeat(-v, 5, axis=0)


RANKING_CASES = [(64, 5, 24, 0), (192, 17, 40, 1), (768, 32, 30, 2)]   # (w, Lq, N, seed)


def ranking_corpus(w, Lq, N, seed):
    """(q [Lq][w], docs, order): document `order[r]` is the r-th best.  The r-th best holds,
    for every query token q_i, a row a_r q_i + sqrt(1 - a_r^2) u (u a unit row orthogonal to
    all query tokens), a_r = 0.9 - 0.02 r, among 1 .. 40 rows orthogonal to the query, at
    random places; lengths are ragged.  Scores are about Lq a_r, 0.02 Lq apart."""
    rng = np.random.default_rng(5000 + seed)
    q = np.linalg.qr(rng.standard_normal((w, Lq)))[0].T.astype(np.float32)   # orthonormal query tokens
    order = rng.permutation(N)
    docs = [None] * N
    for r, d in enumerate(order):
        a = 0.9 - 0.02 * r
        u = orthogonal_to(rng, Lq, q)
        good = (a * q + np.sqrt(1.0 - a * a) * u).astype(np.float32)
        rows = np.concatenate([good, orthogonal_to(rng, int(rng.integers(1, 41)), q)])
        docs[d] = rows[rng.permutation(len(rows))] * np.float32(rng.uniform(0.5, 2.0))
    return q, docs, order


def min_gap(scores):
    s = np.sort(np.asarray(scores, np.float64))
    return float(np.diff(s).min())
