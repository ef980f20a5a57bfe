"""References and the checker of the embedding-index search tests (bertx_index_*).

Reference scores: the float64 dot of float16(query) (numpy, round to nearest even)
with the stored rows as bertx_index_rows returns them (exact f16 values).  Products
of two f16 values are exact in f32, so a device score differs from the reference only
by the f32 accumulation of d terms with sum |q_i c_i| <= |q| |c|: first order
d 2^-24 |q| |c|; the tests allow twice that (the MFMA's internal order and rounding).
"""
import numpy as np


def ref_scores(queries, stored_rows):
    """float64 [B][N]: float16(queries) . stored_rows."""
    q16 = np.asarray(queries, np.float32).astype(np.float16).astype(np.float64)
    return q16 @ np.asarray(stored_rows, np.float64).T


def tolerances(queries, stored_rows):
    """Per query: 2 d 2^-24 |q16| max_i |c_i|."""
    q16 = np.asarray(queries, np.float32).astype(np.float16).astype(np.float64)
    c = np.asarray(stored_rows, np.float64)
    d = q16.shape[1]
    cmax = np.sqrt((c * c).sum(axis=1)).max() if len(c) else 0.0
    return 2.0 * d * 2.0 ** -24 * np.sqrt((q16 * q16).sum(axis=1)) * cmax


def check_topk(ref, scores, ids, k, tol):
    """One query's result against its reference scores ref [N]; excludes no case.
    Raises AssertionError with the first violation."""
    ref = np.asarray(ref, np.float64)
    scores = np.asarray(scores)
    ids = np.asarray(ids)
    N = len(ref)
    assert scores.shape == (k,) and ids.shape == (k,), (scores.shape, ids.shape, k)
    nv = min(k, N)
    got = ids[:nv].astype(np.int64)
    assert np.all((got >= 0) & (got < N)), ("id out of range", ids)
    assert len(set(got.tolist())) == nv, ("duplicate id", ids)
    assert np.all(ids[nv:] == -1) and np.all(np.isneginf(scores[nv:])), ("missing (-1, -inf) fill", ids, scores)
    s = scores[:nv].astype(np.float64)
    for j in range(nv - 1):
        assert s[j] >= s[j + 1], ("scores not descending", j, s[j], s[j + 1])
        assert s[j] != s[j + 1] or got[j] < got[j + 1], ("equal scores not by ascending id", j, got[j], got[j + 1])
    err = np.abs(s - ref[got])
    assert np.all(err <= tol), ("score off its row's reference", float(err.max()), tol)
    best = np.sort(ref)[::-1][:nv]
    err = np.abs(s - best)
    assert np.all(err <= tol), ("score off the sorted reference", float(err.max()), tol)
    if nv < N:
        rest = np.ones(N, bool)
        rest[got] = False
        over = ref[rest].max() - (s[nv - 1] + 2 * tol)
        assert over <= 0, ("a better row was not returned", float(over))


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ids at fragment, tile and workgroup-range edges and in the last, partly filled group
def edge_ids(N):
    return [i for i in (0, 15, 16, 63, 64, 255, 256, 257, N - 2, N - 1, N // 2) if 0 <= i < N]


PLANTED_SHAPES = [(64, 300, 3, 10), (64, 4099, 17, 10), (384, 1025, 5, 16), (768, 4099, 65, 10), (1024, 2049, 2, 32)]


def planted(d, N, B, k, seed=0):
    """(rows f32 [N][d], queries f32 [B][d], ids int [B][k]): for query b its j-th best
    row is a_j q + sqrt(1 - a_j^2) u_j at ids[b][j], a_j = 0.95 - 0.01 j, u_j a unit
    vector orthogonal to q; every other row is a random unit row.  The planted ids
    cover edge_ids(N)."""
    rng = np.random.default_rng(seed)
    rows = unit_rows(rng, N, d)
    queries = unit_rows(rng, B, d)
    edges = list(dict.fromkeys(edge_ids(N)))
    others = [i for i in rng.permutation(N).tolist() if i not in set(edges)]
    pool = edges + others
    assert B * k <= N
    ids = np.array(pool[:B * k], np.int64).reshape(B, k)
    for b in range(B):
        q = queries[b].astype(np.float64)
        for j in range(k):
            u = rng.standard_normal(d)
            u -= (u @ q) / (q @ q) * q
            u /= np.linalg.norm(u)
            a = 0.95 - 0.01 * j
            rows[ids[b, j]] = (a * q / np.linalg.norm(q) + np.sqrt(1.0 - a * a) * u).astype(np.float32)
    return rows, queries, ids


def numpy_device(queries, stored_rows, k):
    """A stand-in device: numpy's f32 matmul of the f16-rounded operands and a stable
    sort (equal scores keep ascending ids)."""
    q = np.asarray(queries, np.float32).astype(np.float16).astype(np.float32)
    sc = q @ np.asarray(stored_rows, np.float32).T
    B, N = sc.shape
    scores = np.full((B, k), -np.inf, np.float32)
    ids = np.full((B, k), -1, np.int32)
    for b in range(B):
        o = np.argsort(-sc[b], kind="stable")[:k]
        scores[b, :len(o)] = sc[b, o]
        ids[b, :len(o)] = o
    return scores, ids
