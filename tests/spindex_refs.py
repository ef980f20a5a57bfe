"""References of the sparse index (bert_hip.h "Sparse index"): the selection as a stable
argsort, the planted selection rows, and the scan's score restated in numpy in the contract's
own order of additions, with the float64 value and bound beside it."""
import numpy as np

F = np.float32
U = 2.0 ** -24
PLANTED = [("zero", "few", "ties"), ("lowbit", "denormal", "random")]


def select_ref(rows, n):
    """(terms int32 [S][n], weights f32 [S][n], counts int32 [S]): per row the min(n, positives)
    largest weights, equal weights to the lower term (a stable sort), re-sorted by term; (-1, 0) fill."""
    S = rows.shape[0]
    terms, wts, counts = np.full((S, n), -1, np.int32), np.zeros((S, n), F), np.zeros(S, np.int32)
    for s in range(S):
        c = min(n, int((rows[s] > 0).sum()))
        keep = np.sort(np.argsort(-rows[s], kind="stable")[:c])
        terms[s, :c], wts[s, :c], counts[s] = keep, rows[s, keep], c
    return terms, wts, counts


def planted_row(kind, V, n, rng):
    """One selection row; every kind shrinks to what V holds."""
    row = np.zeros(V, F)
    if kind == "few":          # fewer than n positive weights
        at = rng.permutation(V)[:min(V, n) // 2]
        row[at] = rng.uniform(0.1, 3.0, len(at)).astype(F)
    elif kind == "ties":       # eight equal weights straddle the cut: n - 4 above them, the rest below
        order = rng.permutation(V)
        tie, rest = order[:min(8, V)], order[min(8, V):]
        above = max(min(n - 4, len(rest)), 0)
        row[tie] = 1.5
        row[rest[:above]] = rng.uniform(2.0, 3.0, above).astype(F)
        row[rest[above:]] = rng.uniform(0.5, 1.0, len(rest) - above).astype(F)
    elif kind == "lowbit":     # the n-th and (n + 1)-th values differ in the lowest mantissa bit
        row[:] = rng.uniform(1.0, 2.0, V).astype(F)
        if V > n:
            order = np.argsort(-row, kind="stable")
            row[order[n]] = np.nextafter(row[order[n - 1]], F(0))
    elif kind == "denormal":   # a denormal f32 weight is > 0
        at = rng.permutation(V)[:max(min(V, n) // 2, 1)]
        row[at] = rng.uniform(0.1, 3.0, len(at)).astype(F)
        row[at[0]] = F(1e-40)
    elif kind == "random":     # about half zeros, many repeated values
        row[:] = (rng.integers(-40, 40, V).clip(0) / 8.0).astype(F)
    return row


def make_docs(V, n_top, n_docs, seed):
    """n_docs documents (terms int32 ascending, weights f32 exact in f16): the lengths walk 0, 1,
    15, 16, 17, 63, 64, 65, n_top and random ones; every seventh document repeats the one before."""
    rng = np.random.default_rng(seed)
    lens = [L for L in (0, 1, 15, 16, 17, 63, 64, 65, n_top) if L <= n_top]
    docs = []
    for i in range(n_docs):
        if i % 7 == 6:
            docs.append(docs[-1])
            continue
        L = n_top if n_docs == 1 else lens[i % len(lens)] if i < 3 * len(lens) else int(rng.integers(0, n_top + 1))
        terms = np.sort(rng.permutation(V)[:L]).astype(np.int32)
        docs.append((terms, rng.uniform(0.0, 3.0, L).astype(np.float16).astype(F)))
    return docs


def scores_ref(queries, docs):
    """(scores f32 [B][docs] in the contract's order, exact float64 [B][docs], bound [B][docs] =
    count * 2^-24 * sum |qh w|).  Posting j adds to sub-sum j % 16 in ascending j; the 16 sub-sums
    fold 8, 4, 2, 1 apart; padding postings are (term 0, +0)."""
    qh = queries.astype(np.float16).astype(F)
    B = qh.shape[0]
    got, exact, bound = np.zeros((B, len(docs)), F), np.zeros((B, len(docs))), np.zeros((B, len(docs)))
    for i, (terms, w) in enumerate(docs):
        pad = -len(terms) % 16
        t, wp = np.concatenate([terms, np.zeros(pad, np.int32)]), np.concatenate([w, np.zeros(pad, F)])
        prod = (qh[:, t] * wp).reshape(B, -1, 16)          # exact in f32
        s = np.zeros((B, 16), F)
        for u in range(prod.shape[1]):
            s = s + prod[:, u]
        for half in (8, 4, 2, 1):
            s = s[:, :half] + s[:, half:]
        got[:, i] = s[:, 0]
        p64 = qh[:, terms].astype(np.float64) * w.astype(np.float64)
        exact[:, i] = p64.sum(axis=1)
        bound[:, i] = len(terms) * U * np.abs(p64).sum(axis=1)
    return got, exact, bound


def topk_ref(scores, k):
    """(scores f32 [B][k], ids int32 [B][k]) of scores [B][docs]: higher first, equal scores by
    ascending id, (-inf, -1) fill."""
    B, n = scores.shape
    out_s, out_i = np.full((B, k), -np.inf, F), np.full((B, k), -1, np.int32)
    for b in range(B):
        order = np.lexsort((np.arange(n), -scores[b].astype(np.float64)))[:k]
        out_s[b, :len(order)], out_i[b, :len(order)] = scores[b, order], order
    return out_s, out_i
