"""Numpy restatements of the host-checkable rules of the full-scan MaxSim search
(maxsim_search.hip, bert_hip.h "Full-scan search"): the (score, id) order of the results
with its fill, and the rule that deals the store's documents to the grid's waves."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def better(a_s, a_i, b_s, b_i):
    """topk_list.h `better`: higher score first, equal scores by ascending id; the id is
    compared unsigned, so the fill id -1 comes behind every document."""
    return a_s > b_s or (a_s == b_s and (a_i & 0xFFFFFFFF) < (b_i & 0xFFFFFFFF))


def topk(scores, k):
    """(scores f32 [k], ids i32 [k]) of the k best of scores[id], (-inf, -1) fill."""
    scores = np.asarray(scores, np.float32)
    order = np.lexsort((np.arange(len(scores)), -scores.astype(np.float64)))[:k]
    s = np.full(k, NEG_INF, np.float32)
    i = np.full(k, -1, np.int32)
    s[:len(order)] = scores[order]
    i[:len(order)] = order
    return s, i


def topk_brute(scores, k):
    """The same by repeated selection with `better`, nothing sorted."""
    left = [(np.float32(s), j) for j, s in enumerate(scores)]
    out = []
    for _ in range(k):
        best = None
        for e in left:
            if best is None or better(e[0], e[1], best[0], best[1]):
                best = e
        if best is None:
            out.append((NEG_INF, -1))
        else:
            out.append(best)
            left.remove(best)
    return np.array([e[0] for e in out], np.float32), np.array([e[1] for e in out], np.int32)


def table_of(lens):
    """(first group, len) per document as the store lays them out: contiguous from group 0,
    ceil(len / 16) groups each.  Returns (table int64 [n][2], used groups)."""
    lens = np.asarray(lens, np.int64).reshape(-1)
    groups = (lens + 15) // 16
    first = np.concatenate([[0], np.cumsum(groups)[:-1]]) if len(lens) else np.zeros(0, np.int64)
    return np.stack([first, lens], axis=1) if len(lens) else np.zeros((0, 2), np.int64), int(groups.sum())


def first_doc_at(table, g):
    """The first document whose first group is >= g (the kernel's binary search)."""
    lo, hi = 0, len(table)
    while lo < hi:
        mid = (lo + hi) >> 1
        if table[mid][0] < g:
            lo = mid + 1
        else:
            hi = mid
    return lo


def wave_ranges(table, G, W):
    """Per wave v of W the documents [dA, dB) it scores: those whose first group lies in
    [v G / W, (v + 1) G / W) (integer division)."""
    return [(first_doc_at(table, v * G // W), first_doc_at(table, (v + 1) * G // W)) for v in range(W)]


def range_groups(table, G, rng):
    """The groups a wave streams for the document range rng."""
    dA, dB = rng
    if dA >= dB:
        return 0
    end = table[dB][0] if dB < len(table) else G
    return int(end - table[dA][0])


def pad_rows(q, Lq):
    """q [n][w] with all-zero rows appended up to Lq rows."""
    q = np.asarray(q, np.float32)
    out = np.zeros((Lq, q.shape[1]), np.float32)
    out[:len(q)] = q
    return out


def maxsim_f32_by_rows(q16, doc16):
    """maxsim_refs.maxsim_f32 with every query row's maximum taken by a call of its own and
    the same sequential f32 sum: a row's similarities then do not depend on how many rows
    the query has (numpy's matrix product may block a taller matrix differently)."""
    import maxsim_refs as M
    s = np.float32(0.0)
    for i in range(len(q16)):
        s = np.float32(s + np.float32(M.maxsim_f32(q16[i:i + 1], doc16)))
    return s


def expected(ix, queries, k):
    """The search results the scorer implies: per query, alone, ix.score over every document,
    ordered by (-score, id), (-inf, -1) fill."""
    S = np.full((len(queries), k), NEG_INF, np.float32)
    I = np.full((len(queries), k), -1, np.int32)
    for b, q in enumerate(queries):
        if len(ix):
            S[b], I[b] = topk(ix.score(q), k)
    return S, I
