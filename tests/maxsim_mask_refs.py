"""References of the token store's document masks (bertx_mvindex_remove,
bertx_mvindex_search_filtered, _candidates_filtered, _search_pruned_filtered; bert_hip.h
"Deleting documents and filtered search").

The masks are the embedding index's with a document in the place of a row, so the packers
and the selection are search_mask_refs' own: the expected result of a masked search is
select() applied to the [B][docs] score matrix that BertTokenIndex.score(q, ids=None) returns
before any removal, and the expected candidates are select() applied to the approx matrix
(candidates(q, docs) of the untouched store, scattered by id).  Nothing here has a tolerance.
"""
import numpy as np

from search_mask_refs import admissible, pack_bits, same, select, tombstones, unpack_bits, words_for  # noqa: F401

NEG_INF = np.float32(-np.inf)


def expected(S, k, dead=None, allow=None):
    """(scores [B][k], ids [B][k]): the k best admissible documents of the score matrix S
    f32 [B][docs] under the tombstones `dead` (bool [docs]) and the filter `allow` (bool [docs]
    or [B][docs])."""
    S = np.asarray(S, np.float32)
    return select(S, admissible(S.shape[1], S.shape[0], dead, allow), k)


def scatter(values, ids, docs):
    """f32 [B][docs] from per-query lists (values [B][n], ids [B][n]) that name every document
    once: matrix[b][ids[b][j]] = values[b][j]."""
    values, ids = np.asarray(values, np.float32), np.asarray(ids)
    out = np.full((values.shape[0], docs), np.nan, np.float32)
    for b in range(values.shape[0]):
        assert sorted(ids[b].tolist()) == list(range(docs)), "the lists must name every document once"
        out[b, ids[b]] = values[b]
    return out


def scores_with_deleted(S_row, ids, dead):
    """What score(q, ids) returns once `dead` documents are removed: S_row[id], -inf for an id
    outside [0, docs) or a deleted one."""
    S_row = np.asarray(S_row, np.float32)
    out = np.full(len(ids), NEG_INF, np.float32)
    for j, i in enumerate(np.asarray(ids, np.int64).tolist()):
        if 0 <= i < len(S_row) and not dead[i]:
            out[j] = S_row[i]
    return out


def map_live(result, dead):
    """The (scores, ids) of a search over a fresh store of the live documents, its ids mapped
    back through flatnonzero(live); the fill id -1 stays."""
    live = np.flatnonzero(~np.asarray(dead, bool))
    s, i = result
    i = np.asarray(i)
    out = np.full(i.shape, -1, np.int32)
    out[i >= 0] = live[i[i >= 0]]
    return s, out


def stand_in_device(S, docs, k, tomb_words=None, filt_words=None, use_tomb=True, use_filt=True):
    """A stand-in device that works from the packed words as the kernels do: document d of query
    b is listed iff d < docs, bit d of tomb_words is 0 and bit d of filter b (filt_words uint32
    [words] shared or [B][words]) is 1.  use_tomb / use_filt False ignore that mask: the devices
    a comparison must reject."""
    S = np.asarray(S, np.float32)
    ok = np.ones((S.shape[0], docs), bool)
    if use_tomb and tomb_words is not None:
        ok &= ~unpack_bits(tomb_words, docs)[None, :]
    if use_filt and filt_words is not None:
        f = unpack_bits(filt_words, docs)
        ok &= f[None, :] if f.ndim == 1 else f
    return select(S[:, :docs], ok, k)


def brute(S, k, dead=None, allow=None):
    """expected() by repeated selection, nothing sorted: per query the best remaining admissible
    document k times (higher score first, equal scores by ascending id), then the fill."""
    S = np.asarray(S, np.float32)
    B, N = S.shape
    out_s, out_i = np.full((B, k), NEG_INF, np.float32), np.full((B, k), -1, np.int32)
    for b in range(B):
        left = []
        for d in range(N):
            if dead is not None and dead[d]:
                continue
            if allow is not None:
                a = np.asarray(allow, bool)
                if not (a[d] if a.ndim == 1 else a[b, d]):
                    continue
            left.append(d)
        for j in range(k):
            best = None
            for d in left:
                if best is None or S[b, d] > S[b, best] or (S[b, d] == S[b, best] and d < best):
                    best = d
            if best is None:
                break
            out_s[b, j], out_i[b, j] = S[b, best], best
            left.remove(best)
    return out_s, out_i


def per_query_filters(B, docs, rng):
    """bool [B][docs] for one pass's worth of queries and more: some documents admitted by every
    query, some by none, some by exactly one (query d % B), the rest at random."""
    f = rng.random((B, docs)) < 0.5
    d = np.arange(docs)
    f[:, d % 5 == 0] = True
    f[:, d % 5 == 1] = False
    one = d % 5 == 2
    f[:, one] = False
    f[d[one] % B, d[one]] = True
    return f
