"""Numpy restatements of the host-checkable rules of the full-scan MaxSim search
(maxsim_search.hip, bert_hip.h "Full-scan search"): the (score, id) order of the results
with its fill, the rule that deals the store's documents to the grid's waves, and what a
wave then does with its run: the mid-stream flushes of the full scan and of the centroid scan
(maxsim_approx.hip) and the chunks of codes, for the shapes of test_gpu_maxsim_grid.py."""
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


# ---- what one wave of a scan does with its run (maxsim_search.hip, maxsim_approx.hip) ----
DOC_LENS = (1, 15, 16, 17, 33, 100)
FULL_WAVES, CENTROID_WAVES = 4, 8        # waves per workgroup of the full scan and of the centroid scan
RING_UNITS = {"f16": 4, "int8": 8}       # units of the full scan's ring (a unit is 64 elements of 16 rows)
CHUNK_GROUPS = 8                         # groups whose codes the centroid scan loads at a time (64 dwords)


def suite_lens(n, seed):
    """The document lengths of the token-store tests' make_docs(w, n, seed): the first draw of its generator."""
    return np.random.default_rng(seed).choice(DOC_LENS, n)


def grid_lens():
    """The store of test_gpu_maxsim_grid.py: 1,200 documents, one of 512 and one of 257 tokens."""
    lens = suite_lens(1200, 1200)
    lens[7], lens[600] = 512, 257
    return lens


def natural_waves(G, per_wg, cus=256, wg_per_cu=4):
    """The waves of a scan's own grid over G groups: wg_per_cu workgroups per CU (fewer where the
    LDS holds fewer), at most 1,024 workgroups, never more waves than groups."""
    return per_wg * max(1, min(wg_per_cu * cus, 1024, -(-G // per_wg)))


def wave_load(lens, W):
    """Per wave of W its run: (dA, dB, groups of each document dA .. dB - 1 in order)."""
    table, G = table_of(lens)
    per_doc = (np.asarray(lens, np.int64).reshape(-1) + 15) // 16
    out = []
    for dA, dB in wave_ranges(table, G, W):
        g = [int(x) for x in per_doc[dA:dB]]
        assert sum(g) == range_groups(table, G, (dA, dB))
        out.append((dA, dB, g))
    return out


def full_scan_flushes(doc_groups, w, kind):
    """The mid-stream flushes of a full-scan wave whose documents take doc_groups groups at width
    w: per flush the number of documents the wave has closed by then.  A group is w / 64 units;
    the wave takes whole passes of NU units, a document closes behind its last group's last
    unit, and behind a pass the pending scores are offered when more than 64 - NU are parked.
    (The units behind the last whole pass and the final flush are not counted.)"""
    NU, upg = RING_UNITS[kind], w // 64
    closes = np.cumsum(doc_groups) * upg          # the unit count at which each document closes
    U = int(closes[-1]) if len(closes) else 0
    out, npend, done = [], 0, 0
    for u0 in range(0, U - NU + 1, NU):
        while done < len(closes) and closes[done] <= u0 + NU:
            done += 1
            npend += 1
        assert npend <= 64
        if npend > 64 - NU:
            out.append(done)
            npend = 0
    return out


def centroid_scan_flushes(doc_groups):
    """The same for a centroid-scan wave: it offers when 64 scores are parked."""
    return list(range(64, len(doc_groups) + 1, 64))


def code_chunks(doc_groups):
    """The loads of 64 dwords of codes a centroid-scan wave consumes: 8 groups each."""
    return -(-sum(doc_groups) // CHUNK_GROUPS)


def closes_on_chunk_end(doc_groups):
    """Whether some document's last group is the last of a chunk (gi == 7)."""
    return any(int(e) % CHUNK_GROUPS == 0 for e in np.cumsum(doc_groups))


def spans_chunks(doc_groups):
    """Whether some document's groups lie in more than one chunk."""
    end = np.cumsum(doc_groups)
    return any((e - g) // CHUNK_GROUPS != (e - 1) // CHUNK_GROUPS for e, g in zip(end, doc_groups))


def one_token_at(lens, ids):
    """The lens of the store in which the documents `ids` are replaced by one-token documents."""
    lens = np.array(lens, np.int64)
    lens[list(ids)] = 1
    return lens


def edge_ids(lens, W):
    """[(wave, side, id)]: the first (side 0) and the last (side 1) document of every wave's
    range of W that has documents."""
    table, G = table_of(lens)
    return [(v, side, (dA, dB - 1)[side]) for v, (dA, dB) in enumerate(wave_ranges(table, G, W)) if dA < dB
            for side in (0, 1)]


def edge_distance(lens, W, id_, side):
    """How many documents lie between document id_ and the first (side 0) or last (side 1)
    document of the range of W that holds it, in the store of these lens.  (Replacing a longer
    document by a one-token document moves the later documents up, and the ranges with them.)"""
    table, G = table_of(lens)
    for dA, dB in wave_ranges(table, G, W):
        if dA <= id_ < dB:
            return (id_ - dA, dB - 1 - id_)[side]
    raise ValueError(id_)


TIE_PATTERN = [0, 0, 0, 1, 1, 1, 2]


def tie_ids(lens, W, w, kind, wave=1):
    """Nine ids for one-token copies of one document: seven in wave `wave` of the full scan's W,
    three offered before its first mid-stream flush, three between the first and the second and
    one behind the second (TIE_PATTERN), as near to the flushes as that allows, then one in the
    first and one in the last wave.  The flushes are those of the store with the copies in
    place, which tie_sides restates."""
    load = wave_load(lens, W)
    dA, dB, g = load[wave]
    f = full_scan_flushes(g, w, kind)
    for m in range(1, 9):
        ids = [dA + 3, dA + f[0] - m - 1, dA + f[0] - m, dA + f[0] + m - 1, dA + f[0] + m, dA + f[1] - m, dA + f[1] + m - 1,
               load[0][0] + 5, load[-1][1] - 6]
        sides = tie_sides(one_token_at(lens, ids), ids, W, w, kind)
        if sides[:7] == [(wave, n) for n in TIE_PATTERN] and sides[7][0] == 0 and sides[8][0] == W - 1:
            return ids
    raise ValueError("no nine ids around the flushes of wave %d" % wave)


def tie_sides(lens, ids, W, w, kind):
    """Per id (wave, mid-stream flushes of that wave before the document is offered), in the
    store whose lens are given (the copies in place)."""
    out = {}
    for v, (dA, dB, g) in enumerate(wave_load(lens, W)):
        f = full_scan_flushes(g, w, kind)
        for i in ids:
            if dA <= i < dB:
                out[i] = (v, sum(1 for x in f if x <= i - dA))
    return [out[i] for i in ids]


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
