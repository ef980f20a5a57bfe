"""Numpy restatements of the host-checkable rules of the centroid codes and the pruned MaxSim
search (bert_hip.h "Centroid codes", "Pruned search"; maxsim_codes.hip, maxsim_approx.hip,
kmeans_update.h): the substitution rule behind the approximate score, the composition of the
pruned search from public pieces, the training sample and update, and the planted store of
the recall test with its float64 margins."""
import numpy as np

import maxsim_i8_refs as R8
import maxsim_refs as M
import maxsim_search_refs as SR

NEG_INF = SR.NEG_INF
SAMPLE_MAX = 1 << 18


# ---- the substitution rule ----
def substitute(cent, codes):
    """The documents of the substituted store: every stored row replaced by the caller's f32
    centroid row of its code.  approx(q, doc) is the scorer's score of q on these."""
    cent = np.asarray(cent, np.float32)
    return [cent[np.asarray(c, np.int64)] for c in codes]


def nearest(sims):
    """The code rule on a row of similarities: the highest, equal ones to the lower index."""
    sims = np.asarray(sims)
    best = 0
    for c in range(1, len(sims)):
        if sims[c] > sims[best]:
            best = c
    return best


# ---- the pruned search from public pieces ----
def compose(exact, ids, k):
    """(scores f32 [k], ids i32 [k]): the k best by `better` of the pairs (exact[j], ids[j]);
    a pair whose id is -1 is the fill (-inf, -1)."""
    pairs = [(np.float32(s), int(i)) for s, i in zip(exact, ids) if i >= 0]
    out = []
    for _ in range(k):
        best = None
        for e in pairs:
            if best is None or SR.better(e[0], e[1], best[0], best[1]):
                best = e
        if best is None:
            out.append((NEG_INF, -1))
        else:
            out.append(best)
            pairs.remove(best)
    return np.array([e[0] for e in out], np.float32), np.array([e[1] for e in out], np.int32)


# ---- training ----
def sample_rule(T, seed):
    """(stride, start, n_sample) of T valid token rows."""
    stride = max(1, -(-T // SAMPLE_MAX))
    start = seed % stride
    n = -(-(T - start) // stride) if T > start else 0
    return stride, start, n


def initial_rows(n_sample, C):
    return [c * n_sample // C for c in range(C)]


def kmeans_update(sample, codes, cent):
    """One update as a plain loop: float64 sums in ascending sample order, divided by the count,
    rounded to f32; a centroid without a member keeps its row.  Returns (new cent, empty count)."""
    sample = np.asarray(sample, np.float32)
    cent = np.array(cent, np.float32)
    C, w = cent.shape
    sums = [[0.0] * w for _ in range(C)]
    cnt = [0] * C
    for i in range(len(sample)):
        c = int(codes[i])
        row = sums[c]
        x = sample[i]
        for e in range(w):
            row[e] = row[e] + float(x[e])
        cnt[c] += 1
    empty = 0
    for c in range(C):
        if cnt[c] == 0:
            empty += 1
            continue
        for e in range(w):
            cent[c, e] = np.float32(sums[c][e] / float(cnt[c]))
    return cent, empty


# ---- the planted store of the recall test ----
PLANT_W, PLANT_DIRS, PLANT_DOCS, PLANT_LEN, PLANT_QUERIES = 64, 64, 300, 8, 6


def planted_case():
    """(cent [64][w], docs, queries, targets): the centroids are 64 orthonormal directions; a
    document is 8 rows, each one direction (8 distinct ones per document) plus noise of norm
    about 0.2; query b is a noisy copy of document targets[b]'s rows.  A document that shares
    m of the target's 8 directions scores about m, so the target leads by about 1 or more."""
    rng = np.random.default_rng(77)
    w = PLANT_W
    cent = np.linalg.qr(rng.standard_normal((w, PLANT_DIRS)))[0].T.astype(np.float32)
    docs, dirs = [], []
    for _ in range(PLANT_DOCS):
        d = rng.choice(PLANT_DIRS, PLANT_LEN, replace=False)
        dirs.append(d)
        docs.append((cent[d] + 0.025 * rng.standard_normal((PLANT_LEN, w))).astype(np.float32))
    targets = [int(t) for t in rng.choice(PLANT_DOCS, PLANT_QUERIES, replace=False)]
    queries = [(docs[t] + 0.025 * rng.standard_normal((PLANT_LEN, w))).astype(np.float32) for t in targets]
    return cent, docs, queries, targets, dirs


def packed_f64(x, storage):
    """The values a store of the kind holds for rows x, as float64, by the restatements of
    maxsim_refs (f16) and maxsim_i8_refs (int8: q * u)."""
    if storage == "int8":
        q, u = R8.pack(x)
        return q.astype(np.float64) * u.astype(np.float64)[:, None]
    return M.f16_view(x).astype(np.float64)


def planted_margins(storage):
    """Per query, in float64 on the packed values: (lead of the target over the runner-up in
    the approximate score, the same in the exact score, the smallest lead of a stored row's
    planted direction over its second nearest centroid)."""
    cent, docs, queries, targets, dirs = planted_case()
    pc = packed_f64(cent, storage)
    pdocs = [packed_f64(d, storage) for d in docs]
    code_lead = np.inf
    codes = []
    for d, pd in zip(dirs, pdocs):
        sims = pd @ pc.T
        top2 = np.sort(sims, axis=1)[:, -2:]
        assert np.array_equal(sims.argmax(axis=1), d)
        code_lead = min(code_lead, float((top2[:, 1] - top2[:, 0]).min()))
        codes.append(sims.argmax(axis=1))
    out = []
    for q, t in zip(queries, targets):
        pq = packed_f64(q, storage)
        exact = np.array([(pq @ pd.T).max(axis=1).sum() for pd in pdocs])
        approx = np.array([(pq @ pc[c].T).max(axis=1).sum() for c in codes])
        lead = []
        for s in (approx, exact):
            others = np.delete(s, t)
            lead.append(float(s[t] - others.max()))
        out.append((lead[0], lead[1], code_lead))
    return out
