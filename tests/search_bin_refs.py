"""The binary embedding index restated in numpy (bert_hip.h, "Binary storage").

Everything here is integer arithmetic, so the device's bits, scores and result order must
equal these bit for bit:
  bit_i = 1 iff x_i > 0 (taken on the float's bit pattern, as the kernels take it);
  stored as np.packbits does: element i is bit 7 - i % 8 of byte i / 8;
  score = d - 2 popcount(bits_q xor bits_row), as float32;
  results by (score descending, id ascending), (-inf, -1) fill.
select() is the last step of the two-stage search (bertx_index_search_rescored).
"""
import numpy as np

from search_i8_refs import expected_topk  # noqa: F401  (the stable sort the int8 tests use)


def binarize(x):
    """uint8 [n][d / 8]: the sign bits of rows x float32 [n][d], from the bit patterns: a
    float is > 0 iff its pattern p satisfies 1 <= p <= 0x7f800000 (positive, not NaN)."""
    x = np.ascontiguousarray(np.asarray(x, np.float32))
    if x.ndim == 1:
        x = x[None, :]
    p = x.view(np.uint32)
    pos = (p - np.uint32(1)) < np.uint32(0x7F800000)     # wraps for p == 0
    return np.packbits(pos, axis=1)


def signs(bits, d):
    """int64 [n][d] of +1 / -1 from packed bits."""
    return np.unpackbits(np.asarray(bits, np.uint8), axis=1)[:, :d].astype(np.int64) * 2 - 1


def hamming(qbits, rbits):
    """int64 [B][N]: popcount(q xor r) of every pair."""
    q = np.unpackbits(np.asarray(qbits, np.uint8), axis=1).astype(np.float32)
    r = np.unpackbits(np.asarray(rbits, np.uint8), axis=1).astype(np.float32)
    if r.shape[0] == 0:
        return np.zeros((q.shape[0], 0), np.int64)
    # |q| + |r| - 2 q.r; every term is an integer of at most 1024, exact in float32
    both = (q @ r.T).astype(np.int64)
    return q.sum(axis=1).astype(np.int64)[:, None] + r.sum(axis=1).astype(np.int64)[None, :] - 2 * both


def ref_scores_bin(qbits, rbits, d):
    """float32 [B][N]: d - 2 hamming."""
    return (d - 2 * hamming(qbits, rbits)).astype(np.float32)


def ranks(ref_row, ids):
    """How many rows come before each of `ids` in the order of the results (score
    descending, id ascending), for one query's scores ref_row [N]."""
    ref_row = np.asarray(ref_row)
    out = []
    for i in ids:
        s = ref_row[i]
        out.append(int(np.count_nonzero(ref_row > s) + np.count_nonzero(ref_row[:i] == s)))
    return out


def select(scores, ids, fine_size, k):
    """The last step of the two-stage search: per query the k best (score, id) pairs by
    (score descending, id ascending); a pair whose id is -1 or >= fine_size is the fill
    (-inf, -1) and comes last."""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int32)
    B = scores.shape[0]
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int32)
    for b in range(B):
        keep = (ids[b] >= 0) & (ids[b] < fine_size)
        s, i = scores[b][keep], ids[b][keep]
        o = np.lexsort((i, -s.astype(np.float64)))[:k]
        out_s[b, :len(o)] = s[o]
        out_i[b, :len(o)] = i[o]
    return out_s, out_i


def special_rows(rng, n, d):
    """Random rows with the binarizer's edge cases planted: +0, -0, NaN, a subnormal,
    -1e-30, +-inf in row 0 .. and an all-negative row (when n allows)."""
    x = rng.standard_normal((n, d)).astype(np.float32)
    edge = np.array([0.0, -0.0, np.nan, 1e-45, -1e-45, -1e-30, 1e-30, np.inf, -np.inf], np.float32)
    x[0, :len(edge)] = edge
    x[0, d - len(edge):] = edge[::-1]
    if n > 2:
        x[n - 1, d // 2:d // 2 + len(edge)] = edge
        x[1] = -np.abs(x[1]) - np.float32(1e-3)          # all negative: no bit set
    return x
