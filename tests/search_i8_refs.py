"""The int8 embedding index restated in numpy float32 (bert_hip.h, "Storage kinds").

Every operation the contract names is one float32 operation here too, so the device's
bytes, scales and scores must equal these bit for bit:
  amax = max |x_i|;  amax == 0: scale 0, q 0;  else inv = 127 / amax,
  q_i = clip(rint(x_i * inv), -127, 127), scale = amax / 127;
  score = float32(isum) * (scale_q * scale_row), isum the exact integer dot.
"""
import numpy as np

F127 = np.float32(127.0)


def quantize(x):
    """(q int8 [n][d], scale float32 [n]) of rows x float32 [n][d]."""
    x = np.ascontiguousarray(np.asarray(x, np.float32))
    if x.ndim == 1:
        x = x[None, :]
    amax = np.abs(x).max(axis=1)
    nz = amax > 0
    safe = np.where(nz, amax, np.float32(1.0)).astype(np.float32)
    inv = (F127 / safe).astype(np.float32)
    scale = np.where(nz, (safe / F127).astype(np.float32), np.float32(0.0)).astype(np.float32)
    prod = (x * inv[:, None]).astype(np.float32)        # one float32 multiply per element
    q = np.clip(np.rint(prod), -127, 127)               # np.rint: nearest even
    q = np.where(nz[:, None], q, 0).astype(np.int8)
    return q, scale


def ref_scores_i8(qq, qs, rq, rs):
    """float32 [B][N]: the score of every (query, row) pair from the quantized operands."""
    isum = qq.astype(np.int64) @ rq.astype(np.int64).T
    assert np.abs(isum).max(initial=0) < 2 ** 24
    ss = (np.asarray(qs, np.float32)[:, None] * np.asarray(rs, np.float32)[None, :]).astype(np.float32)
    return (isum.astype(np.float32) * ss).astype(np.float32)


def error_bound(x, y, sx, sy):
    """The deterministic bound on |x . y - score| of one pair (float64), without the two
    float32 roundings of the final multiplies: each dequantized element is within half a
    scale of its value, so x . y - (x + ex) . (y + ey) is at most
    (sy |x|_1 + sx |y|_1) / 2 + d sx sy / 4."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    sx, sy = float(sx), float(sy)
    return (sy * np.abs(x).sum() + sx * np.abs(y).sum()) / 2 + x.shape[-1] * sx * sy / 4


def expected_topk(ref, k):
    """(scores float32 [B][k], ids int32 [B][k]) of ref float32 [B][N]: descending, equal
    scores by ascending id (a stable sort), (-inf, -1) where N < k."""
    B, N = ref.shape
    scores = np.full((B, k), -np.inf, np.float32)
    ids = np.full((B, k), -1, np.int32)
    for b in range(B):
        o = np.argsort(-ref[b], kind="stable")[:k]
        scores[b, :len(o)] = ref[b, o]
        ids[b, :len(o)] = o
    return scores, ids
