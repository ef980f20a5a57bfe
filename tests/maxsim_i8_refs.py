"""The int8 token store restated in numpy float32 (bert_hip.h, token store, "Storage kinds").

Every operation the contract names is one float32 operation here too, and every sum is
either an exact integer or spelled out lane by lane, so the device's bytes, scales and
scores must equal these bit for bit:
  q = the embedding index's quantizer (search_i8_refs.quantize), its scale dropped;
  n2 = sum q_i^2 (exact integer < 2^24);  u = 1 / sqrt(float32(n2)), 0 where n2 == 0;
  sim = float32(isum) * (u_a * u_c)   (search_i8_refs.ref_scores_i8);
  score = the 16-lane tile sum and xor butterfly over max_j sim.
"""
import numpy as np

import maxsim_refs as M
import search_i8_refs as S

WIDTHS = (64, 192, 768, 1024)   # 1, 3, 12 and 16 blocks of 64 per group
F1 = np.float32(1.0)


def n2_of(q):
    return (q.astype(np.int64) ** 2).sum(axis=-1)


def pack(x):
    """(q int8 [n][w], u float32 [n]) of rows x float32 [n][w]."""
    q, _ = S.quantize(x)
    n2 = n2_of(q)
    assert n2.max(initial=0) < 2 ** 24
    root = np.sqrt(np.where(n2 > 0, n2, 1).astype(np.float32)).astype(np.float32)
    u = np.where(n2 > 0, (F1 / root).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return q, u


def lane_sum(m):
    """The scorer's sum of the per-token maxima m float32 [Lq]: lane c adds m[c], m[16 + c],
    ... from +0 (an index >= Lq adds +0), then s += s[lane ^ o] for o = 8, 4, 2, 1."""
    m = np.asarray(m, np.float32)
    tiles = (len(m) + 15) // 16
    pad = np.zeros(16 * tiles, np.float32)
    pad[:len(m)] = m
    s = np.zeros(16, np.float32)
    for t in range(tiles):
        s = (s + pad[16 * t:16 * t + 16]).astype(np.float32)
    lanes = np.arange(16)
    for o in (8, 4, 2, 1):
        s = (s + s[lanes ^ o]).astype(np.float32)
    return s[0]


def score(qp, dp):
    """float32 score of the packed query qp = (q, u) against the packed document dp."""
    return lane_sum(S.ref_scores_i8(qp[0], qp[1], dp[0], dp[1]).max(axis=1))


def score_loops(qp, dp):
    """The same restated: three loops for the integer dot, scalar float32 operations, the
    butterfly as a recursion over the lanes."""
    (qq, qu), (cq, cu) = qp, dp
    best = []
    for i in range(len(qq)):
        b = np.float32(-np.inf)
        for j in range(len(cq)):
            isum = 0
            for k in range(qq.shape[1]):
                isum += int(qq[i, k]) * int(cq[j, k])
            b = max(b, np.float32(np.float32(isum) * np.float32(qu[i] * cu[j])))
        best.append(b)
    lane = []
    for c in range(16):
        s = np.float32(0.0)
        for i in range(c, 16 * ((len(best) + 15) // 16), 16):
            s = np.float32(s + (best[i] if i < len(best) else np.float32(0.0)))
        lane.append(s)

    def after(l, step):   # lane l's value after `step` butterfly steps
        if step == 0:
            return lane[l]
        o = (8, 4, 2, 1)[step - 1]
        return np.float32(after(l, step - 1) + after(l ^ o, step - 1))
    return after(0, 4)


# ---- the accuracy bound against the exact cosine ----
def quant_err(x):
    """float64 [n]: e_x = |q - x'|_2 / |x'|_2 per row, x' = 127 x / amax in real arithmetic."""
    x64 = np.asarray(x, np.float64)
    xp = 127.0 * x64 / np.abs(x64).max(axis=1, keepdims=True)
    q = pack(x)[0].astype(np.float64)
    return np.linalg.norm(q - xp, axis=1) / np.linalg.norm(xp, axis=1)


def sim_bound(x, y):
    """float64 [n][m]: 2 (e_x + e_y) + 2^-21, the bound on |sim - cos(x, y)| per pair."""
    return 2.0 * (quant_err(x)[:, None] + quant_err(y)[None, :]) + 2.0 ** -21


def exact_maxsim(x, y):
    """float64 MaxSim of the exact unit vectors of the raw rows."""
    return M.maxsim(M.normalise(x), M.normalise(y))
