"""Key counts on the attention kernels: attention_refs.py's batches with one number per
sentence, keys[b], 1 <= keys[b] <= len[b]: every row of the sentence is a query, only its
first keys[b] rows are keys and values (bert_hip.h "Key counts").  Shared by
test_cpu_attention_kv_refs.py and test_gpu_attention_kv.py.

A `KVCase` is a `Case` whose items() cuts each item's K and V to the counted rows; the float64
reference, the bounds and the restatements of attention_refs.py take a Q longer than K as they
are, so the reference is the attention over the counted keys and a bound counts the counted
keys' operations (n = 2 keys + ...: an excluded block is not accumulated).

Planted inputs.  uniform: Q = 0, the output is the exact mean of the counted V rows; the
excluded V rows are 512 (exact in f16), so one leaked key moves a mean by at least
(512 - 1) / (keys + 1) >= about 1 and a dropped last counted key by at least 0.25 / keys --
against a planted bound of about half an f16 step.  onehot: every row's target, the rows >= keys
too, lies inside the counted keys.  Every excluded key has P < 2^-20 there by the builder's
margin, so onehot cannot tell a leaked key from a masked one; random, latemax and uniform do
(`unmasked_reference`).
"""
import functools

import numpy as np

import attention_refs as R
from attention_refs import D, H

# (len, keys) per sentence
SHORT = [(1, 1), (2, 1), (33, 32), (64, 1), (64, 33), (64, 63), (32, 31), (17, 17)]
LDS = [(65, 1), (65, 64), (128, 64), (129, 65), (192, 128), (256, 129), (320, 1), (384, 191), (512, 64), (512, 511),
       (512, 512), (100, 40)]
STREAM = [(1000, 1), (1000, 999), (640, 64), (641, 65), (513, 512), (130, 130)]
HEADS3 = [(130, 65), (64, 1), (300, 129), (1, 1)]
HEADS3_SHORT = [(64, 33), (1, 1), (33, 32)]
EXCLUDED_V = 512.0


class KVCase(R.Case):
    """pairs: (len, keys) per sentence.  The inputs are Case's, then: uniform, the excluded V rows
    set to 512; onehot, Q rebuilt so that every row's target is a counted key."""

    def __init__(self, pairs, n_head, dh, kind, seed=0, head_offset=False):
        self.keys = np.array([k for _, k in pairs], np.int32)
        lens = [n for n, _ in pairs]
        assert all(1 <= k <= n for n, k in pairs)
        super().__init__(lens, n_head, dh, kind, seed=seed, head_offset=head_offset)
        if kind in ("uniform", "onehot"):
            qkv = self.qkv.copy()
            d = self.d
            for b, (n, nk) in enumerate(pairs):
                s = int(self.cu[b])
                if kind == "uniform":
                    qkv[s + nk:s + n, 2 * d:] = EXCLUDED_V
                else:
                    pi = R.onehot_map(b, nk)[np.arange(n) % nk]
                    self.target[s:s + n] = s + pi
                    qkv[s:s + n, :d] = (8.0 * qkv[s:s + n, d:2 * d].astype(D)[pi]).astype(H)
            qkv.setflags(write=False)
            self.qkv = qkv
            self._reference()
            self._bounds = {}

    def items(self):
        """(rows, columns, Q, K, V) of every (sentence, head): K and V the counted rows only."""
        n_head = self.n_head
        for i, (r, c, Q, K, V) in enumerate(super().items()):
            nk = int(self.keys[i // n_head])
            yield r, c, Q, K[:nk], V[:nk]

    def uniform_exact(self):
        """Case.uniform_exact on the counted rows (the excluded ones are 512 and take no part):
        every counted V a multiple of 2^-6 with 0.25 <= |v| < 1 (behind the head offset), Q = 0."""
        ok = not self.qkv[:, :self.d].any()
        for b, (r, c, Q, K, V) in enumerate(self.items()):
            v = V.astype(D) - (c.start // self.dh if self.head_offset else 0)
            ok = ok and np.array_equal(v * 64, np.round(v * 64)) and np.abs(v).min() >= 0.25 and np.abs(v).max() < 1.0
            ok = ok and np.abs(V.astype(D)).sum(axis=0).max() < 2.0 ** 18
        full = self.qkv[:, 2 * self.d:].astype(D)
        for b in range(len(self.lens)):
            ex = full[int(self.cu[b]) + int(self.keys[b]):int(self.cu[b + 1])]
            ok = ok and bool((ex == EXCLUDED_V).all())
        return bool(ok)

    def truncated(self):
        """The plain batch of the counted rows alone: (qkv f16 [sum keys][3d], cu, rows) with rows
        the positions of those rows in this batch."""
        rows = np.concatenate([np.arange(int(self.cu[b]), int(self.cu[b]) + int(self.keys[b]))
                               for b in range(len(self.lens))])
        return np.ascontiguousarray(self.qkv[rows]), R.cu_of(self.keys), rows


def unmasked_reference(cs):
    """The float64 attention of the same inputs with every row a key: what a kernel that ignores
    the counts computes."""
    sl2 = R.LOG2E / np.sqrt(cs.dh)
    out = np.zeros((cs.T, cs.d))
    for r, c, Q, K, V in R.Case.items(cs):
        t = sl2 * (Q.astype(D) @ K.astype(D).T)
        p = np.exp2(t - t.max(axis=1, keepdims=True))
        out[r, c] = (p / p.sum(axis=1, keepdims=True)) @ V.astype(D)
    return out


KV_MUTATIONS = ("drop_last", "mask_gt")


def restate(cs, kind, mut=None, truncate=False):
    """attention_refs' restatement of `kind` over a KVCase: (out f16 [T][d], moves).  drop_last:
    the last counted key masked; mask_gt: key `keys` let in, the sentence's own row where it has
    one (keys < len), else the image's row behind the end as in attention_refs.  truncate: the
    queries cut to the counted rows too (the plain batch of `truncated`, in this batch's rows)."""
    out = np.zeros((cs.T, cs.d), H)
    moves = []
    full = list(R.Case.items(cs))
    for i, (r, c, Q, K, V) in enumerate(cs.items()):
        m = mut
        if mut == "mask_gt" and len(K) < len(Q):
            K, V, m = full[i][3][:len(K) + 1], full[i][4][:len(K) + 1], None
        if truncate:
            Q = Q[:len(K)]
        rows = slice(r.start, r.start + len(Q))
        if kind == R.WAVE64:
            out[rows, c], mv = R.restate_wave64(Q, K, V, m)
            moves.append(mv)
        else:
            out[rows, c] = R.restate_runmax(Q, K, V, kind, m)
    return out, moves if kind == R.WAVE64 else None


BATCHES = {"short": (SHORT, 2, 64), "lds": (LDS, 2, 64), "lds32": (LDS, 2, 32), "stream64": (STREAM, 2, 64),
           "stream32": (STREAM, 2, 32), "heads3": (HEADS3, 3, 64), "heads3_short": (HEADS3_SHORT, 3, 64)}


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """The batches both test files use, built once per process (latemax and onehot in the
    reversed order, as attention_refs.case)."""
    pairs, n_head, dh = BATCHES[name]
    if kind in ("latemax", "onehot"):
        pairs = pairs[::-1]
    return KVCase(pairs, n_head, dh, kind, seed=len(name), head_offset=name.startswith("heads3"))


@functools.lru_cache(maxsize=None)
def wave64_moves(name, kind):
    """Whether AttWave64's restatement moves an offset anywhere, on the batch with counts or on
    its truncated form.  Where it does not, no wave's ballot fires in either run, the ballot is
    the only coupling between the queries of a wave, and rows < keys must have the truncated
    batch's bits."""
    cs = case(name, kind)
    return any(mv.any() for t in (False, True) for mv in restate(cs, R.WAVE64, truncate=t)[1])
