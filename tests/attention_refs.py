"""Inputs, float64 references, numpy float32/float16 restatements and per-element error
bounds of the f16 attention kernels (attention.hip, attention_block.h, attention_cls.hip),
shared by test_gpu_attention_kernels.py (the kernels against them) and
test_cpu_attention_refs.py (the restatements against the references, and planted
mutations of the restatements against the bounds, before a GPU is involved).

Notation, per (sentence, head) and query q: t_j = sl2 (q . k_j) the score of key j in the
exp2 domain (sl2 = log2(e) / sqrt(dh)), p_j = 2^t_j / sum 2^t the reference probability,
o_i = sum_j p_j v_ji the reference output of column i, all float64 on the f16 inputs.

The bound (`Case.bound(kind)`, one per arithmetic: WAVE64 = AttWave64 of attention_short /
attention_pp / attention_lds3, LDS32 = attention_lds_kernel<32>, STREAM = attention_kernel,
CLS = attention_cls_kernel) is counted from the kernels' operations, never from their output:

  |got_i - o_i| <= A_i + b B_i + b0 sum_j |v_ji| + n U (B_i + |o_i|) + half an f16 step

  A_i = sum_j p_j E_j |v_ji - o_i| / (1 - max_j E_j): a kernel that uses P'_j = P_j (1 + e_j)
      in both the P V sum and the row sum returns o_i + sum_j p_j e_j (v_ji - o_i) / (1 + sum_j
      p_j e_j); E_j = expm1(ln 2 (d1_j + d2_j)) + 2^-22 bounds |e_j|:
      d1 (WAVE64, LDS32: Q is pre-scaled in f16, q'_e = f16(q_e s16), s16 = f16(sl2)):
          q'_e = s16 q_e + rho_e moves the score by (s16 / sl2 - 1) t_j + sum_e rho_e k_je.  The
          first part is a change of temperature and a shift common to all keys changes nothing,
          so it counts |s16 / sl2 - 1| |t_j - max t|; the second sum_e |rho_e| |k_je| with
          rho_e the f16 rounding error of the product (computed, at most 2^-11 |q'_e|).
          STREAM and CLS scale the f32 score: d1 = 0.
      d2 = 2 (dh + 2) U (M_j + C): the f32 accumulation of the dh exact f16 x f16 products
          (M_j = sum_e |q'_e k_je| or sl2 sum |q_e k_je|), and the subtraction of the offset or
          the running maximum (C = 1.002 max |t| + 2^-9 bounds it), whether inside the MFMA
          (the bias operand of AttWave64), by a v_sub_f32, or by CLS's fmaf chain, scale and
          log2(e) products; the factor 2 allows an MFMA that truncates instead of rounding.
      2^-22: v_exp_f32 (1 ulp) and exp2f (2 ulp at most).
      The f16 running offset of AttWave64 is f16-exact by construction ((h16)(c + m) - c is an
      exact f32 difference), so it changes which power of two multiplies every P but adds no
      error of its own; that P stays in f16 range is the kernel's ATT_SUMX argument.
  b = 2^-11 (1 + 2 max E), b0 = 2^-25 / 0.9 (not CLS): P is rounded to f16 for the P V MFMA
      while the row sum keeps the f32 value; relative 2^-11 for a normal f16, absolute 2^-25
      below 2^-14 (f16 subnormals are not flushed), over a row sum that is at least 0.9 (the
      key of the running maximum has P = 1; under AttWave64's f16 offset P >= 2^(-half an f16
      step of the offset) >= 0.95 while |t| < 256, which `Case` asserts).  B_i = sum_j p_j |v_ji|.
  n = 2 len + len / 16 + 16: the f32 accumulation of P V over len keys (2 per key, as above),
      of the row sum (relative, so times |o_i|), the rescales by alpha of O and l (two roundings
      per 64-key block or 256-key chunk), 1 / l and the final product.
  half an f16 step: of the value being rounded, taken at |o_i| + the rest of the bound.

U is the f32 unit roundoff 2^-24.
"""
import functools

import numpy as np

F, D, H = np.float32, np.float64, np.float16
U = 2.0 ** -24
LOG2E = 1.4426950408889634
ATT_SUMX = 12
WAVE64, LDS32, STREAM, CLS = "wave64", "lds32", "stream", "cls"
KINDS = ("random", "latemax", "uniform", "onehot")
# A fifth input for AttWave64's f16 offset: scores near 2^7 that differ by a few bits, from a Q
# whose f16 pre-scaling is exact (entries 0, +-16, +-32), and a V that is +-1 (times 0.75 .. 1.25)
# with the sign of keys 0-63 against all later keys.  The score terms of the bound then nearly
# vanish, while an offset that is not the f16 value the bias operand holds weighs block 0
# against the later blocks by up to 2^(half an f16 step at 128) = 4 %.
OFFSET_KIND = "offset"
ALL_KINDS = KINDS + (OFFSET_KIND,)

# launch_attention's g_att_ran values
RAN_SHORT, RAN_PP, RAN_LDS3, RAN_LDS32, RAN_STREAM = 0, 1, 2, 3, 4

# the lengths at the edges each kernel has: a one-token sentence and a maximal one are first
# and last (latemax and onehot run the reversed order, so both ends see both)
SHORT_LENS = [1, 2, 31, 32, 33, 63, 17, 64]
LDS_LENS = [1, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 383, 384, 448, 511, 512]
STREAM_LENS = [1, 1000, 64, 513, 130, 640, 641]
CLS_LENS = [1, 255, 256, 257, 512, 513, 1000]


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def sl2_f32(dh):
    """launch_attention's scale, in its own f32 arithmetic."""
    return F(F(F(1.0) / np.sqrt(F(dh))) * F(LOG2E))


def half_step_f16(x):
    """Half the f16 spacing at |x| (f64 array), taken at the next f16 value at or above it."""
    x = np.abs(np.asarray(x, D))
    h = x.astype(H)
    h = np.where(h.astype(D) < x, np.nextafter(h, H(np.inf)), h).astype(H)
    return np.spacing(h).astype(D) / 2


# ---------------------------------------------------------------- inputs

def onehot_keys(rng, n, dh, length_for_margin):
    """n random +-1 rows of dh, a row drawn again while its inner product with an earlier row
    is too large for the margin: with Q = 8 K[target] the other keys are 8 sl2 (dh - x) below
    the target in the exp2 domain, and length 2^-that must stay below 2^-20."""
    gap = 21.0 + np.log2(length_for_margin)
    xmax = int(np.floor(dh - gap / (8 * float(sl2_f32(dh)))))
    rows = np.zeros((n, dh), D)
    k = 0
    while k < n:
        cand = rng.integers(0, 2, (64, dh)) * 2.0 - 1.0
        for c in cand:
            if k == n:
                break
            if k == 0 or (rows[:k] @ c).max() <= xmax:
                rows[k] = c
                k += 1
    return rows


def onehot_map(b, n):
    """Even sentences: the reversal (query 0 looks at the last key, every query crosses the
    middle); odd ones: a rotation by half the sentence plus one, so neighbouring sentences
    differ and blocks, half-items and tiles are crossed in both directions."""
    i = np.arange(n)
    return n - 1 - i if b % 2 == 0 else (i + n // 2 + 1) % n


class Case:
    """One batch: f16 qkv [T][3d], its float64 reference and the reference's own quantities.
    head_offset: head h's V gets + h, so an output in another head's columns is off by an
    integer."""

    def __init__(self, lens, n_head, dh, kind, seed=0, head_offset=False):
        self.lens, self.n_head, self.dh, self.kind = list(lens), n_head, dh, kind
        self.d = d = n_head * dh
        self.head_offset = head_offset
        self.cu = cu_of(lens)
        self.T = T = int(self.cu[-1])
        rng = np.random.default_rng(1000 * seed + 7 * dh + ALL_KINDS.index(kind))
        q = rng.standard_normal((T, d))
        k = rng.standard_normal((T, d))
        v = rng.standard_normal((T, d))
        self.target = None
        for b, n in enumerate(lens):
            r = slice(self.cu[b], self.cu[b + 1])
            if kind == "latemax":
                # scores whose scale grows along the sentence: the row maximum comes late
                q[r] *= 2.5
                k[r] *= np.linspace(0.3, 2.5, n)[:, None]
            elif kind == "uniform":
                q[r] = 0.0
                mag = rng.integers(16, 64, (n, d)) / 64.0
                v[r] = mag * np.where(rng.integers(0, 2, (n, d)) > 0, 1.0, -1.0)
            elif kind == OFFSET_KIND:
                for h in range(n_head):
                    c = slice(h * dh, (h + 1) * dh)
                    sig = rng.integers(0, 2, 8) * 2.0 - 1.0
                    q[r, c] = 0.0
                    k[r, c] = 0.0
                    q[r, c][:, :8] = 16.0 * sig * rng.integers(1, 3, (n, 8))
                    k[r, c][:, :8] = sig * (4.0 + 0.15 * rng.standard_normal((n, 8)))
                    side = np.where(np.arange(n)[:, None] < 64, 1.0, -1.0) * (rng.integers(0, 2, dh) * 2.0 - 1.0)
                    v[r, c] = side * rng.uniform(0.75, 1.25, (n, dh))
            elif kind == "onehot":
                if self.target is None:
                    self.target = np.zeros(T, np.int64)
                pi = onehot_map(b, n)
                self.target[r] = self.cu[b] + pi
                for h in range(n_head):
                    c = slice(h * dh, (h + 1) * dh)
                    kk = onehot_keys(rng, n, dh, max(lens))
                    k[r, c] = kk
                    q[r, c] = 8.0 * kk[pi]
        if head_offset:
            for h in range(n_head):
                v[:, h * dh:(h + 1) * dh] += h
        self.qkv = np.ascontiguousarray(np.concatenate([q, k, v], axis=1).astype(H))
        self.qkv.setflags(write=False)
        self._reference()
        self._bounds = {}

    def items(self):
        """(rows, columns, Q, K, V) of every (sentence, head), f16."""
        d, dh = self.d, self.dh
        for b in range(len(self.lens)):
            r = slice(int(self.cu[b]), int(self.cu[b + 1]))
            for h in range(self.n_head):
                c = slice(h * dh, (h + 1) * dh)
                yield r, c, self.qkv[r, c], self.qkv[r, d + h * dh:d + (h + 1) * dh], \
                    self.qkv[r, 2 * d + h * dh:2 * d + (h + 1) * dh]

    def _reference(self):
        """f64 attention of the f16 inputs; the probabilities and scores are kept per item."""
        sl2 = LOG2E / np.sqrt(self.dh)
        self.ref = np.zeros((self.T, self.d))
        self.probs, self.scores = [], []
        for r, c, Q, K, V in self.items():
            t = sl2 * (Q.astype(D) @ K.astype(D).T)
            assert np.abs(t).max() < 256.0          # the row-sum floor of the bound's b0
            p = np.exp2(t - t.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            self.ref[r, c] = p @ V.astype(D)
            self.probs.append(p)
            self.scores.append(t)
        self.ref.setflags(write=False)

    # ---- the planted builders' own conditions (asserted by the CPU file, on the reference alone)
    def uniform_exact(self):
        """Every V is a multiple of 2^-6 with 0.25 <= |v| < 1 and a sentence's sum of |v| is
        below 2^18 (head offsets, integers below 4, included), so every partial sum in any order
        is a multiple of 2^-6 below 2^18: exact in f32.  Q = 0: every score is 0, every P exactly 1 and the row sum exactly len."""
        v = self.qkv[:, 2 * self.d:].astype(D)
        if self.head_offset:
            v = v - np.repeat(np.arange(self.n_head), self.dh)[None, :]
        ok = np.array_equal(v * 64, np.round(v * 64)) and np.abs(v).min() >= 0.25 and np.abs(v).max() < 1.0
        ok = ok and not self.qkv[:, :self.d].any()
        return ok and all(np.abs(V.astype(D)).sum(axis=0).max() < 2.0 ** 18 for _, _, _, _, V in self.items())

    def onehot_margin(self):
        """The smallest probability any query gives its target."""
        worst = 1.0
        for (r, c, Q, K, V), p in zip(self.items(), self.probs):
            tg = self.target[r] - r.start
            worst = min(worst, p[np.arange(len(tg)), tg].min())
        return worst

    # ---- bounds
    def bound(self, kind):
        if kind not in self._bounds:
            bd = np.zeros((len(self.lens) if kind == CLS else self.T, self.d))
            for i, ((r, c, Q, K, V), p, t) in enumerate(zip(self.items(), self.probs, self.scores)):
                if kind == CLS:                          # the sentence's first query alone
                    bd[i // self.n_head, c] = _item_bound(Q[:1], K, V, p[:1], t[:1], self.ref[r, c][:1], kind)
                else:
                    bd[r, c] = _item_bound(Q, K, V, p, t, self.ref[r, c], kind)
            bd.setflags(write=False)
            self._bounds[kind] = bd
        return self._bounds[kind]

    def planted_bound(self, kind):
        """uniform: the output is the f16 rounding of x = f32(sum * f32(1 / len)) with the sum
        exact; 1 / len (one rounding, or v_rcp_f32's 1 ulp) and the product (one rounding) put
        x within 2^-22 |mean| of the mean, and the f16 rounding adds half a step.
        onehot: p_target >= 1 - 2^-20, so the reference is within 2^-19 max |v| of the target's
        V row; the target's P, rounded to f16 for the MFMA but not in the row sum, scales the row
        by 1 + rho, |rho| <= 2^-11, which is up to one f16 step of v (not CLS, whose P stays
        f32); accumulation and 1 / l add a few f32 roundings (8 U); then half a step of the
        final rounding: about two f16 steps in all.  Returned with the expected values."""
        if self.kind == "uniform":
            want = self.ref
            pre = 2.0 ** -22 * np.abs(want)
        else:
            v = self.qkv[:, 2 * self.d:].astype(D)
            want = v[self.target]
            vmax = np.abs(v).max()
            pre = (0.0 if kind == CLS else 2.0 ** -11) * np.abs(want) + 2.0 ** -19 * vmax + 8 * U * vmax
        return want, pre + half_step_f16(np.abs(want) + pre)


def _item_bound(Q, K, V, p, t, o, kind):
    Lq, dh = Q.shape
    L = len(K)
    q, k, v = Q.astype(D), K.astype(D), V.astype(D)
    sl2 = LOG2E / np.sqrt(dh)
    absk = np.abs(k)
    if kind in (WAVE64, LDS32):
        s16 = float(H(sl2_f32(dh)))
        qs = (Q * H(s16)).astype(D)                      # f16(q s16), one rounding
        rho = np.abs(qs - q * s16)
        d1 = abs(s16 / sl2 - 1.0) * np.abs(t - t.max(axis=1, keepdims=True)) + rho @ absk.T
        M = np.abs(qs) @ absk.T
    else:
        d1 = 0.0
        M = sl2 * (np.abs(q) @ absk.T)
    C = 1.002 * np.abs(t).max(axis=1, keepdims=True) + 2.0 ** -9
    d2 = 2 * (dh + 2) * U * (M + C)
    E = np.expm1(np.log(2.0) * (d1 + d2)) + 2.0 ** -22
    Emax = E.max(axis=1, keepdims=True)
    W = p * E / (1.0 - Emax)
    A = np.zeros((Lq, dh))
    for q0 in range(0, Lq, 64):
        A[q0:q0 + 64] = np.einsum("qj,qji->qi", W[q0:q0 + 64], np.abs(v[None, :, :] - o[q0:q0 + 64, None, :]))
    B = p @ np.abs(v)
    pre = A + (2 * L + L / 16 + 16) * U * (B + np.abs(o))
    if kind != CLS:
        pre = pre + 2.0 ** -11 * (1 + 2 * Emax) * B + 2.0 ** -25 / 0.9 * np.abs(v).sum(axis=0)[None, :]
    return pre + half_step_f16(np.abs(o) + pre)


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """The batches both test files use, built once per process."""
    lens, n_head, dh = {"short": (SHORT_LENS, 2, 64), "lds": (LDS_LENS, 2, 64), "lds32": (LDS_LENS, 2, 32),
                        "stream64": (STREAM_LENS, 2, 64), "stream32": (STREAM_LENS, 2, 32),
                        "heads3": ([130, 64, 300, 1], 3, 64), "heads3_short": ([64, 1, 33], 3, 64),
                        "cls64": (CLS_LENS, 2, 64), "cls32": (CLS_LENS, 2, 32)}[name]
    if kind in ("latemax", "onehot"):
        lens = lens[::-1]
    return Case(lens, n_head, dh, kind, seed=len(name), head_offset=name.startswith("heads3"))


# ---------------------------------------------------------------- restatements
#
# What is restated op for op: every f16 rounding (Q scaling, the offset, P, the output), every
# f32 VALU operation in the kernel's order (the shifts, the per-half row sums in the lane's
# register order, the rescales, 1 / l), the mask, the wave-wide ballot of the offset move.
# What is not: an MFMA's internal accumulation order is not established, so a 32x32x16 MFMA
# is the float64 sum of its 16 exact products and its accumulator input, rounded to f32 once;
# v_exp_f32 and exp2f are numpy's float32 exp2 (each within an ulp or two of the other); the
# compiler may contract a * b + c into an fma where the source has both, here they round twice.

MUTATIONS = ("drop_last", "drop_block_first", "swap_v", "mask_gt", "skip_rescale", "unrounded_offset")


def _keys(K, V, mut, clamp):
    """K, V padded to whole 64-key blocks as the kernel's image holds them (clamp: copies of
    the last row; else zeros) and which keys take part; the key-level mutations act here."""
    L = len(K)
    nrows = (L + 63) // 64 * 64
    idx = np.minimum(np.arange(nrows), L - 1)
    Kp, Vp = K[idx].copy(), V[idx].copy()
    if not clamp:
        Kp[L:], Vp[L:] = 0, 0
    valid = np.arange(nrows) < L
    if mut == "drop_last":
        valid[L - 1] = False
    elif mut == "drop_block_first":
        valid[0::64] = False
    elif mut == "swap_v" and L >= 2:
        a, b = L // 3, L - 1
        Vp[[a, b]] = Vp[[b, a]]
    elif mut == "mask_gt":
        valid = np.arange(nrows) <= L
    return Kp, Vp, valid


def _half_sums(P):
    """expsum's f32 row sum per 32-lane half: P [L][64] of a block -> [L][2]; half hi adds its
    keys 32 kh + (r & 3) + 8 (r >> 2) + 4 hi in register order kh, r."""
    rs = np.zeros((P.shape[0], 2), F)
    for hi in range(2):
        for kh in range(2):
            for r in range(16):
                rs[:, hi] = rs[:, hi] + P[:, 32 * kh + (r & 3) + 8 * (r >> 2) + 4 * hi]
    return rs


def _pv(o, P, Vb):
    """O += P V over a 64-key block: four MFMAs of 16 keys, P as f16."""
    P16 = P.astype(H).astype(D)
    for g in range(4):
        o = (o.astype(D) + P16[:, 16 * g:16 * g + 16] @ Vb[16 * g:16 * g + 16].astype(D)).astype(F)
    return o


def restate_wave64(Q, K, V, mut=None):
    """AttWave64 (block0, block, store) for every query of one (sentence, head), queries
    32 w .. 32 w + 31 forming wave w as in attention_lds3 / attention_pp / attention_short.
    Returns (out f16 [L][64], moved bool [L][blocks]: the block moved the query's offset)."""
    L, dh = Q.shape
    assert dh == 64
    Kp, Vp, valid = _keys(K, V, mut, clamp=True)
    nblk = len(Kp) // 64
    rounded = mut != "unrounded_offset"
    qs = (Q * H(sl2_f32(dh))).astype(D)                  # scale_q: f16 products
    o = np.zeros((L, dh), F)
    l = np.zeros((L, 2), F)
    c = np.zeros(L, F)
    moved = np.zeros((L, nblk), bool)
    wave = np.arange(L) // 32
    with np.errstate(over="ignore", invalid="ignore"):
        for blk in range(nblk):
            ks = slice(64 * blk, 64 * blk + 64)
            dot = qs @ Kp[ks].astype(D).T
            if blk == 0:
                s = dot.astype(F)
                s[:, ~valid[ks]] = -np.inf
                m = s.max(axis=1)
                if rounded:
                    m = m.astype(H).astype(F)
                s = (s - m[:, None]).astype(F)
                c = m
                P = np.exp2(s).astype(F)
                l = _half_sums(P)
            else:
                cb = c.astype(H).astype(F)               # set_offset's bias operand (h16)(-c)
                s = (dot - cb[:, None].astype(D)).astype(F)
                s[:, ~valid[ks]] = -np.inf
                P = np.exp2(s).astype(F)
                rs = _half_sums(P)
                trig = (rs > F(1 << ATT_SUMX)).any(axis=1)
                sel = np.isin(wave, wave[trig])          # the ballot: the whole wave redoes the block
                if sel.any():
                    m = s[sel].max(axis=1)
                    cs = c[sel]
                    step = (cs + m).astype(F)
                    if rounded:
                        step = step.astype(H).astype(F)
                    sh = np.where(m > 0, (step - cs).astype(F), F(0)).astype(F)
                    alpha = np.exp2(-sh).astype(F)
                    s[sel] = (s[sel] - sh[:, None]).astype(F)
                    c[sel] = (cs + sh).astype(F)
                    l[sel] = (l[sel] * alpha[:, None]).astype(F)
                    if mut != "skip_rescale":
                        o[sel] = (o[sel] * alpha[:, None]).astype(F)
                    P[sel] = np.exp2(s[sel]).astype(F)
                    rs[sel] = _half_sums(P[sel])
                    moved[sel, blk] = sh != 0
                l = (l + rs).astype(F)
            o = _pv(o, P, Vp[ks])
        inv = (F(1) / (l[:, 0] + l[:, 1]).astype(F)).astype(F)
        return (o * inv[:, None]).astype(F).astype(H), moved


def restate_runmax(Q, K, V, kind, mut=None):
    """The running-max kernels for every query of one (sentence, head): LDS32
    (attention_lds_kernel<32>: Q pre-scaled in f16, v_exp_f32, clamped copies past the end) or
    STREAM (attention_kernel<DH>: the f32 score times sl2, exp2f, zero rows past the end)."""
    L, dh = Q.shape
    Kp, Vp, valid = _keys(K, V, mut, clamp=kind == LDS32)
    sl2 = sl2_f32(dh)
    qs = (Q * H(sl2)).astype(D) if kind == LDS32 else Q.astype(D)
    o = np.zeros((L, dh), F)
    l = np.zeros(L, F)
    m = np.full(L, -np.inf, F)
    with np.errstate(over="ignore", invalid="ignore"):
        for blk in range(len(Kp) // 64):
            ks = slice(64 * blk, 64 * blk + 64)
            s = (qs @ Kp[ks].astype(D).T).astype(F)
            if kind == STREAM:
                s = (s * sl2).astype(F)
            s[:, ~valid[ks]] = -np.inf
            m_new = np.maximum(m, s.max(axis=1))
            alpha = np.exp2((m - m_new).astype(F)).astype(F)
            P = np.exp2((s - m_new[:, None]).astype(F)).astype(F)
            rs = _half_sums(P)
            l = ((l * alpha).astype(F) + (rs[:, 0] + rs[:, 1]).astype(F)).astype(F)
            o = (o * alpha[:, None]).astype(F)
            m = m_new
            o = _pv(o, P, Vp[ks])
        inv = (F(1) / l).astype(F)
        return (o * inv[:, None]).astype(F).astype(H)


def restate_cls(Q, K, V, mut=None):
    """attention_cls_kernel for one (sentence, head): the query is row 0; chunks of 256 keys,
    a key per thread, the fmaf chains, the butterfly sums and the key-group order as written.
    (fmaf is the float64 sum of the exact product and the accumulator rounded to f32: a double
    rounding in rare ties.)  Returns f16 [dh]."""
    L, dh = Q.shape
    NV = dh // 8
    KG = 256 // NV
    Kp, Vp, valid = _keys(K, V, mut if mut != "mask_gt" else None, clamp=False)
    scale = F(F(1.0) / np.sqrt(F(dh)))
    q = Q[0].astype(D)
    m_run, l_run = F(-np.inf), F(0)
    acc = np.zeros((KG, dh), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, L, 256):
            n_c = min(256, L - c0)
            a = np.zeros(n_c, F)
            kk = Kp[c0:c0 + n_c].astype(D)
            for e in range(dh):
                a = (q[e] * kk[:, e] + a.astype(D)).astype(F)
            sc = np.full(256, -np.inf, F)
            sc[:n_c] = (a * scale).astype(F)
            sc[:n_c][~valid[c0:c0 + n_c]] = -np.inf
            m_new = max(m_run, sc.max())
            # __expf(x) = v_exp_f32(x * log2(e))
            p = np.exp2(((sc - m_new).astype(F) * F(LOG2E)).astype(F)).astype(F)
            ps = p.reshape(4, 64).copy()
            for w in (32, 16, 8, 4, 2, 1):
                ps = (ps[:, :w] + ps[:, w:2 * w]).astype(F)
            corr = np.exp2(F(F(m_run - m_new) * F(LOG2E))).astype(F)
            l_run = F(F(l_run * corr) + F(F(ps[0, 0] + ps[1, 0]) + F(ps[2, 0] + ps[3, 0])))
            m_run = m_new
            acc = (acc * corr).astype(F)
            vv = Vp[c0:c0 + n_c].astype(D)
            for k0 in range(0, n_c, KG):
                n = min(KG, n_c - k0)
                acc[:n] = (p[k0:k0 + n, None].astype(D) * vv[k0:k0 + n] + acc[:n].astype(D)).astype(F)
        o = np.zeros(dh, F)
        for g in range(min(KG, L)):
            o = (o + acc[g]).astype(F)
        return (o / l_run).astype(F).astype(H)


def restate(cs, kind, mut=None):
    """The restatement of `kind` over a whole Case: (out f16 [T][d] -- CLS: [n_seqs][d] --,
    moved: per item the [L][blocks] offset moves, WAVE64 only)."""
    if kind == CLS:
        out = np.zeros((len(cs.lens), cs.d), H)
        b = 0
        for r, c, Q, K, V in cs.items():
            out[b // cs.n_head, c] = restate_cls(Q, K, V, mut)
            b += 1
        return out, None
    out = np.zeros((cs.T, cs.d), H)
    moves = []
    for r, c, Q, K, V in cs.items():
        if kind == WAVE64:
            out[r, c], mv = restate_wave64(Q, K, V, mut)
            moves.append(mv)
        else:
            out[r, c] = restate_runmax(Q, K, V, kind, mut)
    return out, moves if kind == WAVE64 else None


def worst_ratio(got, want, bound):
    """max |got - want| / bound; a value that is not finite counts as infinitely far."""
    got = np.asarray(got, D)
    if not np.isfinite(got).all():
        return np.inf
    return float((np.abs(got - want) / bound).max())
