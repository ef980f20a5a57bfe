"""References of the SPLADE sparse head (bert_hip.h "Sparse"): a float64 restatement of its
arithmetic on the f16 operands the kernels multiply, the bounds the GPU tests hold it to,
seeded model files with the masked-LM head records, and the planted decoder cases."""
import math
import os

import numpy as np

import bertpy
import rerank_refs as RR

F = np.float32
U = 2.0 ** -24
WORD = "embeddings.word_embeddings.weight"
_erf = np.vectorize(math.erf, otypes=[np.float64])


def transform_ref(x, Wt, bt, gamma, beta, dt=np.float64):
    """h before its f16 rounding, [T][d], in dtype dt on the f16-rounded x and Wt.  dt float32:
    the plain restatement whose distance from float64 is the f32 term of transform_tol."""
    a, W = x.astype(np.float16).astype(dt), Wt.astype(np.float16).astype(dt)
    u = a @ W.T + bt.astype(dt)
    g = (dt(0.5) * u * (dt(1) + _erf(u * dt(0.70710678)).astype(dt))).astype(dt)
    c = g - g.mean(axis=1, keepdims=True, dtype=dt)
    rstd = dt(1) / np.sqrt((c * c).mean(axis=1, keepdims=True, dtype=dt) + dt(1e-5))
    return (c * rstd * gamma.astype(dt) + beta.astype(dt)).astype(dt)


def ulp16(v):
    """The spacing of f16 at |v| (subnormal spacing below 2^-14)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def transform_tol(h64, h32):
    """Per element: one f16 ulp of the reference value (the rounding of h, which may fall on the
    other side of a tie) plus 4 x what the float32 restatement loses against float64 at this
    shape (the margin for the kernel's other summation order)."""
    return ulp16(h64) + 4.0 * float(np.abs(h32.astype(np.float64) - h64).max())


def decoder_ref(h, E, b, cu):
    """(w [S][V] float64, m [S][V] the pooled logit + bias, bound [S][V]) from exact-f16 h
    [T][d] and E [V][d]: bound = (d + 8) U sum_k |h_k E_vk| at the arg-max row plus two f32
    ulps each of m and w (the bias add and log1pf; log1p is 1-Lipschitz)."""
    h, E = h.astype(np.float64), E.astype(np.float64)
    l = h @ E.T + b.astype(np.float64)
    mag = np.abs(h) @ np.abs(E).T
    d, S = h.shape[1], len(cu) - 1
    m, bound = np.zeros((S, E.shape[0])), np.zeros((S, E.shape[0]))
    for s in range(S):
        seg = l[cu[s]:cu[s + 1]]
        arg = seg.argmax(axis=0)
        m[s] = seg.max(axis=0)
        bound[s] = (d + 8) * U * mag[cu[s]:cu[s + 1]][arg, np.arange(E.shape[0])]
    w = np.log1p(np.maximum(m, 0.0))
    return w, m, bound + 4 * U * (np.abs(m) + w)


def decoder_naive(h, E, b, cu):
    """SPLADE as published: log(1 + relu(logit)) per token, then the max over the sentence."""
    l = np.log1p(np.maximum(h.astype(np.float64) @ E.astype(np.float64).T + b, 0.0))
    return np.stack([l[cu[s]:cu[s + 1]].max(axis=0) for s in range(len(cu) - 1)])


class DecoderCase:
    """Exact-f16 h [T][d] and E [V][d] with planted logits.  Channel 0 feeds the terms v % 4
    == 0 and holds a descending chain F_0 > T_0 > F_1 > T_1 .. (F_s in sentence s's first
    row, T_s in its last row): a sentence's max is in its first row, and the row before it,
    the neighbour's last, holds a larger value.  Channel 1 feeds v % 4 == 1 with the
    ascending mirror image (the max in the last row, a larger value in the next sentence's
    first row).  Channel 2 feeds v % 4 == 2 with -64 in every row of the even sentences: all
    their logits there are negative.  The other channels are noise of |logit| < 1."""

    def __init__(self, d, V, lens, seed):
        rng = np.random.default_rng(seed)
        self.cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        T, S = int(self.cu[-1]), len(lens)
        h = (rng.standard_normal((T, d)) / 32).astype(np.float16)
        E = (rng.standard_normal((V, d)) / 32).astype(np.float16)
        h[:, :3] = 0
        E[:, :3] = 0
        for c in range(3):
            E[c::4, c] = 1
        for s in range(S):
            first, last = self.cu[s], self.cu[s + 1] - 1
            h[first, 0] = 32 + 2 * (S - s)
            h[last, 1] = 32 + 2 * s
            if last > first:
                h[last, 0] = 32 + 2 * (S - s) - 1
                h[first, 1] = 32 + 2 * s - 1
            if s % 2 == 0:
                h[first:last + 1, 2] = -64
        self.h, self.E = h, E
        self.b = (rng.uniform(-0.1, 0.1, V)).astype(F)
        self.neg = [(s, v) for s in range(0, S, 2) for v in range(2, V, 4)]


def run_sparse(lib, mode, out_rows, width, dtype, x=None, Wt=None, bt=None, gamma=None, beta=None, h=None, E=None,
               b=None, cu=None):
    """bertx_test_sparse on out_rows rows of NaN bits; returns the whole output."""
    c = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    x, Wt, bt, gamma, beta, E, b = (c(a, F) for a in (x, Wt, bt, gamma, beta, E, b))
    h, cu = c(h, np.float16), c(cu, np.int32)
    src = x if x is not None else h
    out = np.frombuffer(bytearray(b"\xff" * (out_rows * width * np.dtype(dtype).itemsize)), dtype).reshape(out_rows, width)
    p = lambda a: None if a is None else a.ctypes.data
    rc = lib.bertx_test_sparse(mode, p(x), src.shape[0], src.shape[1], p(Wt), p(bt), p(gamma), p(beta), p(h), p(E),
                               0 if E is None else E.shape[0], p(b), p(cu), 0 if cu is None else len(cu) - 1,
                               out.ctypes.data, out_rows)
    assert rc == 0, rc
    return out


def mlm_tensors(d, n_vocab, seed):
    rng = np.random.default_rng(seed)
    return {bertpy.MLM_NAMES[0]: (rng.standard_normal((d, d)) / np.sqrt(d)).astype(F),
            bertpy.MLM_NAMES[1]: (0.1 * rng.standard_normal(d)).astype(F),
            bertpy.MLM_NAMES[2]: (1 + 0.1 * rng.standard_normal(d)).astype(F),
            bertpy.MLM_NAMES[3]: (0.1 * rng.standard_normal(d)).astype(F),
            bertpy.MLM_NAMES[4]: (0.5 * rng.standard_normal(n_vocab)).astype(F)}


def make_sparse_models(lib, golden, outdir, tiny="tiny64"):
    """{fmt: path} of a committed tiny model with a seeded masked-LM head appended; the q
    formats by bertx_quantize_file from the f16 file."""
    out = {}
    n_vocab = RR.tensor_f32(os.path.join(golden, tiny, "ggml-model-f32.bin"), WORD).shape[0]
    for fmt in ("f32", "f16"):
        out[fmt] = bertpy.append_mlm_head(os.path.join(golden, tiny, "ggml-model-%s.bin" % fmt),
                                          os.path.join(outdir, "%s-mlm-%s.bin" % (tiny, fmt)), mlm_tensors(64, n_vocab, 90))
    for fmt in RR.QUANT:
        out[fmt] = os.path.join(outdir, "%s-mlm-%s.bin" % (tiny, fmt))
        assert lib.bertx_quantize_file(out["f16"].encode(), out[fmt].encode(), bertpy.FTYPE[fmt]) == 0
    return out


def head_f32(path):
    """(Wt, bt, gamma, beta, E, b) in f32 as the library dequantizes the file's records."""
    t = [np.ascontiguousarray(RR.tensor_f32(path, n)) for n in bertpy.MLM_NAMES[:4] + [WORD, bertpy.MLM_NAMES[4]]]
    return t[0], t[1].reshape(-1), t[2].reshape(-1), t[3].reshape(-1), t[4], t[5].reshape(-1)
