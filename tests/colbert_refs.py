"""References, fixtures and bounds of the ColBERT tests (the projection record, the
[Q] / [D] tokenisation, the fused projector).

TEST INFRASTRUCTURE ONLY.

Projection fixtures are seeded: W = standard_normal / sqrt(d), so a projected element of an
O(1) LayerNorm row is O(1) and ||p|| is about sqrt(dim).  Every test that gates a tolerance
runs on inputs whose reference rows satisfy `well_scaled`: ||p||_2 >= 0.1 sqrt(dim)
(test_cpu_colbert.py checks this on the same seeds, so the reference alone satisfies it).

The bounds (U = 2^-24, the f32 unit roundoff):

  p_j.  The operands a_k = f16(x_k) and w_jk = f16(W_jk) are the same exact values on both
  sides; a product of two f16 values has at most 22 significant bits and is exact in f32.
  The device adds the d products to an f32 accumulator in ascending blocks of 32; whatever
  the order inside a block, a sum of d terms takes at most d roundings, each relative U to
  a partial sum no larger than S_j = sum_k |a_k w_jk|.  First order that is d U S_j; the 8
  covers the second-order terms ((1 + U)^d - 1 - d U < 8 U for d <= 1024):
      |dp_j| <= E_j = (d + 8) U S_j.

  out_j = p_j / ||p||.  With n = ||p||_2 of the exact p: the error of p_j contributes
  E_j / n, the error of the norm |out_j| ||E||_2 / n (Cauchy-Schwarz on sum p_j dp_j / n),
  and the roundings of the squares (1), of the dim - 1 + 2 adds of the square sum (halved
  by the square root), of the square root, the division and the final product (3) at most
  (dim / 2 + 5) U < (dim + 8) U relative:
      |dout_j| <= (E_j + |out_j| ||E||_2) / n + (dim + 8) U |out_j|.
"""
import os
import string

import numpy as np

import bertpy
import rerank_refs as RR
import row_kernel_refs as R

F, D = np.float32, np.float64
U = 2.0 ** -24
NAN_BITS = np.uint32(0xFFFFFFFF)
PUNCT = set(string.punctuation)
DIMS = {"tiny32": 32, "tiny64": 64}      # tiny32: width 64 with 32 padded columns
REC = "linear.weight"


def width_of(dim):
    return (dim + 63) // 64 * 64


def proj_weight(d, dim, seed):
    return (np.random.default_rng(seed).standard_normal((dim, d)) / np.sqrt(d)).astype(F)


# ---------------------------------------------------------------- model files

def make_proj_models(lib, golden, outdir, head=False):
    """{(tiny, fmt): path} of the committed tiny models with a seeded projection appended (and,
    head, a seeded classification head before it); the q formats by bertx_quantize_file from
    the f16 file, as rerank_refs.make_head_models makes them."""
    out = {}
    for k, (tiny, dim) in enumerate(sorted(DIMS.items())):
        W = proj_weight(64, dim, 70 + k)
        for fmt in ("f32", "f16"):
            src = os.path.join(golden, tiny, "ggml-model-%s.bin" % fmt)
            if head:
                src = bertpy.append_head(src, os.path.join(outdir, "%s-h-%s.bin" % (tiny, fmt)),
                                         RR.head_tensors(64, 3, 50 + k))
            out[(tiny, fmt)] = bertpy.append_projection(src, os.path.join(outdir, "%s-proj-%s.bin" % (tiny, fmt)), W)
        for fmt in RR.QUANT:
            p = os.path.join(outdir, "%s-proj-%s.bin" % (tiny, fmt))
            assert lib.bertx_quantize_file(out[(tiny, "f16")].encode(), p.encode(), bertpy.FTYPE[fmt]) == 0
            out[(tiny, fmt)] = p
    return out


def proj_f32(path):
    """linear.weight [dim][d] in f32 as the library dequantizes it."""
    return np.ascontiguousarray(RR.tensor_f32(path, REC))


# ---------------------------------------------------------------- tokenisation

def pieces(m, text):
    """bert_tokenize of the text alone (no token limit), without its [CLS] / [SEP]."""
    ids, n = m.tokenize(text, n_max_tokens=4096)
    assert n == len(ids) and ids[0] == 101 and ids[-1] == 102
    return list(ids[1:-1])


def restated_colbert(m, text, kind, maxlen):
    """(ids, keep): bertx_tokenize_colbert transcribed."""
    p = pieces(m, text)[:maxlen - 3]
    ids = [101, 1 if kind == 0 else 2] + p + [102]
    if kind == 0:
        ids += [103] * (maxlen - len(ids))
        return ids, [1] * len(ids)
    keep = [0 if m.id_to_token(i).decode("utf-8", "replace") in PUNCT else 1 for i in ids]
    return ids, keep


# ---------------------------------------------------------------- the projector

class ProjCase:
    """Operands of one kernel shape: T rows of the LN-fold stream (mode 0: z f16, statistics,
    gamma, beta as row_kernel_refs.stream_rows makes them) or of f32 rows (mode 1), and W."""

    def __init__(self, d, dim, T, seed):
        self.d, self.dim, self.T, self.width = d, dim, T, width_of(dim)
        rng = np.random.default_rng(seed)
        self.W = proj_weight(d, dim, seed + 1)
        y, self.g, self.b = R.stream_rows(T, d, rng)
        mean, r = R.ln_ref(y)
        self.z = np.ascontiguousarray((y * self.g).astype(np.float16))
        self.stats = np.ascontiguousarray(np.stack([mean, r], axis=1).astype(F))
        self.x32 = np.ascontiguousarray(rng.standard_normal((T, d)).astype(F) * F(1.5))

    def ln_f64(self):
        """The mode-0 rows in float64 from the values the kernel reads (never the device's bits:
        for conditions on the reference only)."""
        z, m, r = self.z.astype(D), self.stats[:, :1].astype(D), self.stats[:, 1:].astype(D)
        return r * z - r * m * self.g.astype(D) + self.b.astype(D)


def project_ref(x, W):
    """Float64 reference on the device's operands: x f32 [T][d] (the rows the kernel rounds to
    f16), W f32 [dim][d].  Returns (p, out, E, bound): the exact products' sums, the unit
    rows, and the two bounds of the module docstring, [T][dim]."""
    a = np.asarray(x, F).astype(np.float16).astype(D)
    w = np.asarray(W, F).astype(np.float16).astype(D)
    d, dim = a.shape[1], w.shape[0]
    p = a @ w.T
    E = (d + 8) * U * (np.abs(a) @ np.abs(w).T)
    n = np.linalg.norm(p, axis=1, keepdims=True)
    out = p / n
    bound = (E + np.abs(out) * np.linalg.norm(E, axis=1, keepdims=True)) / n + (dim + 8) * U * np.abs(out)
    return p, out, E, bound


def well_scaled(p):
    """The condition on the reference: every row's ||p||_2 >= 0.1 sqrt(dim)."""
    return bool(np.all(np.linalg.norm(p, axis=1) >= 0.1 * np.sqrt(p.shape[1])))


def nan_rows(rows, width):
    out = np.zeros((rows, width), F)
    out.view(np.uint32)[:] = NAN_BITS
    return out


def run_project(lib, mode, src, stats, g, b, W, rows=None, pad=5, out_rows=None):
    """bertx_test_project: (rc, rows it owns, the rows behind them)."""
    T, d = src.shape
    dim = W.shape[0]
    n_out = T if rows is None else len(rows)
    total = n_out + pad if out_rows is None else out_rows
    out = nan_rows(max(total, 1), width_of(dim))
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    W = np.ascontiguousarray(W, F)
    rc = lib.bertx_test_project(mode, R.ptr(src), None if stats is None else R.ptr(stats),
                                None if g is None else R.ptr(g), None if b is None else R.ptr(b), T, d, R.ptr(W), dim,
                                None if rows is None else R.ptr(rows), n_out, R.ptr(out), total)
    return rc, out[:n_out], out[n_out:]


def run_case(lib, case, mode, T=None, rows=None, pad=5):
    T = case.T if T is None else T
    if mode == 0:
        rc, out, tail = run_project(lib, 0, case.z[:T], case.stats[:T], case.g, case.b, case.W, rows, pad)
    else:
        rc, out, tail = run_project(lib, 1, case.x32[:T], None, None, None, case.W, rows, pad)
    assert rc == 0, rc
    assert np.all(tail.view(np.uint32) == NAN_BITS), "rows behind n_out were written"
    return out


def tokens_on_device(lib, case):
    """The BERTX_OUT_TOKENS expression of the case's mode-0 rows, from the library's own
    per-token kernel (bertx_test_pool kind 3): the exact bits x of the contract."""
    out = np.zeros((case.T, case.d), F)
    rc = lib.bertx_test_pool(3, R.ptr(case.z), R.ptr(case.stats), R.ptr(case.g), R.ptr(case.b), None, 0, 0, case.T,
                             case.d, R.ptr(out), case.T)
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------- the forward

class ProjBatch(RR.DeviceBatch):
    """DeviceBatch with the projected output: BERTX_OUT_PROJ through bertx_forward_device_ex
    and bertx_forward_project_device with a row map."""

    PROJ = 3

    def __init__(self, hip, m, ids):
        super().__init__(hip, m, ids)
        self.width = m.proj_width
        self.d_proj = hip.malloc(max(self.T, 1) * max(self.width, 64) * 4)

    def proj(self):
        self.hip.h.hipMemset(self.d_proj, 0xFF, self.T * max(self.width, 64) * 4)
        rc = self.m.lib.bertx_forward_device_ex(self.m.ctx, 0, self.d_ids, None, self.d_cu, self.B, self.max_len, self.T,
                                                self.PROJ, self.d_proj, self.s)
        assert rc == 0, rc
        assert self.hip.h.hipStreamSynchronize(self.s) == 0
        return self.hip.download(self.d_proj, (self.T, self.width))

    def proj_rows(self, rows):
        rows = np.ascontiguousarray(rows, np.int32)
        d_rows = self.hip.upload(rows)
        self.hip.h.hipMemset(self.d_proj, 0xFF, self.T * max(self.width, 64) * 4)
        rc = self.m.lib.bertx_forward_project_device(self.m.ctx, 0, self.d_ids, None, self.d_cu, self.B, self.max_len,
                                                     self.T, d_rows, len(rows), self.d_proj, self.s)
        assert rc == 0, rc
        assert self.hip.h.hipStreamSynchronize(self.s) == 0
        out = self.hip.download(self.d_proj, (self.T, self.width))
        self.hip.h.hipFree(d_rows)
        return out[:len(rows)], out[len(rows):]

    def close(self):
        self.hip.h.hipFree(self.d_proj)
        super().close()
