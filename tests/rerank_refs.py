"""References, fixtures and bounds of the cross-encoder reranking tests.

TEST INFRASTRUCTURE ONLY.  The reference is tests/ref_forward.RefModel (float64 numpy,
pinned to the oracle for type-0 input by test_cpu_pooling_ref.py) extended here with a
per-token type row and the head tanh(h0 Wp^T + bp) Wc^T + bc.  The oracle has no token
types, so that pin is the only one this code has.

Head fixtures are seeded random: Wp and Wc from N(0, 1/d) (pre-activations and logits
O(1) on O(1) rows), the biases from N(0, 0.1^2).  A saturated tanh hides errors, so every
test that gates a tolerance first checks `unsaturated`: at least 90 % of the reference's
pooler pre-activations have |a| < 2.
"""
import ctypes
import os
import struct

import numpy as np

import bertpy
import ref_forward
import row_kernel_refs as R

F = np.float32
FORMATS = ["f32", "f16", "q4_0", "q4_1", "q8_0"]
QUANT = ["q4_0", "q4_1", "q8_0"]
HEAD = ["pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias"]
TYPE_NAME = "embeddings.token_type_embeddings.weight"
NAN_BITS = np.uint32(0xFFFFFFFF)


def head_tensors(d, n_labels, seed):
    rng = np.random.default_rng(seed)
    s = F(1.0 / np.sqrt(d))
    return {"pooler.dense.weight": rng.standard_normal((d, d), dtype=F) * s,
            "pooler.dense.bias": rng.standard_normal(d, dtype=F) * F(0.1),
            "classifier.weight": rng.standard_normal((n_labels, d), dtype=F) * s,
            "classifier.bias": rng.standard_normal(n_labels, dtype=F) * F(0.1)}


# ---------------------------------------------------------------- model files

def records(path):
    """(offset of the first tensor record, [(name, n_dims, ftype, ne, data offset, n bytes, record offset)])."""
    data = open(path, "rb").read()
    hp = struct.unpack_from("<7i", data, 4)
    p = 32
    for _ in range(hp[0]):
        n, = struct.unpack_from("<i", data, p)
        p += 4 + n
    first, out = p, []
    while p < len(data):
        p0 = p
        nd, nl, tt = struct.unpack_from("<3i", data, p)
        p += 12
        ne = [1, 1]
        for i in range(nd):
            ne[i], = struct.unpack_from("<i", data, p)
            p += 4
        name = data[p:p + nl].decode()
        p += nl
        nbytes = ref_forward._ROW_BYTES[tt](ne[0]) * ne[1]
        out.append((name, nd, tt, tuple(ne), p, nbytes, p0))
        p += nbytes
    return first, out


def tensor_f32(path, name):
    """A tensor as the library dequantizes it (f32 arithmetic, row_kernel_refs.decode_table_f32): [ne1][ne0]."""
    data = open(path, "rb").read()
    for n, _, tt, ne, off, nb, _ in records(path)[1]:
        if n == name:
            return R.decode_table_f32(tt, data[off:off + nb], ne[1], ne[0])
    raise KeyError(name)


def head_f32(path):
    """(Wp [d][d], bp [d], Wc [n_labels][d], bc [n_labels]) in f32, the values the device image holds."""
    wp, bp, wc, bc = (tensor_f32(path, n) for n in HEAD)
    return (np.ascontiguousarray(wp), np.ascontiguousarray(bp.reshape(-1)), np.ascontiguousarray(wc),
            np.ascontiguousarray(bc.reshape(-1)))


def drop_record(src, dst, name):
    """src without the record `name`."""
    data = open(src, "rb").read()
    for n, _, _, _, off, nb, p0 in records(src)[1]:
        if n == name:
            open(dst, "wb").write(data[:p0] + data[off + nb:])
            return dst
    raise KeyError(name)


def swap_type_rows(src, dst):
    """src with the two rows of the token-type table exchanged (whatever the format)."""
    data = bytearray(open(src, "rb").read())
    for n, _, _, ne, off, nb, _ in records(src)[1]:
        if n == TYPE_NAME:
            assert ne[1] == 2
            h = nb // 2
            data[off:off + nb] = data[off + h:off + nb] + data[off:off + h]
            open(dst, "wb").write(bytes(data))
            return dst
    raise KeyError(TYPE_NAME)


def make_head_models(lib, golden, outdir, labels={"tiny32": 1, "tiny64": 3}):
    """{(tiny, fmt): path} of the committed tiny models with a seeded head appended; the q
    formats by bertx_quantize_file from the f16 head file."""
    out = {}
    for k, (tiny, nl) in enumerate(sorted(labels.items())):
        t = head_tensors(64, nl, 50 + k)
        for fmt in ("f32", "f16"):
            out[(tiny, fmt)] = bertpy.append_head(os.path.join(golden, tiny, "ggml-model-%s.bin" % fmt),
                                                  os.path.join(outdir, "%s-head-%s.bin" % (tiny, fmt)), t)
        for fmt in QUANT:
            p = os.path.join(outdir, "%s-head-%s.bin" % (tiny, fmt))
            assert lib.bertx_quantize_file(out[(tiny, "f16")].encode(), p.encode(), bertpy.FTYPE[fmt]) == 0
            out[(tiny, fmt)] = p
    return out


# ---------------------------------------------------------------- the float64 reference

class RerankRef(ref_forward.RefModel):
    """RefModel with token types and the head.  The head's weights are the f32 values the
    library dequantizes (head_f32), widened: the same operands as the device."""

    def __init__(self, path):
        super().__init__(path)
        self.head = tuple(a.astype(np.float64) for a in head_f32(path))

    def hidden(self, ids, types=None):
        if types is None:
            return super().hidden(ids)
        # RefModel adds row 0 of the type table to every token: run it on a private copy of the
        # tables, word row i = word[id_i] + type[ty_i] for token i (ids 0 .. L - 1), type rows zero
        t = self.t
        tab = t[TYPE_NAME]
        types = np.asarray(types, np.int64)
        assert set(np.unique(types)) <= {0, 1}
        word = t["embeddings.word_embeddings.weight"]
        ids = np.asarray(ids, np.int64)
        try:
            self.t = dict(t)
            self.t["embeddings.word_embeddings.weight"] = word[ids] + tab[types]
            self.t[TYPE_NAME] = np.zeros_like(tab)
            return super().hidden(np.arange(len(ids)))
        finally:
            self.t = t

    def head_of(self, h0):
        """(pre-activations, pooler output, logits) of [CLS] rows h0 [n][d]."""
        wp, bp, wc, bc = self.head
        a = np.asarray(h0, np.float64) @ wp.T + bp
        p = np.tanh(a)
        return a, p, p @ wc.T + bc

    def logits(self, ids, types=None):
        return self.head_of(self.hidden(ids, types)[:1])[2][0]


def unsaturated(a):
    """The condition on the reference: at least 90 % of the pooler pre-activations have |a| < 2."""
    return np.mean(np.abs(a) < 2.0) >= 0.9


def head_bound(x, wp, bp, wc, p):
    """Per-logit bound [n][n_labels] of the f32 head against float64 on the same f32 operands,
    first order and doubled: 2 [sum_i |wc_i| (d 2^-24 sum_j |Wp_ij| |x_j| + 2^-21) + d 2^-24
    sum_i |wc_i| |p_i|].  2^-21: eight f32 ulps below 1, for the device tanh."""
    x, wp, wc, p = (np.abs(np.asarray(v, np.float64)) for v in (x, wp, wc, p))
    d = x.shape[1]
    u = d * 2.0 ** -24
    pre = u * (x @ wp.T) + 2.0 ** -21           # [n][d]: the error of each p_i
    return 2.0 * (pre @ wc.T + u * (p @ wc.T))


def run_head(lib, x, wp, bp, wc, bc, pad=5):
    """bertx_test_head on x [n][d]: (logits [n][n_labels], the rows behind them)."""
    x = np.ascontiguousarray(x, F)
    n, d = x.shape
    nl = wc.shape[0]
    out = np.full((n + pad, nl), np.nan, F)
    out.view(np.uint32)[:] = NAN_BITS
    rc = lib.bertx_test_head(x.ctypes.data, n, d, wp.ctypes.data, bp.ctypes.data, wc.ctypes.data, bc.ctypes.data, nl,
                             out.ctypes.data, n + pad)
    assert rc == 0, rc
    return out[:n], out[n:]


# ---------------------------------------------------------------- inputs

def pair_ids(n_vocab, la, lb, rng):
    """(ids, types) of a pair with la and lb pieces: la + lb + 3 tokens."""
    a, b = rng.integers(104, n_vocab, la), rng.integers(104, n_vocab, lb)
    ids = np.concatenate([[101], a, [102], b, [102]]).astype(np.int32)
    types = np.concatenate([np.zeros(la + 2), np.ones(lb + 1)]).astype(np.int32)
    return ids, types


def pairs_of_lengths(n_vocab, lens, seed):
    """Mixed-type pairs of the given total lengths (>= 3), A about two fifths of the pieces."""
    rng = np.random.default_rng(seed)
    out = []
    for L in lens:
        la = (L - 3) * 2 // 5
        out.append(pair_ids(n_vocab, la, L - 3 - la, rng))
    return [p[0] for p in out], [p[1] for p in out]


# ---------------------------------------------------------------- device calls

class Hip:
    """The HIP runtime libbert.so is linked against, by soname (the process already holds it)."""

    def __init__(self):
        h = ctypes.CDLL("libamdhip64.so.7")
        vp = ctypes.c_void_p
        h.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
        h.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        h.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
        h.hipMemset.argtypes = [vp, ctypes.c_int, ctypes.c_size_t]
        h.hipStreamSynchronize.argtypes = [vp]
        h.hipFree.argtypes = [vp]
        h.hipStreamDestroy.argtypes = [vp]
        self.h = h

    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.h.hipMalloc(ctypes.byref(p), max(int(nbytes), 16)) == 0
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        assert self.h.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def download(self, p, shape, dtype=F):
        out = np.zeros(shape, dtype)
        assert self.h.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def stream(self):
        s = ctypes.c_void_p()
        assert self.h.hipStreamCreate(ctypes.byref(s)) == 0
        return s


class DeviceBatch:
    """A batch resident on the GPU for the device entries: ids, types, cu, one output buffer
    large enough for every kind, one stream.  Free with close()."""

    POOLED, TOKENS, LOGITS = 0, 1, 2

    def __init__(self, hip, m, ids, types=None):
        self.hip, self.m = hip, m
        self.lens = [len(x) for x in ids]
        self.cu = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        self.T, self.B, self.max_len = int(self.cu[-1]), len(ids), max(self.lens)
        self.d_ids = hip.upload(np.concatenate(ids).astype(np.int32))
        self.d_types = hip.upload(np.concatenate(types).astype(np.int32)) if types is not None else None
        self.d_cu = hip.upload(self.cu)
        self.d_out = hip.malloc(self.T * m.n_embd * 4)
        self.s = hip.stream()
        assert m.lib.bertx_reserve(m.ctx, 0, self.T, self.B) == 0

    def shape(self, kind):
        return {0: (self.B, self.m.n_embd), 1: (self.T, self.m.n_embd), 2: (self.B, max(self.m.n_labels, 1))}[kind]

    def _finish(self, rc, kind):
        assert rc == 0, rc
        assert self.hip.h.hipStreamSynchronize(self.s) == 0
        return self.hip.download(self.d_out, self.shape(kind))

    def ex(self, kind, types=True):
        """bertx_forward_device_ex (types False: a NULL types pointer)."""
        self.hip.h.hipMemset(self.d_out, 0xFF, self.T * self.m.n_embd * 4)
        rc = self.m.lib.bertx_forward_device_ex(self.m.ctx, 0, self.d_ids, self.d_types if types else None, self.d_cu,
                                                self.B, self.max_len, self.T, kind, self.d_out, self.s)
        return self._finish(rc, kind)

    def old(self, kind):
        """bertx_forward_device / bertx_forward_tokens_device."""
        fn = self.m.lib.bertx_forward_tokens_device if kind == 1 else self.m.lib.bertx_forward_device
        self.hip.h.hipMemset(self.d_out, 0xFF, self.T * self.m.n_embd * 4)
        return self._finish(fn(self.m.ctx, 0, self.d_ids, self.d_cu, self.B, self.max_len, self.T, self.d_out, self.s),
                            kind)

    def cls_rows(self, tokens):
        return tokens[self.cu[:-1]]

    def close(self):
        for p in (self.d_ids, self.d_types, self.d_cu, self.d_out):
            if p is not None:
                self.hip.h.hipFree(p)
        self.hip.h.hipStreamDestroy(self.s)
