"""A float64 numpy forward of a model file: the reference for what the oracle cannot
return ([CLS] pooling, per-token hidden states).

TEST INFRASTRUCTURE ONLY.  Reads the model file itself (layout: bertpy.write_model /
bertpy.tensor_names; q4_0 / q4_1 / q8_0 blocks dequantized per oracle/ggml_era.h) and
runs the era's graph (bert.cpp:963-1095) in float64: position + type-0 + word
embeddings, LayerNorm eps 1e-5, scores / sqrt(dh), tanh GELU, post-LN residuals.
tests/test_cpu_pooling_ref.py pins its mean-pooled output to the oracle.
"""
import struct

import numpy as np

QK = 32


def _dequant(raw, ttype, ne0, ne1):
    """File bytes of a tensor [ne1][ne0] -> float64 array."""
    n = ne0 * ne1
    if ttype == 0:
        return np.frombuffer(raw, "<f4", n).astype(np.float64).reshape(ne1, ne0)
    if ttype == 1:
        return np.frombuffer(raw, "<f2", n).astype(np.float64).reshape(ne1, ne0)
    nb = n // QK
    if ttype == 2:     # {f16 d; u8 qs[16]}: element j = low nibble of qs[j], j + 16 = high; x = (q - 8) d
        b = np.frombuffer(raw, np.uint8, nb * 18).reshape(nb, 18)
        d = b[:, :2].copy().view("<f2").astype(np.float64)
        qs = b[:, 2:]
        q = np.concatenate([qs & 15, qs >> 4], axis=1).astype(np.float64)
        return ((q - 8.0) * d).reshape(ne1, ne0)
    if ttype == 3:     # {f16 d; f16 m; u8 qs[16]}: x = q d + m
        b = np.frombuffer(raw, np.uint8, nb * 20).reshape(nb, 20)
        d = b[:, :2].copy().view("<f2").astype(np.float64)
        m = b[:, 2:4].copy().view("<f2").astype(np.float64)
        qs = b[:, 4:]
        q = np.concatenate([qs & 15, qs >> 4], axis=1).astype(np.float64)
        return (q * d + m).reshape(ne1, ne0)
    if ttype == 8:     # {f16 d; i8 qs[32]}: x = q d
        b = np.frombuffer(raw, np.uint8, nb * 34).reshape(nb, 34)
        d = b[:, :2].copy().view("<f2").astype(np.float64)
        q = b[:, 2:].copy().view(np.int8).astype(np.float64)
        return (q * d).reshape(ne1, ne0)
    raise ValueError("unknown tensor type %d" % ttype)


_ROW_BYTES = {0: lambda k: 4 * k, 1: lambda k: 2 * k, 2: lambda k: k // QK * 18, 3: lambda k: k // QK * 20,
              8: lambda k: k // QK * 34}


def load_model(path):
    """(hparams dict, {tensor name: float64 array})."""
    data = open(path, "rb").read()
    magic, = struct.unpack_from("<I", data, 0)
    assert magic == 0x67676D6C, hex(magic)
    keys = ("n_vocab", "n_max_tokens", "n_embd", "n_intermediate", "n_head", "n_layer", "ftype")
    hp = dict(zip(keys, struct.unpack_from("<7i", data, 4)))
    p = 32
    for _ in range(hp["n_vocab"]):
        n, = struct.unpack_from("<i", data, p)
        p += 4 + n
    tensors = {}
    while p < len(data):
        nd, nl, tt = struct.unpack_from("<3i", data, p)
        p += 12
        ne = [1, 1]
        for i in range(nd):
            ne[i], = struct.unpack_from("<i", data, p)
            p += 4
        name = data[p:p + nl].decode()
        p += nl
        nbytes = _ROW_BYTES[tt](ne[0]) * ne[1]
        a = _dequant(data[p:p + nbytes], tt, ne[0], ne[1])
        p += nbytes
        tensors[name] = a if nd == 2 else a.reshape(-1)
    return hp, tensors


def _ln(x, g, b):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + np.tanh(0.79788456080286535587989211986876 * x * (1.0 + 0.044715 * x * x)))


class RefModel:
    def __init__(self, path):
        self.hp, self.t = load_model(path)

    def hidden(self, ids):
        """Final LayerNorm output of every token of one sentence: float64 [len][n_embd]."""
        hp, t = self.hp, self.t
        ids = np.asarray(ids, np.int64)
        L, d, H = len(ids), hp["n_embd"], hp["n_head"]
        dh = d // H
        x = (t["embeddings.word_embeddings.weight"][ids] + t["embeddings.token_type_embeddings.weight"][0] +
             t["embeddings.position_embeddings.weight"][:L])
        x = _ln(x, t["embeddings.LayerNorm.weight"], t["embeddings.LayerNorm.bias"])
        for l in range(hp["n_layer"]):
            p = "encoder.layer.%d." % l
            lin = lambda v, n: v @ t[p + n + ".weight"].T + t[p + n + ".bias"]
            q = lin(x, "attention.self.query").reshape(L, H, dh).transpose(1, 0, 2)
            k = lin(x, "attention.self.key").reshape(L, H, dh).transpose(1, 0, 2)
            v = lin(x, "attention.self.value").reshape(L, H, dh).transpose(1, 0, 2)
            s = q @ k.transpose(0, 2, 1) / np.sqrt(dh)
            s = np.exp(s - s.max(axis=-1, keepdims=True))
            s /= s.sum(axis=-1, keepdims=True)
            a = (s @ v).transpose(1, 0, 2).reshape(L, d)
            x = _ln(x + lin(a, "attention.output.dense"), t[p + "attention.output.LayerNorm.weight"],
                    t[p + "attention.output.LayerNorm.bias"])
            y = lin(_gelu(lin(x, "intermediate.dense")), "output.dense")
            x = _ln(x + y, t[p + "output.LayerNorm.weight"], t[p + "output.LayerNorm.bias"])
        return x

    def hidden_batch(self, ids_list):
        return [self.hidden(i) for i in ids_list]


def _l2(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def mean_pool(hidden_list):
    """The default embeddings: per-sentence mean of the rows, L2-normalised."""
    return np.stack([_l2(h.mean(axis=0)) for h in hidden_list])


def cls_pool(hidden_list):
    """[CLS] embeddings: the first row, L2-normalised."""
    return np.stack([_l2(h[0]) for h in hidden_list])
