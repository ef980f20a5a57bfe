"""References of the key-count forward tests (bert_hip.h "Key counts"): ColBERT queries whose
[MASK] rows are queries but not attention keys.

TEST INFRASTRUCTURE ONLY.

`KVRefModel.hidden(ids, n_keys)` is ref_forward.RefModel.hidden with every layer's K and V cut
to the sentence's first n_keys rows: all rows are queries and output rows, which is HF's
attention_mask of a right-padded row.  test_cpu_colbert_kv.py pins it on the reference alone
(rows below the count equal the forward of the truncated sentence) and asserts the condition the
GPU test needs of its inputs: on every shape below the masked and the unmasked references
differ, on every row, by at least 5 COS_TOL in 1 - cos, so a forward that ignored the counts
cannot pass the accuracy test.
"""
import numpy as np

import ref_forward
from ref_forward import _gelu, _ln

COS_TOL = 1e-3                 # test_gpu_pooling.COS_TOL (asserted equal by the CPU test)
TINIES = ("tiny32", "tiny64")
# (len, keys): [CLS] [Q] pieces [SEP] then [MASK] up to len
SHAPES = [(4, 3), (32, 5), (64, 4), (100, 40), (128, 65)]


class KVRefModel(ref_forward.RefModel):
    def hidden(self, ids, n_keys=None):
        """Final LayerNorm output of every token of one sentence, float64 [len][n_embd]; only
        the first n_keys rows are attention keys and values (None: all)."""
        if n_keys is None:
            return super().hidden(ids)
        hp, t = self.hp, self.t
        ids = np.asarray(ids, np.int64)
        L, d, H = len(ids), hp["n_embd"], hp["n_head"]
        assert 1 <= n_keys <= L
        dh = d // H
        x = (t["embeddings.word_embeddings.weight"][ids] + t["embeddings.token_type_embeddings.weight"][0] +
             t["embeddings.position_embeddings.weight"][:L])
        x = _ln(x, t["embeddings.LayerNorm.weight"], t["embeddings.LayerNorm.bias"])
        for l in range(hp["n_layer"]):
            p = "encoder.layer.%d." % l
            lin = lambda v, n: v @ t[p + n + ".weight"].T + t[p + n + ".bias"]
            q = lin(x, "attention.self.query").reshape(L, H, dh).transpose(1, 0, 2)
            k = lin(x, "attention.self.key").reshape(L, H, dh).transpose(1, 0, 2)[:, :n_keys]
            v = lin(x, "attention.self.value").reshape(L, H, dh).transpose(1, 0, 2)[:, :n_keys]
            s = q @ k.transpose(0, 2, 1) / np.sqrt(dh)
            s = np.exp(s - s.max(axis=-1, keepdims=True))
            s /= s.sum(axis=-1, keepdims=True)
            a = (s @ v).transpose(1, 0, 2).reshape(L, d)
            x = _ln(x + lin(a, "attention.output.dense"), t[p + "attention.output.LayerNorm.weight"],
                    t[p + "attention.output.LayerNorm.bias"])
            y = lin(_gelu(lin(x, "intermediate.dense")), "output.dense")
            x = _ln(x + y, t[p + "output.LayerNorm.weight"], t[p + "output.LayerNorm.bias"])
        return x


def query_ids(length, keys, n_vocab=692, seed=0):
    """[101, 1, pieces, 102, 103 ...]: keys - 3 seeded pieces, then [MASK] up to length."""
    rng = np.random.default_rng(9000 + 131 * length + keys + seed)
    ids = [101, 1] + [int(x) for x in rng.integers(104, n_vocab, keys - 3)] + [102] + [103] * (length - keys)
    assert len(ids) == length
    return np.array(ids, np.int32)


def queries():
    """(ids list, counts) of SHAPES."""
    return [query_ids(n, k) for n, k in SHAPES], np.array([k for _, k in SHAPES], np.int32)


def one_minus_cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
