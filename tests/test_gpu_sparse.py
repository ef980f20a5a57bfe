"""GPU tests of the SPLADE sparse head (sparse.hip): the decoder with its fused segmented max
and the transform alone through bertx_test_sparse, and BERTX_OUT_SPARSE end to end under
every chain.  References, planted cases and bounds: sparse_refs.py."""
import ctypes
import os

import numpy as np
import pytest

import bertpy
import rerank_refs as RR
import sparse_refs as SR
from row_kernel_refs import bits

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POOLED, TOKENS, SPARSE = 0, 1, 4
CHAINS = [("f16", None), ("f32", None), ("q4_0", None), ("q8_0", "q8")]
LENS = [[1], [15, 16, 17], [130], [3, 200, 1, 60]]


@pytest.fixture(autouse=True)
def _one_device(monkeypatch):
    monkeypatch.delenv("BERT_HOST_ONLY", raising=False)
    monkeypatch.setenv("BERT_DEVICES", "0")


@pytest.fixture(scope="module")
def models(lib, tmp_path_factory):
    return SR.make_sparse_models(lib, GOLDEN, str(tmp_path_factory.mktemp("mlm")))


@pytest.fixture(scope="module")
def hip():
    return RR.Hip()


@pytest.mark.parametrize("lens", LENS, ids=lambda l: "-".join(map(str, l)))
@pytest.mark.parametrize("V", [1, 130, 1027])
@pytest.mark.parametrize("d", [64, 128, 768])
def test_decoder_segmented_max(lib, d, V, lens):
    case = SR.DecoderCase(d, V, lens, 1000 + d + V + len(lens))
    S = len(lens)
    got = SR.run_sparse(lib, 1, S + 3, V, F, h=case.h, E=case.E, b=case.b, cu=case.cu)   # (-5: a guard row was written)
    assert np.all(got[S:].view(np.uint32) == 0xFFFFFFFF)
    w, m, bound = SR.decoder_ref(case.h, case.E, case.b, case.cu)
    for s, v in case.neg:
        assert got[s, v:v + 1].view(np.uint32)[0] == 0, (s, v)
    assert np.all(got[:S] >= 0) and not np.signbit(got[:S]).any()
    ratio = float((np.abs(got[:S].astype(np.float64) - w) / bound).max())
    print("decoder d %d V %d lens %s: worst |dw| / bound = %.4f" % (d, V, lens, ratio))
    assert ratio <= 1.0, ratio


_tf = {}   # d -> (operands, float64 h, tolerance)


def transform_case(d):
    """129 rows per width, shared by the row counts and never changed."""
    if d not in _tf:
        rng = np.random.default_rng(2000 + d)
        a = dict(x=rng.standard_normal((129, d)).astype(F), Wt=(rng.standard_normal((d, d)) / np.sqrt(d)).astype(F),
                 bt=(0.1 * rng.standard_normal(d)).astype(F), gamma=(1 + 0.1 * rng.standard_normal(d)).astype(F),
                 beta=(0.1 * rng.standard_normal(d)).astype(F))
        h64 = SR.transform_ref(**a)
        _tf[d] = (a, h64, SR.transform_tol(h64, SR.transform_ref(dt=np.float32, **a)))
    return _tf[d]


@pytest.mark.parametrize("T", [1, 17, 129])
@pytest.mark.parametrize("d", [64, 384, 1024])
def test_transform(lib, d, T):
    a, h64, tol = transform_case(d)
    got = SR.run_sparse(lib, 0, T + 2, d, np.float16, **dict(a, x=a["x"][:T]))
    assert np.all(got[T:].view(np.uint16) == 0xFFFF)
    err = np.abs(got[:T].astype(np.float64) - h64[:T])
    ratio = float((err / tol[:T]).max())
    print("transform d %d T %d: worst |dh| / tol = %.4f, f32 term %.3g" % (d, T, ratio, float((tol - SR.ulp16(h64)).max())))
    assert ratio <= 1.0, ratio


class SparseBatch(RR.DeviceBatch):
    """DeviceBatch with an output buffer that also holds [B][n_vocab]."""
    def __init__(self, hip, m, ids):
        super().__init__(hip, m, ids)
        self.V = m.hparams()[0]
        hip.h.hipFree(self.d_out)
        self.nbytes = 4 * max(self.T * m.n_embd, self.B * self.V)
        self.d_out = hip.malloc(self.nbytes)

    def run(self, kind):
        self.hip.h.hipMemset(self.d_out, 0xFF, self.nbytes)
        rc = self.m.lib.bertx_forward_device_ex(self.m.ctx, 0, self.d_ids, None, self.d_cu, self.B, self.max_len, self.T,
                                                kind, self.d_out, self.s)
        assert rc == 0, rc
        assert self.hip.h.hipStreamSynchronize(self.s) == 0
        shape = {POOLED: (self.B, self.m.n_embd), TOKENS: (self.T, self.m.n_embd), SPARSE: (self.B, self.V)}[kind]
        return self.hip.download(self.d_out, shape)


def ragged(n_vocab, lens, seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([[101], rng.integers(104, n_vocab, L - 2), [102]]).astype(np.int32) for L in lens]


@pytest.mark.parametrize("fmt,act", CHAINS)
def test_sparse_output(lib, models, hip, fmt, act):
    """BERTX_OUT_SPARSE is, bit for bit, the whole head (mode 2) on that run's TOKENS rows and the
    file's records as the library dequantizes them; every replay of the captured forward repeats the
    eager bits; a sentence alone gives its row of the ragged batch; the host form agrees."""
    m = bertpy.BertModel(models[fmt], act=act)
    V = m.sparse_width
    assert V == m.hparams()[0]
    ids = ragged(V, [5, 140, 3, 33], 5)
    db = SparseBatch(hip, m, ids)
    eager = db.run(SPARSE)
    Wt, bt, gamma, beta, E, b = SR.head_f32(models[fmt])
    want = SR.run_sparse(lib, 2, db.B, V, F, x=db.run(TOKENS), Wt=Wt, bt=bt, gamma=gamma, beta=beta, E=E, b=b, cu=db.cu)
    assert np.array_equal(bits(eager), bits(want))
    assert (eager > 0).any() and (eager == 0).any()
    for _ in range(3):   # (the second use of a shape captures it, the later ones replay)
        assert np.array_equal(bits(db.run(SPARSE)), bits(eager))
    db.close()
    for i in (1, 2):
        one = SparseBatch(hip, m, ids[i:i + 1])
        assert np.array_equal(bits(one.run(SPARSE)), bits(eager[i:i + 1])), i
        one.close()
    assert np.array_equal(bits(m.forward_sparse(ids)), bits(eager))


def test_file_without_the_records(lib, models, hip):
    """-6 from the sparse entries with the output untouched; the records change no other output."""
    plain = bertpy.BertModel(os.path.join(GOLDEN, "tiny64", "ggml-model-f16.bin"))
    m = bertpy.BertModel(models["f16"])
    ids = ragged(plain.hparams()[0], [5, 9], 1)
    assert plain.sparse_width == 0
    db, dm = SparseBatch(hip, plain, ids), SparseBatch(hip, m, ids)
    assert lib.bertx_forward_sparse_device(plain.ctx, 0, db.d_ids, None, db.d_cu, db.B, db.max_len, db.T, db.d_out,
                                           db.s) == -6
    for kind in (POOLED, TOKENS):
        assert np.array_equal(bits(db.run(kind)), bits(dm.run(kind)))
    db.close()
    dm.close()
    out = np.full((2, 8), np.nan, F)
    flat = np.ascontiguousarray(np.concatenate(ids))
    tp = (flat.ctypes.data + 4 * np.array([0, 5], np.uintp)).astype(np.uintp)
    op = (out.ctypes.data + out.strides[0] * np.arange(2, dtype=np.uintp)).astype(np.uintp)
    lens = np.array([5, 9], np.int32)
    assert lib.bertx_forward_sparse(plain.ctx, 1, 2, tp.ctypes.data_as(ctypes.POINTER(bertpy.c_i32p)),
                                    lens.ctypes.data_as(bertpy.c_i32p), op.ctypes.data_as(ctypes.POINTER(bertpy.c_f32p))) == -6
    assert np.isnan(out).all()
