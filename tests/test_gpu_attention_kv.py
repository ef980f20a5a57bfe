"""The attention kernels with key counts (bert_hip.h "Key counts"; attention_kv_refs.py, shown
reachable and tight by test_cpu_attention_kv_refs.py): each kernel by name against the float64
attention over the counted keys, with attention_refs' per-element bounds, on batches whose
(len, keys) pairs sit at every edge -- one key, one key short of a block, one key into the next
block, all keys -- and on the planted inputs: uniform, where a leaked key is a V row of 512 and a
dropped one moves an exact mean, and onehot.  Then what the counts must not change: with
keys == len the bits of the plain launch, and on the rows below the count the bits of the same
kernel on the batch cut to those rows.

Every test here fails on a build whose kernels ignore the counts (or has no _kv hooks)."""
import os

import numpy as np
import pytest

import attention_kv_refs as KV
import attention_refs as R
import row_kernel_refs as RK

pytestmark = pytest.mark.gpu

# id: (batch, variant, arithmetic, the kernel that must have run)
KERNELS = {
    "short": ("short", 0, R.WAVE64, R.RAN_SHORT),
    "pp": ("lds", 0, R.WAVE64, R.RAN_PP),
    "lds3": ("lds", 8, R.WAVE64, R.RAN_LDS3),
    "lds3_7wg": ("lds", 7, R.WAVE64, R.RAN_LDS3),
    "lds32": ("lds32", 0, R.LDS32, R.RAN_LDS32),
    "stream64": ("stream64", 0, R.STREAM, R.RAN_STREAM),
    "stream32": ("stream32", 0, R.STREAM, R.RAN_STREAM),
    "stream64_forced": ("lds", -1, R.STREAM, R.RAN_STREAM),
    "stream32_forced": ("lds32", -1, R.STREAM, R.RAN_STREAM),
    "heads3_short": ("heads3_short", 0, R.WAVE64, R.RAN_SHORT),
    "heads3_pp": ("heads3", 0, R.WAVE64, R.RAN_PP),
    "heads3_lds3": ("heads3", 8, R.WAVE64, R.RAN_LDS3),
    "heads3_stream": ("heads3", -1, R.STREAM, R.RAN_STREAM),
}
SWITCH = {R.RAN_PP: "BERT_ATT_PP", R.RAN_SHORT: "BERT_ATT_SHORT"}
CASES = [(k, kind) for k in KERNELS for kind in R.KINDS]


def launch(lib, qkv, cu, keys, n_head, d, variant, want_ran):
    """One launch through the hook (keys None: the plain hook); every row written, by the kernel meant."""
    T = int(cu[-1])
    out = np.zeros((T, d), np.float16)
    if keys is None:
        rc = lib.bertx_test_attention(qkv.ctypes.data, cu.ctypes.data, len(cu) - 1, n_head, d, variant, out.ctypes.data)
    else:
        rc = lib.bertx_test_attention_kv(qkv.ctypes.data, cu.ctypes.data, keys.ctypes.data, len(cu) - 1, n_head, d,
                                         variant, out.ctypes.data)
    assert rc == 0, rc                        # -3 / -4: launch or execution error; -5: a store behind row T
    ran = lib.bertx_test_attention_ran()
    if ran != want_ran and os.environ.get(SWITCH.get(want_ran, ""), "")[:1] == "0":
        pytest.skip("%s=0 takes the batch off the kernel under test" % SWITCH[want_ran])
    assert ran == want_ran, (ran, want_ran)
    bits = out.view(np.uint16)
    assert not (bits == 0xffff).any(), ("rows left unwritten", np.unique(np.argwhere(bits == 0xffff)[:, 0])[:8])
    assert np.isfinite(out).all()
    return out


def launch_case(lib, cs, variant, want_ran, keys="own"):
    return launch(lib, cs.qkv, cs.cu, cs.keys if isinstance(keys, str) else keys, cs.n_head, cs.d, variant, want_ran)


def check(cs, arith, out, key):
    ratio = R.worst_ratio(out, cs.ref, cs.bound(arith))
    planted = None
    if cs.kind in ("uniform", "onehot"):
        want, bd = cs.planted_bound(arith)
        planted = R.worst_ratio(out, want, bd)
    print("%s %s with key counts: worst |got - ref| / bound %.3f" % (key, cs.kind, ratio) +
          ("" if planted is None else ", planted %.3f" % planted))
    assert ratio <= 1.0, ratio
    assert planted is None or planted <= 1.0, planted


@pytest.fixture(scope="module")
def outputs(lib):
    """The output of each (kernel, kind) with the batch's counts, launched once."""
    cache = {}

    def get(kernel, kind):
        if (kernel, kind) not in cache:
            batch, variant, _, want_ran = KERNELS[kernel]
            cache[kernel, kind] = launch_case(lib, KV.case(batch, kind), variant, want_ran)
        return cache[kernel, kind]
    return get


@pytest.mark.parametrize("kernel,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_kernel_within_bound_with_key_counts(outputs, kernel, kind):
    batch, _, arith, _ = KERNELS[kernel]
    check(KV.case(batch, kind), arith, outputs(kernel, kind), kernel)


BITWISE = [(b, kind) for b in ("short", "lds", "heads3", "heads3_short") for kind in R.KINDS]


@pytest.mark.parametrize("batch,kind", BITWISE, ids=["%s-%s" % c for c in BITWISE])
def test_wave64_kernels_share_their_bits_with_key_counts(lib, batch, kind):
    cs = KV.case(batch, kind)
    prod = R.RAN_SHORT if max(cs.lens) <= 64 else R.RAN_PP
    outs = [launch_case(lib, cs, v, ran) for v, ran in ((0, prod), (8, R.RAN_LDS3), (7, R.RAN_LDS3))]
    for o in outs[1:]:
        assert np.array_equal(outs[0].view(np.uint16), o.view(np.uint16))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_full_counts_are_the_plain_launch(lib, kernel):
    """keys == len for every sentence: the bits of the hook without counts."""
    batch, variant, _, want_ran = KERNELS[kernel]
    for kind in ("random", "latemax"):
        cs = KV.case(batch, kind)
        full = np.array(cs.lens, np.int32)
        a = launch_case(lib, cs, variant, want_ran, keys=full)
        b = launch_case(lib, cs, variant, want_ran, keys=None)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


def truncated_agrees(lib, cs, variant, want_ran, out):
    qkv, cu, rows = cs.truncated()
    plain = launch(lib, qkv, cu, None, cs.n_head, cs.d, variant, want_ran)
    return np.array_equal(out[rows].view(np.uint16), plain.view(np.uint16))


PER_QUERY = [k for k, v in KERNELS.items() if v[2] != R.WAVE64]


@pytest.mark.parametrize("kernel", PER_QUERY)
def test_rows_below_the_count_are_the_truncated_batch_per_query_kernels(lib, outputs, kernel):
    """attention_lds<32> and the streaming kernel treat each query on its own: its bits depend
    on its Q row and the counted K / V rows only, so they are those of the plain kernel on the
    batch cut to the counted rows."""
    batch, variant, _, want_ran = KERNELS[kernel]
    for kind in R.KINDS:
        assert truncated_agrees(lib, KV.case(batch, kind), variant, want_ran, outputs(kernel, kind)), kind


WAVE64_KERNELS = [k for k, v in KERNELS.items() if v[2] == R.WAVE64]


@pytest.mark.parametrize("kernel", WAVE64_KERNELS)
def test_rows_below_the_count_are_the_truncated_batch_wave64(lib, outputs, kernel):
    """The same for the AttWave64 kernels, whose only coupling between the queries of a wave is
    the ballot of the offset move: on the kinds where the restatement moves no offset with the
    counts or without the rows behind them (attention_kv_refs.wave64_moves)."""
    batch, variant, _, want_ran = KERNELS[kernel]
    kinds = [k for k in R.KINDS if not KV.wave64_moves(batch, k)]
    assert "uniform" in kinds and len(kinds) >= 2
    for kind in kinds:
        cs = KV.case(batch, kind)
        assert int(cs.keys.max()) > 64 or want_ran != R.RAN_PP      # the truncated batch takes the same kernel
        assert truncated_agrees(lib, cs, variant, want_ran, outputs(kernel, kind)), kind


# ---------------------------------------------------------------- the f32 kernel

PAD = 8
# (the second-to-last sentence is the sharp one)
F32_LENS = [512, 1, 15, 16, 17, 63, 64, 130, 65, 200]
F32_KEYS = [65, 1, 1, 16, 16, 62, 1, 129, 64, 128]


def f32_case(dh):
    """row_kernel_refs' f32 batch (lengths around the 16-query group and the 64-key tile, one
    sharp sentence) with a count per sentence: 1, all, one short of all, and both sides of the
    64-key tile's edge."""
    qkv, cu, n_head, d = RK.attention_case(dh, lens=F32_LENS)
    return qkv, cu, np.array(F32_KEYS, np.int32), n_head, d


def f32_ref_kv(qkv, cu, keys, n_head, d):
    """row_kernel_refs.attention_ref (the era softmax in f64 and its bound, derived there) with
    each item's K and V cut to the counted rows: the same expressions, n the counted keys."""
    table = RK.era_exp_table()
    D, U = np.float64, RK.U
    dh = d // n_head
    out = np.zeros((qkv.shape[0], d), D)
    bound = np.zeros_like(out)
    x = qkv.astype(D)
    for s in range(len(cu) - 1):
        a, b, n = int(cu[s]), int(cu[s + 1]), int(keys[s])
        for h in range(n_head):
            c = slice(h * dh, (h + 1) * dh)
            q, k, v = x[a:b, c], x[a:a + n, d:2 * d][:, c], x[a:a + n, 2 * d:][:, c]
            sc = q @ k.T / np.sqrt(dh)
            ds = (dh + 1) * U * (np.abs(q) @ np.abs(k).T) / np.sqrt(dh)
            arg = sc - sc.max(axis=1, keepdims=True)
            da = ds + ds.max(axis=1, keepdims=True) + U * np.abs(arg)
            a16 = arg.astype(np.float16)
            Da = da + np.spacing(np.abs(a16)).astype(D)
            e = table[a16.view(np.uint16)].astype(D)
            de = np.exp(arg + Da) * Da + np.spacing(table[a16.view(np.uint16)]).astype(D)
            sm = e.sum(axis=1, keepdims=True)
            p = e / sm
            dp = de / sm + p * (de.sum(axis=1, keepdims=True) / sm + 2 * U)
            out[a:b, c] = p @ v
            bound[a:b, c] = dp @ np.abs(v) + n * U * (p @ np.abs(v))
    return out, bound


def run_f32(lib, qkv, cu, keys, n_head, d, era, max_len=512):
    T = qkv.shape[0]
    out = np.full((T + PAD, d), np.nan, np.float32)
    kp = None if keys is None else keys.ctypes.data
    rc = lib.bertx_test_attention_f32_kv(qkv.ctypes.data, cu.ctypes.data, kp, len(cu) - 1, max_len, n_head, d, era,
                                         out.ctypes.data, T + PAD)
    return rc, out


@pytest.mark.parametrize("era", [0, 1])
@pytest.mark.parametrize("dh", [32, 64])
def test_f32_attention_with_key_counts(lib, dh, era):
    """f32_attention_kernel<DH, ERA> (the f32 chain and the q8-activation chain): every row
    against the float64 attention over the counted keys within row_kernel_refs' bound; rows below
    the count with the bits of the plain kernel on the truncated batch (a query per 16 lanes, no
    coupling); with keys == len the plain hook's bits."""
    qkv, cu, keys, n_head, d = f32_case(dh)
    T = qkv.shape[0]
    assert (keys < np.diff(cu)).any()
    rc, out = run_f32(lib, qkv, cu, keys, n_head, d, era)
    assert rc == 0, rc
    assert np.isnan(out[T:]).all() and np.isfinite(out[:T]).all()
    ref, bound = f32_ref_kv(qkv, cu, keys, n_head, d)
    ratio = float((np.abs(out[:T] - ref) / bound).max())
    print("f32_attention dh %d era %d with key counts: worst error / bound %.3f" % (dh, era, ratio))
    assert ratio <= 1.0
    rows = np.concatenate([np.arange(int(cu[b]), int(cu[b]) + int(keys[b])) for b in range(len(keys))])
    tq = np.ascontiguousarray(qkv[rows])
    rc, plain = run_f32(lib, tq, R.cu_of(keys), None, n_head, d, era)
    assert rc == 0, rc
    assert np.array_equal(out[rows].view(np.uint32), plain[:len(rows)].view(np.uint32))
    rc, a = run_f32(lib, qkv, cu, np.diff(cu).astype(np.int32), n_head, d, era)
    assert rc == 0, rc
    b = np.full((T + PAD, d), np.nan, np.float32)
    assert lib.bertx_test_attention_f32(qkv.ctypes.data, cu.ctypes.data, len(cu) - 1, 512, n_head, d, era,
                                        b.ctypes.data, T + PAD) == 0
    assert np.array_equal(a[:T].view(np.uint32), b[:T].view(np.uint32))


def test_counts_out_of_range_are_refused(lib):
    cs = KV.case("short", "random")
    out = np.zeros((cs.T, cs.d), np.float16)
    for bad in (0, None):
        keys = cs.keys.copy()
        keys[2] = 0 if bad == 0 else cs.lens[2] + 1
        assert lib.bertx_test_attention_kv(cs.qkv.ctypes.data, cs.cu.ctypes.data, keys.ctypes.data, len(cs.lens),
                                           cs.n_head, cs.d, 0, out.ctypes.data) == -1
        qkv, cu, k32, n_head, d = f32_case(64)
        k32 = k32.copy()
        k32[1] = 0 if bad == 0 else int(np.diff(cu)[1]) + 1
        rc, o = run_f32(lib, qkv, cu, k32, n_head, d, 0)
        assert rc == -1 and np.isnan(o).all()
