"""The f16 attention kernels, each by name, against the float64 attention of their f16
inputs with the per-element bounds of attention_refs.py (derived from the kernels' operation
sequences and shown reachable and tight by test_cpu_attention_refs.py), on random, late-maximum,
uniform and one-hot inputs at every length edge the kernels have.  The hooks fill the output
with NaN bits before the launch and check the rows behind it, so an unwritten row, a row written
for another sentence and a store past the batch all show; bertx_test_attention_ran says which
kernel produced the bits.

Run with -s for the worst error / bound per kernel.  On an MI355X: short 0.984, pp = lds3 (on one
workgroup per CU and on seven) 0.997 with 0.921 on the late-maximum input, lds<32> 0.999, streaming
0.997 (0.999 through variant -1), attention_cls 0.999; the values next to 1 are uniform inputs whose
exact mean lies next to an f16 rounding boundary, where the bound is half an f16 step."""
import os

import numpy as np
import pytest

import attention_refs as R

pytestmark = pytest.mark.gpu

# id: (batch, variant, arithmetic, the kernel that must have run)
KERNELS = {
    "short": ("short", 0, R.WAVE64, R.RAN_SHORT),
    "pp": ("lds", 0, R.WAVE64, R.RAN_PP),
    "lds3": ("lds", 8, R.WAVE64, R.RAN_LDS3),
    "lds3_7wg": ("lds", 7, R.WAVE64, R.RAN_LDS3),
    "lds32": ("lds32", 0, R.LDS32, R.RAN_LDS32),
    "stream64": ("stream64", 0, R.STREAM, R.RAN_STREAM),       # a batch that holds sentences over 512 tokens
    "stream32": ("stream32", 0, R.STREAM, R.RAN_STREAM),
    "stream64_forced": ("lds", -1, R.STREAM, R.RAN_STREAM),    # variant -1: tiles past a sentence return early
    "stream32_forced": ("lds32", -1, R.STREAM, R.RAN_STREAM),
    # three heads, head h's V offset by h: an output in another head's columns is off by an integer
    "heads3_short": ("heads3_short", 0, R.WAVE64, R.RAN_SHORT),
    "heads3_pp": ("heads3", 0, R.WAVE64, R.RAN_PP),
    "heads3_lds3": ("heads3", 8, R.WAVE64, R.RAN_LDS3),
    "heads3_stream": ("heads3", -1, R.STREAM, R.RAN_STREAM),
}
SWITCH = {R.RAN_PP: "BERT_ATT_PP", R.RAN_SHORT: "BERT_ATT_SHORT"}
OFFSET_BATCHES = ("lds", "heads3")            # the batches with blocks behind block 0 at dh 64

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\nworst error / bound on the GPU, %-16s: " % k + "  ".join("%s %.3f" % kv for kv in WORST[k].items()))


def launch(lib, cs, variant, want_ran):
    """One launch through the hook; the output with every row written, from the kernel meant."""
    out = np.zeros((cs.T, cs.d), np.float16)
    rc = lib.bertx_test_attention(cs.qkv.ctypes.data, cs.cu.ctypes.data, len(cs.lens), cs.n_head, cs.d, variant,
                                  out.ctypes.data)
    assert rc == 0, rc                        # -3 / -4: launch or execution error; -5: a store behind row T
    ran = lib.bertx_test_attention_ran()
    if ran != want_ran and os.environ.get(SWITCH.get(want_ran, ""), "")[:1] == "0":
        pytest.skip("%s=0 takes the batch off the kernel under test" % SWITCH[want_ran])
    assert ran == want_ran, (ran, want_ran)
    bits = out.view(np.uint16)
    assert not (bits == 0xffff).any(), ("rows left unwritten", np.unique(np.argwhere(bits == 0xffff)[:, 0])[:8])
    assert np.isfinite(out).all()
    return out


def check(cs, arith, out, key):
    """The general bound, and a planted input's own; records the worst ratio."""
    rows = cs.cu[:-1] if arith == R.CLS else slice(None)
    ratio = R.worst_ratio(out, cs.ref[rows], cs.bound(arith))
    planted = None
    if cs.kind in ("uniform", "onehot"):
        want, bd = cs.planted_bound(arith)
        planted = R.worst_ratio(out, want[rows], bd[rows])
    seen = WORST.setdefault(key, {})
    seen[cs.kind] = max(seen.get(cs.kind, 0.0), ratio, planted or 0.0)
    print("%s %s: worst |got - ref| / bound %.3f" % (key, cs.kind, ratio) +
          ("" if planted is None else ", planted %.3f" % planted))
    err = np.abs(out.astype(np.float64) - cs.ref[rows])
    bad = np.argwhere(err > cs.bound(arith))
    assert ratio <= 1.0, (ratio, [(tuple(i), float(out[tuple(i)]), float(cs.ref[rows][tuple(i)])) for i in bad[:5]])
    assert planted is None or planted <= 1.0, planted


def kinds_of(batch, arith):
    return R.ALL_KINDS if arith == R.WAVE64 and batch in OFFSET_BATCHES else R.KINDS


CASES = [(k, kind) for k, (batch, _, arith, _) in KERNELS.items() for kind in kinds_of(batch, arith)]


@pytest.mark.parametrize("kernel,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_attention_kernel_within_bound(lib, kernel, kind):
    batch, variant, arith, want_ran = KERNELS[kernel]
    cs = R.case(batch, kind)
    check(cs, arith, launch(lib, cs, variant, want_ran), kernel)


BITWISE = [(b, kind) for b in ("short", "lds", "heads3", "heads3_short") for kind in kinds_of(b, R.WAVE64)]


@pytest.mark.parametrize("batch,kind", BITWISE, ids=["%s-%s" % c for c in BITWISE])
def test_wave64_kernels_share_their_bits(lib, batch, kind):
    """attention_short, attention_pp and attention_lds3 (on one workgroup per CU and on seven)
    run every query through AttWave64: the same bits, and those bits inside the bound, on the
    inputs where the restatement says the offset moved (latemax, onehot) as on the others."""
    cs = R.case(batch, kind)
    prod = R.RAN_SHORT if max(cs.lens) <= 64 else R.RAN_PP
    outs = [launch(lib, cs, v, ran) for v, ran in ((0, prod), (8, R.RAN_LDS3), (7, R.RAN_LDS3))]
    for o in outs[1:]:
        assert np.array_equal(outs[0].view(np.uint16), o.view(np.uint16))
    check(cs, R.WAVE64, outs[0], "wave64 shared")


def gather_launch(lib, cs, Mc, z=None, st=None):
    n = len(cs.lens)
    out = np.zeros((Mc, cs.d), np.float16)
    zc = stc = None
    if z is not None:
        zc = np.zeros((Mc, cs.d), np.float16)
        stc = np.zeros((Mc, 2), np.float32)
    rc = lib.bertx_test_attention_cls_gather(cs.qkv.ctypes.data, cs.cu.ctypes.data, n, cs.n_head, cs.d, Mc,
                                             out.ctypes.data, R_ptr(z), R_ptr(st), R_ptr(zc), R_ptr(stc))
    assert rc == 0, rc
    assert np.isfinite(out[:n]).all() and not (out.view(np.uint16) == 0xffff).any()
    assert not out[n:].view(np.uint16).any()              # the padding rows: the kernel's own zeros
    return out, zc, stc


def R_ptr(a):
    return None if a is None else a.ctypes.data


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dh", [64, 32])
def test_attention_cls_within_bound(lib, dh, kind):
    """The single-query kernel at the edges of its 256-key chunks and past the LDS form's 512."""
    cs = R.case("cls%d" % dh, kind)
    out, _, _ = gather_launch(lib, cs, 64)
    check(cs, R.CLS, out[:len(cs.lens)], "attention_cls<%d>" % dh)


@pytest.mark.parametrize("n_seqs", [1, 64, 65])
@pytest.mark.parametrize("dh", [64, 32])
def test_attention_cls_gather_is_exact(lib, dh, n_seqs):
    """zc[b] = z[cu[b]] and stc[b] = st[cu[b]] bit for bit, rows n_seqs <= row < Mc of all three
    compact buffers zero, no NaN bits left (the buffers start as 0xff bytes), with n_seqs on both
    sides of a 64-row tile edge; the attention rows themselves within the bound."""
    rng = np.random.default_rng(n_seqs + dh)
    lens = [int(x) for x in rng.integers(1, 40, n_seqs)]
    cs = R.Case(lens, 3, dh, "random", seed=n_seqs)
    z = rng.standard_normal((cs.T, cs.d)).astype(np.float16)
    st = rng.standard_normal((cs.T, 2)).astype(np.float32)
    Mc = (n_seqs + 63) // 64 * 64
    out, zc, stc = gather_launch(lib, cs, Mc, z, st)
    first = cs.cu[:-1]
    assert np.array_equal(zc[:n_seqs].view(np.uint16), z[first].view(np.uint16))
    assert np.array_equal(stc[:n_seqs].view(np.uint32), st[first].view(np.uint32))
    assert not zc[n_seqs:].view(np.uint16).any() and not stc[n_seqs:].view(np.uint32).any()
    assert not (zc.view(np.uint16) == 0xffff).any() and not (stc.view(np.uint32) == 0xffffffff).any()
    check(cs, R.CLS, out[:n_seqs], "attention_cls<%d> gather" % dh)
