"""Per-kernel parity of the memory-bound row kernels on the GPU: the embeddings + LayerNorm
kernels of both chains with their two table readers, the statistics kernel, the pooling
and per-token kernels (norm.hip), and the f32 chain's LayerNorm, attention, pool and CLS
kernels (f32.hip), each one launch through a bertx_test_* hook against a numpy f64
reference of the same operation computed from exactly the values the kernel reads
(row_kernel_refs.py: inputs, references, restatements, and bounds counted from the kernels'
operation sequences).  Bits are asserted wherever the arithmetic is reproducible.  Every
output carries sentinel rows behind the last row the kernel may write."""
import numpy as np
import pytest

import row_kernel_refs as R
from row_kernel_refs import D, F, PAD, SENT, SENT16, U, bits, ptr

pytestmark = pytest.mark.gpu


def report(name, err, bound):
    w = R.worst(err, bound)
    print("%s: worst error / bound %.3f" % (name, w))
    return w


def out_f32(rows, d):
    return np.full((rows + PAD, d), SENT, F)


def untouched(a, rows):
    """The sentinel rows behind the first `rows` rows still hold the sentinel's bits."""
    s = SENT16 if a.dtype == np.float16 else SENT
    return np.array_equal(bits(a[rows:]), bits(np.full_like(a[rows:], s)))


# ---------------------------------------------------------------- embeddings + LayerNorm

def run_embed(lib, case, mode):
    d, T = case.d, case.T
    out = np.full((T + PAD, d), SENT16, np.float16) if mode == 0 else out_f32(T, d)
    stats = np.full((T + PAD, 2), SENT, F)
    rc = lib.bertx_test_embed_ln(mode, case.fmts[0], case.fmts[1], case.fmts[2], R.WORD_ROWS, R.POS_ROWS, d,
                                 case.raw[0], case.raw[1], case.raw[2], ptr(case.g), ptr(case.b), ptr(case.ids),
                                 ptr(case.cu), len(case.lens), case.max_len, ptr(out), ptr(stats), T + PAD)
    assert rc == 0, rc
    assert untouched(out, T)
    assert untouched(stats, T if mode == 0 else 0)
    return out[:T], stats[:T]


def check_embed(lib, case, tag):
    y = case.sum_f32()
    # mode 0 (table32): z bit for bit, the statistics within their counted bound
    z, st = run_embed(lib, case, 0)
    assert np.array_equal(bits(z), R.embed_z_bits(y, case.g)), tag
    mean, r = R.ln_ref(y)
    bm, br = R.embed_stats_bound(y)
    assert report("embed_ln mean " + tag, np.abs(st[:, 0] - mean), bm) <= 1
    assert report("embed_ln 1/sigma " + tag, np.abs(st[:, 1] - r), br) <= 1
    # modes 1, 2 (table4): the LayerNorm of the same sum, and the exact form's bits
    ref, bound = R.ln_ref_bound(y, case.g, case.b)
    assert R.ln_tie_ok(y) > 1
    for mode in (1, 2):
        x, _ = run_embed(lib, case, mode)
        assert report("f32_embed_ln mode %d %s" % (mode, tag), np.abs(x - ref), bound) <= 1
        if mode == 2:
            assert np.array_equal(bits(x), bits(R.ln_exact_f32(y, case.g, case.b))), tag


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_embed_ln_every_format(lib, oracle, fmt, d):
    """Table decode, embedding sum and LayerNorm of both chains' embed kernels for every
    table format: q d (+ m) is exact in f32 and every sum is one f32 add in the order
    pos + (type + word), so z = f16(f32(y) gamma) is asserted bit for bit (table32), the
    f32 chain's exact LayerNorm bit for bit (table4) and the rest within counted bounds.
    Ragged lengths around the 8- and 4-row workgroup edges, ids on row 0, the last row and
    repeated rows, every quant block with its own scale and minimum."""
    check_embed(lib, R.EmbedCase((fmt, fmt, fmt), d, seed=fmt), "%s d %d" % (R.FMTS[fmt], d))


@pytest.mark.parametrize("d", [384, 1024])
@pytest.mark.parametrize("fmts", [(2, 0, 1), (8, 3, 0)])
def test_embed_ln_mixed_formats(lib, oracle, fmts, d):
    """Tables of three different formats (the TF = -1 instantiation no model file selects):
    the bits of the same values passed as three f32 tables, in all three modes."""
    case = R.EmbedCase(fmts, d, seed=20 + fmts[0])
    plain = case.as_f32_tables()
    check_embed(lib, case, "mixed %s d %d" % ("+".join(R.FMTS[f] for f in fmts), d))
    for mode in (0, 1, 2):
        a, sa = run_embed(lib, case, mode)
        b, sb = run_embed(lib, plain, mode)
        assert np.array_equal(bits(a), bits(b)), mode
        assert np.array_equal(bits(sa), bits(sb)), mode


# ---------------------------------------------------------------- ln_stats

def run_ln_stats(lib, part, G, rows, d):
    stats = np.full((rows + PAD, 2), SENT, F)
    rc = lib.bertx_test_ln_stats(ptr(part), G, part.shape[1], rows, d, ptr(stats), rows + PAD)
    return rc, stats


@pytest.mark.parametrize("G", R.STATS_G)
def test_ln_stats(lib, G):
    """ln_stats_kernel<G> (G 12, 16, 24, 32) and ln_stats_any (G 2, 20) for 1 .. 66 row
    blocks (13 and 16 blocks: the XCD row-block permutation with and without a remainder;
    1 row, 64, 65: the block edge), every row with its own mean, the partial planes wider
    than the rows: Chan's combination of the same f32 partials in f64 within the counted
    bound, and ln_row_stats restated in numpy float32 within the device's division / root."""
    for rows in R.STATS_ROWS:
        part = R.stats_parts(rows, G, seed=100 * G + rows % 97)
        rc, st = run_ln_stats(lib, part, G, rows, 32 * G)
        assert rc == 0, (rc, rows)
        assert untouched(st, rows), rows
        ref, bound = R.stats_ref(part, rows)
        assert report("ln_stats G %d rows %d" % (G, rows), np.abs(st[:rows] - ref), bound) <= 1
        f32 = R.ln_row_stats_f32(np.ascontiguousarray(part[:, :rows]), 32 * G)
        assert np.allclose(st[:rows], f32, rtol=5e-7, atol=1e-12), (rows, np.abs(st[:rows] - f32).max())


def test_ln_stats_refusals(lib):
    """More than 32 partials per row, or a width that is not 32 G, is refused with nothing
    launched: -1 and the output untouched."""
    for G, d in ((33, 33 * 32), (24, 1024), (12, 768)):
        part = R.stats_parts(70, G, seed=3)
        rc, st = run_ln_stats(lib, part, G, 70, d)
        assert rc == -1, (G, d, rc)
        assert untouched(st, 0)


# ---------------------------------------------------------------- pooling and per-token output

def run_pool(lib, case, kind, max_len=0, z=None, stats=None, cu=None, n=None):
    z = case.z if z is None else z
    stats = case.stats if stats is None else stats
    cu = case.cu if cu is None else cu
    n = len(cu) - 1 if n is None else n
    rows = z.shape[0] if kind == 3 else n
    out = out_f32(rows, case.d)
    rc = lib.bertx_test_pool(kind, ptr(z), ptr(stats), ptr(case.g), ptr(case.b), None if kind >= 2 else ptr(cu), n,
                             max_len, z.shape[0], case.d, ptr(out), rows + PAD)
    assert rc == 0, rc
    assert untouched(out, rows)
    return out[:rows]


def norms_are_one(out, c):
    """||out|| = 1 within c f32 roundings (c: the norm's and the division's, counted at
    row_kernel_refs C_NORM / f32_pool_ref)."""
    return np.all(np.abs(np.linalg.norm(out.astype(D), axis=1) - 1) <= c * U)


@pytest.mark.parametrize("d", R.WIDTHS)
def test_pool_mean(lib, d):
    """Mean pool + L2 from z and the row statistics, two launches (max_len 512) and one
    (a batch of at most 256 tokens per sentence), against f64; lengths around the 64-token
    chunk edges; max_len rows of poison follow the batch, so a chunk running past its
    sentence's end reads them (and stays inside the buffers) and is seen."""
    for lens, max_len in R.POOL_BATCHES:
        case = R.StreamCase(lens, d, seed=d + max_len, pad=max_len)
        out = run_pool(lib, case, 0, max_len)
        ref, bound = R.pool_ref(case, max_len)
        assert report("pool_l2 d %d max_len %d" % (d, max_len), np.abs(out - ref), bound) <= 1
        assert norms_are_one(out, R.C_NORM + 1)


@pytest.mark.parametrize("d", [384, 768, 1024])
def test_pool_bits_do_not_depend_on_the_batch(lib, d):
    """A sentence pooled alone with max_len = len (one launch up to 256 tokens) and inside a
    batch with max_len 512 (two launches) gives the same bits: the forward's batch
    invariance rests on it."""
    case = R.StreamCase(R.LENS, d, seed=d + 1, pad=512)
    batch = run_pool(lib, case, 0, 512)
    for s, n in enumerate(case.lens):
        a = int(case.cu[s])
        alone = run_pool(lib, case, 0, n, z=np.ascontiguousarray(case.z[a:a + n + 64]),
                         stats=np.ascontiguousarray(case.stats[a:a + n + 64]), cu=R.cu_of([n]))
        assert np.array_equal(bits(alone[0]), bits(batch[s])), (n, d)


@pytest.mark.parametrize("d", R.WIDTHS)
def test_cls_and_tokens(lib, d):
    """[CLS] pooling in its cu form and its compact-row form, and the per-token output,
    against f64; CLS with cu = CLS on the compacted rows, bit for bit; CLS = the tokens
    output's row cu[b] normalised in f64, within the norm's and the division's roundings."""
    case = R.StreamCase(R.LENS, d, seed=d + 2, pad=0)
    tok = run_pool(lib, case, 3)
    v, mag = case.terms()
    assert report("tokens_f32 d %d" % d, np.abs(tok - v), R.C_TOKEN * U * mag) <= 1
    cls = run_pool(lib, case, 1)
    ref, bound = R.cls_ref(case)
    assert report("cls_l2 d %d" % d, np.abs(cls - ref), bound) <= 1
    assert norms_are_one(cls, R.C_NORM + 1)
    rows = case.cu[:-1]
    compact = run_pool(lib, case, 2, z=np.ascontiguousarray(case.z[rows]),
                       stats=np.ascontiguousarray(case.stats[rows]), n=len(rows))
    assert np.array_equal(bits(cls), bits(compact))
    t = tok[rows].astype(D)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    assert np.all(np.abs(cls - t) <= (R.C_NORM + 1) * U * np.abs(t))


def test_tokens_grid_stride(lib):
    """T d / 8 above 4096 * 256 threads: the grid-stride loop takes a second pass; every
    row is checked."""
    case = R.StreamCase([8195], 1024, seed=9, pad=0)
    tok = run_pool(lib, case, 3)
    v, mag = case.terms()
    assert report("tokens_f32 T 8195", np.abs(tok - v), R.C_TOKEN * U * mag) <= 1


# ---------------------------------------------------------------- the f32 chain

@pytest.mark.parametrize("d", R.WIDTHS)
def test_f32_ln(lib, d):
    """f32_ln_kernel, both forms, against f64; the exact form bit for bit against ln_row
    restated in numpy (no row's mean or variance near an f32 rounding tie, checked first)."""
    x, g, b = R.f32_ln_case(d)
    n = x.shape[0]
    assert R.ln_tie_ok(x) > 1
    ref, bound = R.ln_ref_bound(x, g, b)
    for exact in (0, 1):
        out = out_f32(n, d)
        assert lib.bertx_test_f32_rows(0, ptr(x), None, n, d, ptr(g), ptr(b), exact, ptr(out), n + PAD) == 0
        assert untouched(out, n)
        assert report("f32_ln exact %d d %d" % (exact, d), np.abs(out[:n] - ref), bound) <= 1
        if exact:
            assert np.array_equal(bits(out[:n]), bits(R.ln_exact_f32(x, g, b)))


def run_attention(lib, qkv, cu, n_head, d, era, max_len):
    T = qkv.shape[0]
    out = out_f32(T, d)
    rc = lib.bertx_test_attention_f32(ptr(qkv), ptr(cu), len(cu) - 1, max_len, n_head, d, era, ptr(out), T + PAD)
    return rc, out


@pytest.mark.parametrize("dh", [32, 64])
def test_f32_attention(lib, oracle, dh):
    """f32_attention_kernel<DH, ERA>: lengths around the 16-query group and the 64-key tile,
    one sentence with sharp scores.  era 0 against f64 with the era softmax; era 1 bit for
    bit against the oracle's dot_f32 order restated in numpy float32."""
    qkv, cu, n_head, d = R.attention_case(dh)
    T = qkv.shape[0]
    ref, bound = R.attention_ref(qkv, cu, n_head, d)
    for era in (0, 1):
        rc, out = run_attention(lib, qkv, cu, n_head, d, era, 512)
        assert rc == 0, rc
        assert untouched(out, T)
        assert report("f32_attention dh %d era %d" % (dh, era), np.abs(out[:T] - ref), bound) <= 1
        if era:
            assert np.array_equal(bits(out[:T]), bits(R.attention_era_f32(qkv, cu, n_head, d)))


def test_f32_attention_long_sentences(lib, oracle):
    """Lengths above 512, which the loader accepts: 1000 tokens ask for about 85 KB of
    dynamic LDS (dh 64), above 64 KiB, and nothing raises the kernel's dynamic-LDS
    attribute.  On an MI355X (ROCm 7) the runtime accepts the launch as it is -- the hook
    returns -3 if it ever refuses -- and the result is within the bound of the short
    lengths.  A length whose score rows exceed the device's 160 KiB is refused by the
    launcher: -1, nothing written."""
    for dh in (64, 32):
        qkv, cu, n_head, d = R.attention_case(dh, lens=[600, 1000, 17], seed=1)
        T = qkv.shape[0]
        rc, out = run_attention(lib, qkv, cu, n_head, d, 0, 1000)
        assert rc == 0, rc
        assert untouched(out, T)
        ref, bound = R.attention_ref(qkv, cu, n_head, d)
        assert report("f32_attention long dh %d" % dh, np.abs(out[:T] - ref), bound) <= 1
        rc, out = run_attention(lib, qkv, cu, n_head, d, 0, 4096)
        assert rc == -1
        assert untouched(out, 0)


@pytest.mark.parametrize("d", R.WIDTHS)
def test_f32_pool_and_cls(lib, d):
    """f32_pool_kernel in both orders and f32_cls_kernel against f64; the era order bit for
    bit against the eight-lane restatement over the tokens (lengths that are no multiple of
    8 included); norms 1 within f32 rounding."""
    x, cu = R.f32_pool_case(d)
    n = len(cu) - 1
    ref, bound = R.f32_pool_ref(x, cu)
    era_bits, tie = R.f32_pool_era_f32(x, cu)
    assert tie.min() > 1
    for era in (0, 1):
        out = out_f32(n, d)
        assert lib.bertx_test_f32_rows(1, ptr(x), ptr(cu), n, d, None, None, era, ptr(out), n + PAD) == 0
        assert untouched(out, n)
        assert report("f32_pool era %d d %d" % (era, d), np.abs(out[:n] - ref), bound) <= 1
        assert norms_are_one(out[:n], 3)
        if era:
            assert np.array_equal(bits(out[:n]), bits(era_bits))
    out = out_f32(n, d)
    assert lib.bertx_test_f32_rows(2, ptr(x), ptr(cu), n, d, None, None, 0, ptr(out), n + PAD) == 0
    assert untouched(out, n)
    ref, bound = R.f32_cls_ref(x, cu)
    assert report("f32_cls d %d" % d, np.abs(out[:n] - ref), bound) <= 1
    assert norms_are_one(out[:n], 3)
