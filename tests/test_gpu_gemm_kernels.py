"""The fused-dequant GEMM (gemm.hip), every format, shipped tile config and epilogue form, against
the float64 references and per-element bounds of gemm_refs.py (counted from the kernel's
operations; shown reachable and tight by test_cpu_gemm_refs.py), bit for bit on integer and
one-hot operands, at the row counts the small-batch forward launches (64 .. 320, the tile
fallbacks among them), on persistent grids that walk more than one tile per workgroup, with the
residual form's per-group partials read back, and the GELU epilogue over every normal f16 input.

The hooks (bertx_test_gemm_rows / bertx_test_gemm_fold_rows) launch exactly `rows` rows, fill the
rows behind M with non-zero values, start every written buffer as 0xFF bytes and check 64 guard
rows behind it (-5), so an unwritten element, and a store past the launch, both show;
bertx_test_gemm_ran says which tile config produced the bits.

Run with -s for the worst error / bound per (format, config, form).  On an MI355X (256 CUs), the
worst over the five configs: per-element bound at K = 64 .. 448, f32 files 0.957, f16 0.978, q4_0
0.979, q4_1 0.974, q8_0 0.975 (the f16 rounding of the output: the statistics fold gives the input-LN
form's ratio, the bits being the same), the partials 0.005 and the statistics 0.002 of theirs; under
the heuristic at rows 64 .. 320, 0.77 at K = 384, 0.49 at K = 768, 0.30 at K = 1536; the integer and
one-hot launches bit for bit, the fallbacks ran 3 and 4 and the heuristic 4 (f16, f32 files) and 16
at every row count; 528 and 520 tiles walked by 512 workgroups bit for bit for each tile shape;
gelu8_era 15 f16 steps from the era table where |T| >= 2^-13 (the numpy restatement: 15; asserted:
19) and 6.2e-5 below that; behind a dequantized product 0.125 of its allowance.
"""
import os

import numpy as np
import pytest

import gemm_refs as R

pytestmark = pytest.mark.gpu

D, F, H = np.float64, np.float32, np.float16
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\nworst error / bound on the GPU, %-14s: " % k + "  ".join("%s %.3f" % kv for kv in sorted(WORST[k].items())))


def note(key, sub, ratio):
    seen = WORST.setdefault(key, {})
    seen[sub] = max(seen.get(sub, 0.0), ratio)


def ptr(a):
    return None if a is None else a.ctypes.data


def f32c(a):
    return None if a is None else np.ascontiguousarray(a, F)


def written(a):
    """No 0xFF byte pattern left and every value finite."""
    bits = a.view(np.uint16 if a.dtype == H else np.uint32)
    nan_bits = 0xffff if a.dtype == H else 0xffffffff
    assert not (bits == nan_bits).any(), ("left unwritten", np.argwhere(bits == nan_bits)[:4])
    assert np.isfinite(a).all()


def launch(lib, wt, rows, x, bias, epi, cfg, in_ln=None, res=None, res_ln=None, gn=None, oop=0, want_ran=None):
    """bertx_test_gemm_rows: (out f16 [rows][N], stats f32 [rows][2] or None, partials f32
    [N/32][rows][2] or None).  in_ln / res_ln = (stats, gamma, beta); x (and res) may hold fewer
    than `rows` rows, the hook fills the others."""
    N, K, M = wt.N, wt.K, x.shape[0]
    x = np.ascontiguousarray(x, H)
    res = None if res is None else np.ascontiguousarray(res, H)
    out = np.zeros((rows, N), H)
    st = np.zeros((rows, 2), F) if gn is not None else None
    part = np.zeros((N // 32, rows, 2), F) if gn is not None else None
    keep = [f32c(a) for a in (bias,) + (in_ln or (None,) * 3) + (res_ln or (None,) * 3) + (gn,)]
    b, ist, ig, ib, rst, rg, rb, g_next = (ptr(a) for a in keep)
    rc = lib.bertx_test_gemm_rows(wt.fmt, N, K, wt.wb, b, M, rows, ptr(x), ist, ig, ib, epi, ptr(res), rst, rg, rb,
                                  g_next, oop, ptr(out), ptr(st), ptr(part), cfg)
    assert rc == 0, rc                        # -5: a store behind row `rows`
    if want_ran is None and cfg:
        want_ran = R.ran_cfg(cfg, rows)
    if want_ran is not None:
        assert lib.bertx_test_gemm_ran() == want_ran, (lib.bertx_test_gemm_ran(), want_ran, cfg, rows)
    for a in (out, st, part):
        if a is not None:
            written(a)
    return out, st, part


def launch_fold(lib, wt, rows, x, part, g, be, bias, epi, cfg, want_ran=None):
    """bertx_test_gemm_fold_rows: (rc, out, the fold's statistics, the statistics kernel's)."""
    N, K, M = wt.N, wt.K, x.shape[0]
    x = np.ascontiguousarray(x, H)
    out = np.zeros((rows, N), H)
    st, stk = np.zeros((rows, 2), F), np.zeros((rows, 2), F)
    keep = [f32c(a) for a in (bias, part, g, be)]
    b, p, gg, bb = (ptr(a) for a in keep)
    rc = lib.bertx_test_gemm_fold_rows(wt.fmt, N, K, wt.wb, b, M, rows, ptr(x), p, gg, bb, epi, ptr(out), ptr(st),
                                       ptr(stk), cfg)
    if rc != 0:
        return rc, None, None, None
    if want_ran is None and cfg:
        want_ran = R.ran_cfg(cfg, rows)
    if want_ran is not None:
        assert lib.bertx_test_gemm_ran() == want_ran
    for a in (out, st, stk):
        written(a)
    return rc, out, st, stk


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_fold(lib, wt, rows, y, g, be, z, bias, epi, cfg, want_ran=None):
    """The statistics fold on the partials of y: statistics bitwise the statistics kernel's and
    ln_row_stats restated within the device's division / square root; returns (out, statistics)."""
    part = R.group_partials(y)
    rc, out, st, stk = launch_fold(lib, wt, rows, z, part, g, be, bias, epi, cfg, want_ran)
    assert rc == 0, rc
    M = len(y)
    assert bits_equal(st, stk)
    assert np.allclose(st[:M], R.ln_row_stats_f32(part, wt.K), rtol=5e-7, atol=1e-12)
    return out, st


# ---------------------------------------------------------------- a. the per-element bound

@pytest.mark.parametrize("cfg", R.CONFIGS)
@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_bound_every_form(lib, fmt, cfg):
    """K = 64 .. 448 (every remainder of the unrolled K loop), N one column tile plus a partial
    one, one row tile: plain epi 0 / 2, the input-LN fold, the residual LN with g_next and its
    partials, and the statistics fold (-2 for the 256-row configs, which have no fold form)."""
    rows, N = R.ROW_TILE[cfg], R.COL_TILE[cfg] + 32
    key = "%s cfg %d" % (R.FMTS[fmt], cfg)
    for ks in range(1, 8):
        K = 64 * ks
        kind = R.KINDS[ks % 3]
        M = rows - 3 if ks == 2 else rows      # once with pad rows behind M
        rng = np.random.default_rng(1000 * cfg + 100 * ks + fmt)
        wt = R.random_weights(fmt, N, K, rng, kind)
        bias = (rng.standard_normal(N) * 0.1).astype(F)
        x = R.random_x(M, K, rng, kind)
        res = rng.standard_normal((M, N)).astype(H)
        out, _, _ = launch(lib, wt, rows, x, bias, 0, cfg)
        note(key, "plain0", R.worst_ratio(out[:M], *R.plain(wt, x, bias)))
        out, _, _ = launch(lib, wt, rows, x, bias, 2, cfg, res=res)
        note(key, "plain2", R.worst_ratio(out[:M], *R.plain(wt, x, bias, res)))
        y, g, be, z, stats = R.ln_stream(M, K, rng)
        out, _, _ = launch(lib, wt, rows, z, bias, 0, cfg, in_ln=(stats, g, be))
        note(key, "inln", R.worst_ratio(out[:M], *R.input_ln(wt, z, stats, g, be, bias)))
        if R.ROW_TILE[cfg] == 256:
            assert launch_fold(lib, wt, rows, z, R.group_partials(y), g, be, bias, 0, cfg)[0] == -2
        else:
            out, st = check_fold(lib, wt, rows, y, g, be, z, bias, 0, cfg)
            note(key, "fold", R.worst_ratio(out[:M], *R.input_ln(wt, z, st[:M], g, be, bias)))
        _, g, be, z, stats = R.ln_stream(M, N, rng)
        gn = (1.0 + rng.standard_normal(N) * 0.3).astype(F)
        out, st, part = launch(lib, wt, rows, x, bias, 2, cfg, res=z, res_ln=(stats, g, be), gn=gn)
        ref = R.ResidualLn(wt, x, bias, z, stats, g, be, gn)
        note(key, "resln", R.worst_ratio(out[:M], ref.ref, ref.bound))
        note(key, "partials", max(R.worst_ratio(part[:, :M, 0], ref.s, ref.s_bound),
                                  R.worst_ratio(part[:, :M, 1], ref.q, ref.q_bound)))
    assert max(WORST[key].values()) <= 1.0, WORST[key]


# ---------------------------------------------------------------- b. exact integers

@pytest.mark.parametrize("cfg", R.CONFIGS)
@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_exact_integers(lib, fmt, cfg):
    """Operands whose every partial sum is a multiple of 1/4 below 2^13: the f32 accumulator is
    exact in any order, so the output is float16(want) bit for bit -- at one K-step, one unrolled
    triple and K = 3072, at every launched row count 64 .. 320; a config whose row tile does not
    divide the rows runs the next smaller one (2, 11 -> 3 at 128; 3 -> 4 at 64, 192, 320)."""
    ran = set()
    for c, rows, N, K, res, seed in R.integer_battery(fmt):
        if c != cfg:
            continue
        wt, x, bias, r, want = R.integer_case(fmt, N, K, rows, seed, res)
        assert R.integer_condition(wt, x, bias, r, want) >= 0.99
        out, _, _ = launch(lib, wt, rows, x, bias, 2 if res else 0, cfg, res=r)
        ran.add(lib.bertx_test_gemm_ran())
        bad = out.view(np.uint16) != want.astype(H).view(np.uint16)
        assert not bad.any(), (rows, K, res, lib.bertx_test_gemm_ran(), np.argwhere(bad)[:4])
    assert ran == {R.ran_cfg(cfg, rows) for rows in R.INTEGER_ROWS}, ran
    print("\n%s cfg %d: exact at rows %s, ran %s" % (R.FMTS[fmt], cfg, R.INTEGER_ROWS, sorted(ran)))


# ---------------------------------------------------------------- c. one-hot decode

@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_onehot_decode(lib, fmt):
    """X row m is 1 at k = pi(m): the output is w[n][pi(m)] exactly, every (feature, k) position
    and the one-rounding dequantization of each format bit for bit; for fmt 0 the residual -hi
    returns f16(lo), the only way the lo plane shows in an f16 output."""
    for K in (64, 256):
        N = 160
        rng = np.random.default_rng(fmt + K)
        wt = R.random_weights(fmt, N, K, rng)
        x, pi = R.onehot_x(K), R.onehot_map(K)
        zero = np.zeros(N, F)
        for cfg in R.CONFIGS:
            out, _, _ = launch(lib, wt, K, x, zero, 0, cfg)
            want = wt.value()[:, pi].T.astype(H)
            bad = out != want                  # (by value: a zero weight of either sign sums to +0)
            assert not bad.any(), (K, cfg, np.argwhere(bad)[:4])
            if fmt == 0:
                hi = wt.hi[:, pi].T.astype(H)
                out, _, _ = launch(lib, wt, K, x, zero, 2, cfg, res=-hi)
                assert np.array_equal(out, wt.lo[:, pi].T.astype(H)), (K, cfg)


# ---------------------------------------------------------------- d. the small-batch shapes

def heuristic_ran(fmt, cus):
    if cus != 256:
        pytest.skip("the tile choices are pinned for the 256 CUs of an MI355X in SPX mode, this device has %d" % cus)
    return 4 if fmt in (0, 1) else 16          # small batches: 64 x 64, 2 waves for f16 weights, else 4


@pytest.mark.parametrize("N,K", [(1152, 384), (384, 1536), (2304, 768)])
@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_small_batch_shapes(lib, fmt, N, K):
    """The projections of MiniLM and bge-base at the row counts the small-batch forward launches,
    under the heuristic (cfg 0): the per-element bound on random operands and the exact integers."""
    want_ran = heuristic_ran(fmt, lib.bertx_test_cu_count())
    key = "%s %dx%d" % (R.FMTS[fmt], N, K)
    rng = np.random.default_rng(fmt + N)
    wt = R.random_weights(fmt, N, K, rng)
    bias = (rng.standard_normal(N) * 0.1).astype(F)
    for rows in (64, 128, 192, 320):
        x = R.random_x(rows, K, rng)
        out, _, _ = launch(lib, wt, rows, x, bias, 0, 0, want_ran=want_ran)
        note(key, "plain0", R.worst_ratio(out, *R.plain(wt, x, bias)))
        _, g, be, z, stats = R.ln_stream(rows, K, rng)
        out, _, _ = launch(lib, wt, rows, z, bias, 0, 0, in_ln=(stats, g, be), want_ran=want_ran)
        note(key, "inln", R.worst_ratio(out, *R.input_ln(wt, z, stats, g, be, bias)))
        if N <= 1024:
            _, g, be, z, stats = R.ln_stream(rows, N, rng)
            gn = (1.0 + rng.standard_normal(N) * 0.3).astype(F)
            out, st, part = launch(lib, wt, rows, x, bias, 2, 0, res=z, res_ln=(stats, g, be), gn=gn, want_ran=want_ran)
            ref = R.ResidualLn(wt, x, bias, z, stats, g, be, gn)
            note(key, "resln", R.worst_ratio(out, ref.ref, ref.bound))
        for res in (rows % 128 == 0,):         # (the residual form at rows 128)
            iw, ix, ib, ir, want = R.integer_case(fmt, N, K, rows, 31 * rows + fmt + res, res)
            assert R.integer_condition(iw, ix, ib, ir, want) >= 0.99
            out, _, _ = launch(lib, iw, rows, ix, ib, 2 if res else 0, 0, res=ir, want_ran=want_ran)
            assert bits_equal(out, want.astype(H)), (rows, res)
    assert max(WORST[key].values()) <= 1.0, WORST[key]


@pytest.mark.parametrize("N,K", [(1152, 384), (2304, 768)])
@pytest.mark.parametrize("fmt", [1, 2, 3, 8])
def test_statistics_fold_small_rows(lib, fmt, N, K):
    """The statistics fold at the rows it exists for (64, 128) with G = 12 and 24 groups, under
    the heuristic and on each fold config: the output is bitwise the same launch given the
    statistics, the statistics bitwise ln_stats's."""
    want0 = heuristic_ran(fmt, lib.bertx_test_cu_count())
    rng = np.random.default_rng(fmt + K)
    wt = R.random_weights(fmt, N, K, rng)
    bias = (rng.standard_normal(N) * 0.1).astype(F)
    for rows in (64, 128):
        y, g, be, z, _ = R.ln_stream(rows, K, rng)
        for cfg in (0, 3, 4, 16):
            want_ran = want0 if cfg == 0 else None
            for epi in (0, 1):
                out, st = check_fold(lib, wt, rows, y, g, be, z, bias, epi, cfg, want_ran)
                ref, _, _ = launch(lib, wt, rows, z, bias, epi, cfg, in_ln=(st, g, be), want_ran=want_ran)
                assert bits_equal(out, ref), (rows, cfg, epi)


def test_statistics_fold_cfg3_capacity(lib):
    """cfg 3 holds 24 partial groups only where its tiles are at most one per CU: on the far side
    of that rule d = 384 (12 groups) still folds, bitwise as above, and d = 768 is refused (-2)."""
    cus = lib.bertx_test_cu_count()
    N, rows = 128 * (cus + 1), 128
    rng = np.random.default_rng(5)
    for K, ok in ((384, True), (768, False)):
        wt = R.Weights(1, (rng.standard_normal((N, K)) * 0.05).astype(H).tobytes(), N, K)
        bias = (rng.standard_normal(N) * 0.1).astype(F)
        y, g, be, z, _ = R.ln_stream(rows, K, rng)
        if not ok:
            assert launch_fold(lib, wt, rows, z, R.group_partials(y), g, be, bias, 0, 3)[0] == -2
            continue
        out, st = check_fold(lib, wt, rows, y, g, be, z, bias, 0, 3)
        ref, _, _ = launch(lib, wt, rows, z, bias, 0, 3, in_ln=(st, g, be))
        assert bits_equal(out, ref)


# ---------------------------------------------------------------- e. the persistent walk

@pytest.mark.parametrize("cfg,row_tiles,fmts", [(4, 16, (0, 1, 2, 3, 8)), (16, 16, (0, 1, 2, 3, 8)), (3, 8, (1, 3)),
                                                (2, 8, (1, 2))])
def test_persistent_walk(lib, cfg, row_tiles, fmts):
    """A grid smaller than the tile count (two workgroups per CU walking the tiles: dispatch_z
    takes that form for OCC cus < tiles <= 2 OCC cus on whole column tiles), sized from the
    device's CU count; K = 64, integers, bit for bit."""
    if os.environ.get("BERT_GEMM_PERSIST") is not None:
        pytest.skip("BERT_GEMM_PERSIST overrides the grid this test is about")
    cus = lib.bertx_test_cu_count()
    col_tiles = R.OCC * cus // row_tiles + 1
    tiles, rows, N = row_tiles * col_tiles, row_tiles * R.ROW_TILE[cfg], col_tiles * R.COL_TILE[cfg]
    assert R.OCC * cus < tiles <= 2 * R.OCC * cus and N % R.COL_TILE[cfg] == 0, (cus, tiles)
    for fmt in fmts:
        for res in (False, True):
            wt, x, bias, r, want = R.integer_case(fmt, N, 64, rows, 7 * cfg + fmt + res, res)
            assert R.integer_condition(wt, x, bias, r, want) >= 0.99
            out, _, _ = launch(lib, wt, rows, x, bias, 2 if res else 0, cfg, res=r)
            bad = out.view(np.uint16) != want.astype(H).view(np.uint16)
            assert not bad.any(), (fmt, res, np.argwhere(bad)[:4])
    print("\ncfg %d: %d tiles on %d workgroups (%d CUs), rows %d, N %d" % (cfg, tiles, R.OCC * cus, cus, rows, N))


# ---------------------------------------------------------------- f. the residual partials

@pytest.mark.parametrize("N", [64, 384, 1024])
@pytest.mark.parametrize("fmt", [1, 3])
def test_residual_partials(lib, fmt, N):
    """The per-group (sum, squared deviations) the residual epilogue writes, every group and row,
    within their bound of the float64 ones, and ln_stats of them against two-pass statistics at
    the bound that follows (gemm_refs.stats_bound)."""
    K, M, rows = 128, 250, 256
    rng = np.random.default_rng(fmt + N)
    wt = R.random_weights(fmt, N, K, rng)
    bias = (rng.standard_normal(N) * 0.1).astype(F)
    x = R.random_x(M, K, rng)
    _, g, be, z, stats = R.ln_stream(M, N, rng)
    gn = (1.0 + rng.standard_normal(N) * 0.3).astype(F)
    ref = R.ResidualLn(wt, x, bias, z, stats, g, be, gn)
    st_ref, st_bound = ref.stats()
    key = "%s partials" % R.FMTS[fmt]
    for cfg in R.CONFIGS:
        out, st, part = launch(lib, wt, rows, x, bias, 2, cfg, res=z, res_ln=(stats, g, be), gn=gn)
        note(key, "out", R.worst_ratio(out[:M], ref.ref, ref.bound))
        note(key, "s", R.worst_ratio(part[:, :M, 0], ref.s, ref.s_bound))
        note(key, "q", R.worst_ratio(part[:, :M, 1], ref.q, ref.q_bound))
        note(key, "stats", R.worst_ratio(st[:M], st_ref, st_bound))
        assert max(WORST[key].values()) <= 1.0, (cfg, WORST[key])
        # the statistics are ln_row_stats of exactly these partials
        assert np.allclose(st[:M], R.ln_row_stats_f32(np.ascontiguousarray(part[:, :M]), N), rtol=5e-7, atol=1e-12)


# ---------------------------------------------------------------- g. the GELU epilogue

def test_gelu_every_normal_f16_input(lib):
    """One launch whose accumulator is each normal f16 value exactly (gemm_refs.gelu_input_launch):
    the epilogue against the era table, within the numpy restatement's measured worst distance
    plus two steps each for v_exp_f16 and v_rcp_f16 (GELU_STEPS_DEVICE), and within 2^-13 where
    |T| < 2^-13 (results the f16 overflow of exp2 flushes)."""
    W, X, acc = R.gelu_input_launch()
    wt = R.Weights(1, W.astype(H).tobytes(), 1024, 64)
    for cfg in (4, 3):
        out, _, _ = launch(lib, wt, 128 if cfg == 3 else 64, X, np.zeros(1024, F), 1, cfg)
        steps, small = R.gelu_distance(out[:60], acc[:60])
        print("\ngelu8_era cfg %d over %d inputs: worst %d f16 steps from the table where |T| >= 2^-13 (restated %d), "
              "worst |error| %.3g below" % (cfg, acc[:60].size, steps, R.GELU_STEPS_RESTATED, small))
        assert steps <= R.GELU_STEPS_DEVICE and small <= R.GELU_FLOOR, (steps, small)
        assert not out[60:64].any()            # gelu(0) = 0


@pytest.mark.parametrize("fmt", [2, 3, 8])
def test_gelu_dequantized(lib, fmt):
    """The GELU epilogue behind a dequantized product: against T(f16(reference accumulator)),
    allowing the accumulator's own bound and one input step (the sum may round to the neighbouring
    table entry; GELU's slope is at most 1.13) and the epilogue's distance from the table."""
    N, K, M = 96, 64, 64
    rng = np.random.default_rng(fmt)
    wt = R.random_weights(fmt, N, K, rng)
    x = R.random_x(M, K, rng)
    bias = (rng.standard_normal(N) * 0.1).astype(F)
    for cfg in R.CONFIGS:
        out, _, _ = launch(lib, wt, R.ROW_TILE[cfg], x, bias, 1, cfg)
        acc, A, n = R.plain_f32(wt, x, bias)
        x16 = acc.astype(H)
        T = R.era_gelu_table()[x16.view(np.uint16)].astype(D)
        delta = 2 * (wt.Ke + n) * R.U * A
        ulp_in = np.spacing(np.abs(x16)).astype(D)
        ulp = np.spacing(np.abs(T).astype(H)).astype(D)
        tol = 1.2 * (delta + ulp_in) + np.where(np.abs(T) >= R.GELU_FLOOR, R.GELU_STEPS_DEVICE * ulp, R.GELU_FLOOR)
        err = np.abs(out[:M].astype(D) - T)
        note("%s gelu" % R.FMTS[fmt], "cfg%d" % cfg, float((err / tol).max()))
        assert (err <= tol).all(), (cfg, float((err / tol).max()))


# ---------------------------------------------------------------- h. out of place

@pytest.mark.parametrize("fmt", sorted(R.FMTS))
def test_out_of_place_residual(lib, fmt):
    """res != out gives the in-place bits, for the plain residual and the LN form (output,
    partials and statistics)."""
    N, K, M, rows = 160, 192, 125, 128
    rng = np.random.default_rng(fmt)
    wt = R.random_weights(fmt, N, K, rng)
    bias = (rng.standard_normal(N) * 0.1).astype(F)
    x = R.random_x(M, K, rng)
    _, g, be, z, stats = R.ln_stream(M, N, rng)
    gn = (1.0 + rng.standard_normal(N) * 0.3).astype(F)
    for cfg in (3, 16):
        a = launch(lib, wt, rows, x, bias, 2, cfg, res=z)
        b = launch(lib, wt, rows, x, bias, 2, cfg, res=z, oop=1)
        assert bits_equal(a[0], b[0])
        a = launch(lib, wt, rows, x, bias, 2, cfg, res=z, res_ln=(stats, g, be), gn=gn)
        b = launch(lib, wt, rows, x, bias, 2, cfg, res=z, res_ln=(stats, g, be), gn=gn, oop=1)
        for u, v in zip(a, b):
            assert bits_equal(u, v)
