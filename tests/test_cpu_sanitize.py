"""ASan + UBSan runs of the host C++ (tokenizer, model-file loader, quantizer, converter)
and of the C oracle, as standalone programs built by tests/sanitize/Makefile (SURVEY §5:
sanitizers on host code only; GPU sanitizers are unavailable on this pool).  Each run
must exit 0 with no sanitizer report and give the same results as the production build."""
import fcntl
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_cpu_abi import _parse_model_file, _write_hf_dir

SAN = os.path.join(ROOT, "tests", "sanitize")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def harness():
    # one build at a time: pytest-xdist workers each run this fixture, and a worker
    # must not exec a harness another worker's make is still linking
    with open(os.path.join(SAN, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", SAN, "-j2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(SAN, "_build")


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=ENV, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def write_blobs(path, blobs, with_nmax=None):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)))
        for i, b in enumerate(blobs):
            if with_nmax is not None:
                f.write(struct.pack("<i", with_nmax[i]))
            f.write(struct.pack("<I", len(b)))
            f.write(b)


def read_ids(path, n_max):
    out, data, o = [], open(path, "rb").read(), 0
    for nm in n_max:
        (n,) = struct.unpack_from("<i", data, o)
        o += 4
        w = min(n, nm)
        out.append((n, list(struct.unpack_from("<%di" % w, data, o)) if w > 0 else []))
        o += 4 * max(w, 0)
    assert o == len(data)
    return out


def random_texts(n, seed):
    """ASCII, punctuation, accents, CJK, emoji and invalid UTF-8 bytes."""
    rnd = random.Random(seed)
    pieces = [b"hello", b"World", b" ", b"  ", b"\t", b"\n", b"!", b"?", b"x!x", b"caf\xc3\xa9", b"\xc3\x80",
              b"\xe4\xb8\xad\xe6\x96\x87", b"\xe3\x80\x82", b"\xef\xbc\x8c", b"\xf0\x9f\x98\x80", b"\xff", b"\xc3",
              b"##", b"w12", b"w3", b"[UNK]", b"a" * 700]
    return [b"".join(rnd.choice(pieces) for _ in range(rnd.randint(0, 40))) for _ in range(n)]


def test_tokenizer_under_sanitizers(harness, tmp_path, tok_golden, lib, monkeypatch):
    vocab = [v.encode("utf-8") for v in tok_golden["vocab"]]
    cases = tok_golden["cases"]
    texts = [bytes.fromhex(c["text_hex"]) for c in cases]
    n_max = [c["n_max_tokens"] for c in cases]
    extra = random_texts(200, 3)
    texts += extra
    n_max += [random.Random(i).choice([1, 2, 8, 64, 512]) for i in range(len(extra))]
    write_blobs(tmp_path / "vocab.bin", vocab)
    write_blobs(tmp_path / "texts.bin", texts, n_max)
    run(os.path.join(harness, "host_harness"), "tok", tmp_path / "vocab.bin", tmp_path / "texts.bin",
        tmp_path / "ids.bin")
    got = read_ids(tmp_path / "ids.bin", n_max)
    for c, (n, ids) in zip(cases, got):
        assert n == len(c["ids"]) and ids == c["ids"][: c["n_max_tokens"]]
    # the random texts: same ids as the production library's tokenizer
    import bertpy
    monkeypatch.setenv("BERT_HOST_ONLY", "1")
    m = bertpy.BertModel(os.path.join(GOLDEN, "tiny32", "ggml-model-f32.bin"))
    write_blobs(tmp_path / "vocab2.bin", [m.id_to_token(i) for i in range(m.hparams()[0])])
    write_blobs(tmp_path / "texts2.bin", extra, n_max[len(cases):])
    run(os.path.join(harness, "host_harness"), "tok", tmp_path / "vocab2.bin", tmp_path / "texts2.bin",
        tmp_path / "ids2.bin")
    for t, nm, (n, ids) in zip(extra, n_max[len(cases):], read_ids(tmp_path / "ids2.bin", n_max[len(cases):])):
        ref, rn = m.tokenize(t, nm)
        assert (n, ids) == (rn, ref[:nm])


@pytest.mark.parametrize("tiny", ["tiny32", "tiny64"])
def test_loader_quantizer_under_sanitizers(harness, tmp_path, lib, tiny):
    exe = os.path.join(harness, "host_harness")
    src = os.path.join(GOLDEN, tiny, "ggml-model-f16.bin")
    for ft in ("f32", "f16"):
        run(exe, "load", os.path.join(GOLDEN, tiny, f"ggml-model-{ft}.bin"))
    for it in (2, 3, 8):
        out = tmp_path / f"q{it}.bin"
        run(exe, "quant", src, out, it)
        ref = tmp_path / f"ref{it}.bin"
        assert lib.bertx_quantize_file(src.encode(), str(ref).encode(), it) == 0
        assert open(out, "rb").read() == open(ref, "rb").read()
        hp = run(exe, "load", out).split()
        assert int(hp[6]) == it
    # a truncated file is refused cleanly (no out-of-bounds read)
    data = open(src, "rb").read()
    (tmp_path / "trunc.bin").write_bytes(data[: len(data) // 2])
    r = subprocess.run([exe, "load", str(tmp_path / "trunc.bin")], capture_output=True, text=True, env=ENV)
    assert r.returncode == 5 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


BLOCK_BYTES = {0: 128, 1: 64, 2: 18, 3: 20, 8: 34}   # per 32 elements, by file format (ggml type id)


def _file_rows(fmt, rows, N, K):
    """File-format rows [N][K] -> (codes [N][K], d [N][K/32] f16 bits, m likewise or None,
    w [N][K] f32 as dequantized): codes are f16 bits (f16), nibbles (q4_0 / q4_1: element
    e < 16 the low nibble of byte e, else the high nibble of byte e - 16) or int8 (q8_0)."""
    b = np.frombuffer(rows, np.uint8).reshape(N, K // 32, BLOCK_BYTES[fmt])
    if fmt == 1:
        codes = b.reshape(N, -1).view(np.uint16)
        return codes, None, None, codes.view(np.float16).astype(np.float32)
    d = np.ascontiguousarray(b[:, :, 0:2]).view(np.uint16)[:, :, 0]
    df = d.view(np.float16).astype(np.float32)[:, :, None]
    if fmt == 8:
        q = np.ascontiguousarray(b[:, :, 2:]).view(np.int8)
        return q.reshape(N, K), d, None, (q.astype(np.float32) * df).reshape(N, K)
    nib = b[:, :, (4 if fmt == 3 else 2):]
    q = np.concatenate([nib & 15, nib >> 4], axis=2)
    if fmt == 2:
        return q.reshape(N, K), d, None, ((q.astype(np.float32) - 8) * df).reshape(N, K)
    m = np.ascontiguousarray(b[:, :, 2:4]).view(np.uint16)[:, :, 0]
    mf = m.view(np.float16).astype(np.float32)[:, :, None]
    return q.reshape(N, K), d, m, (q.astype(np.float32) * df + mf).reshape(N, K)


def _lane_order(fmt, codes, d, m):
    """The lane-order layout as the top of kernels.h describes it: per K-step ks (64 k:
    blocks 2ks, 2ks + 1) and 32-feature group grp, 64 lane records; lane 16g + f holds the
    fragments u = 2a + s = feature 32grp + 16a + f, block 2ks + s, elements 8g .. 8g + 7."""
    N, K = codes.shape
    x = codes.reshape(N // 32, 2, 16, K // 64, 2, 4, 8)          # grp a f ks s g i
    x = x.transpose(3, 0, 5, 2, 1, 4, 6).reshape(K // 64, N // 32, 64, 4, 8)   # ks grp lane u i
    if fmt == 1:
        qs = x.astype("<u2").tobytes()                           # 64 B per lane
    elif fmt == 8:                                               # 8 B per u: e0 e2 e1 e3 per 4-group, ^ 0x80
        y = x.reshape(x.shape[:-1] + (2, 4))[..., [0, 2, 1, 3]]
        qs = (y.astype(np.int8).view(np.uint8) ^ 0x80).tobytes()
    else:                                                        # one word per u: element i at bit 4(i/2) + 16(i%2)
        sh = np.array([4 * (i // 2) + 16 * (i % 2) for i in range(8)], np.uint32)
        qs = np.bitwise_or.reduce(x.astype(np.uint32) << sh, axis=-1).astype("<u4").tobytes()

    def plane(p):                                                # f16 [ks][grp][f][u]
        if p is None:
            return b""
        y = p.reshape(N // 32, 2, 16, K // 64, 2).transpose(3, 0, 2, 1, 4)
        return np.ascontiguousarray(y).astype("<u2").tobytes()
    return qs, plane(d), plane(m)


def test_repack_under_sanitizers(harness, tmp_path):
    """The weight layout code (repack.cpp) under ASan + UBSan over the tiny64 files in all
    five formats (every table, every layer's linear weights and LN folds), and the dump of
    one weight against restatements that share no code with it.  tiny64 (n_embd 64) has
    one K-step, so the harness dumps its synthetic [64][128] weight: two 32-feature groups,
    two K-steps, two parts.  The qs / d / m planes are compared byte for byte with
    _lane_order.  c1 / c2 are compared for exact f32 equality: the restatement adds the
    float64 products in the loop's own left-to-right order (np.cumsum) and makes the same
    double -> float casts, so not even the last bit is free (a pairwise np.dot would need
    a 1-ulp allowance for sums that land next to a rounding boundary)."""
    exe = os.path.join(harness, "host_harness")
    files = {ft: os.path.join(GOLDEN, "tiny64", f"ggml-model-{ft}.bin") for ft in ("f32", "f16")}
    for name, it in (("q4_0", 2), ("q4_1", 3), ("q8_0", 8)):
        files[name] = str(tmp_path / f"{name}.bin")
        run(exe, "quant", files["f16"], files[name], it)
    for name, path in files.items():
        dump = tmp_path / f"{name}.repack"
        fmt, N, K = map(int, run(exe, "repack", path, dump).split())
        data = open(dump, "rb").read()
        hdr = np.frombuffer(data, "<i4", 8)
        assert (hdr[0], hdr[1]) == (fmt, N) and N >= 64 and hdr[2] >= 128, hdr
        Kf = int(hdr[2])                                         # K of the file rows (f32 files: K = 2 Kf)
        o = 32

        def take(n):
            nonlocal o
            o += n
            return data[o - n:o]
        rows = take(N * (Kf // 32) * BLOCK_BYTES[fmt])
        gamma, beta, bias = (np.frombuffer(take(4 * n), "<f4").astype(np.float64) for n in (Kf, Kf, N))
        qs, dpl, mpl, c1, c2 = (take(int(n)) for n in hdr[3:8])
        assert o == len(data)
        if fmt == 0:
            # f32 files: rows [hi | lo] of f16 pairs along a doubled K, hi = f16(w), lo = f16(w - hi)
            w = np.frombuffer(rows, "<f4").reshape(N, Kf)
            hi = w.astype(np.float16)
            lo = (w - hi.astype(np.float32)).astype(np.float16)
            assert K == 2 * Kf
            want = _lane_order(1, np.concatenate([hi, lo], axis=1).view(np.uint16), None, None)
            wq = w.astype(np.float64)                            # the fold takes the f32 value itself
        else:
            assert K == Kf
            codes, d, m, w = _file_rows(fmt, rows, N, Kf)
            want = _lane_order(fmt, codes, d, m)
            wq = w.astype(np.float16).astype(np.float64)         # rounded once to f16, as the GEMM multiplies it
        assert (qs, dpl, mpl) == want, name
        assert len(dpl) == (0 if fmt in (0, 1) else N * (Kf // 32) * 2) and (len(mpl) > 0) == (fmt == 3)
        s1 = np.cumsum(wq * gamma, axis=1)[:, -1].astype(np.float32)
        s2 = np.cumsum(wq * beta, axis=1)[:, -1].astype(np.float32)
        s2 = (s2.astype(np.float64) + bias).astype(np.float32)
        assert np.array_equal(np.frombuffer(c1, "<f4"), s1), name
        assert np.array_equal(np.frombuffer(c2, "<f4"), s2), name


def test_converter_under_sanitizers(harness, tmp_path):
    ref32 = os.path.join(GOLDEN, "tiny32", "ggml-model-f32.bin")
    hp, vocab, tens = _parse_model_file(ref32)
    d = str(tmp_path / "hf")
    _write_hf_dir(d, hp, vocab, tens, prefix="bert.", shards=2)
    for ft, fn in ((0, "ggml-model-f32.bin"), (1, "ggml-model-f16.bin")):
        out = tmp_path / fn
        run(os.path.join(harness, "host_harness"), "convert", d, out, ft)
        assert open(out, "rb").read() == open(os.path.join(GOLDEN, "tiny32", fn), "rb").read()


def test_oracle_under_sanitizers(harness, tmp_path, oracle):
    path = os.path.join(GOLDEN, "tiny64", "ggml-model-f32.bin")
    o = oracle.Oracle(path)
    rng = np.random.default_rng(4)
    lens = [1, 2, 17, 64, o.n_max_tokens]
    ids = [np.concatenate([[101], rng.integers(104, o.n_vocab, max(L - 2, 0)), [102]])[:L].astype(np.int32)
           for L in lens]
    with open(tmp_path / "ids.bin", "wb") as f:
        f.write(struct.pack("<I", len(ids)))
        for x in ids:
            f.write(struct.pack("<I", len(x)))
            f.write(x.tobytes())
    run(os.path.join(harness, "oracle_harness"), "fwd", path, tmp_path / "ids.bin", tmp_path / "out.bin")
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(len(ids), -1)
    ref = o.forward_batch(ids)
    assert np.allclose(got, ref, rtol=0, atol=1e-6)
