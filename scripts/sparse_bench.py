#!/usr/bin/env python3
"""The SPLADE sparse head: its two kernels alone and the whole forward.

Every figure is the median of R rounds with its min-max spread; a round is one
bertx_bench_* call (3 warm-up launches, then `iters` timed launches between two device
events) or one forward ending in a device synchronise.

--kernel   bertx_bench_sparse at bge-base dims (d 768, V 30,522) for 64 x 512, 64 x 32 and
           1 x 32 tokens: microseconds and TF/s of the transform (2 T d^2 FLOP) and the
           decoder (2 T d V FLOP, its fill and log1p launches included), as fractions of
           FFN-up's rate measured in the same process (bertx_bench_gemm, q4_0, N 3072, K
           768, the same token count padded to 256) and of the 2.5 PF/s f16 peak; the bytes
           an unfused head would write (4 T V) against the bytes this one moves.
--forward  a synthetic bge-base f16 model with a seeded masked-LM head: a BERTX_OUT_SPARSE
           forward against a BERTX_OUT_TOKENS forward of the same device-resident batch.
One JSON line per point into --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))

import bertpy  # noqa: E402

PEAK = 2.5e15
D, V = 768, 30522
SHAPES = [(64, 512), (64, 32), (1, 32)]


def spread(t):
    return {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}


def kernel_part(lib, rounds, emit):
    for n_seqs, length in SHAPES:
        T = n_seqs * length
        iters = 5 if T > 4096 else 50
        tf, dc, up = [], [], []
        us2, us = (ctypes.c_float * 2)(), ctypes.c_float()
        M = (T + 255) // 256 * 256
        for _ in range(rounds):
            assert lib.bertx_bench_sparse(D, V, n_seqs, length, iters, us2) == 0
            tf.append(us2[0])
            dc.append(us2[1])
            assert lib.bertx_bench_gemm(2, 3072, D, M, 1, 0, iters, ctypes.byref(us)) == 0
            up.append(us.value)
        rec = {"part": "kernel", "d": D, "V": V, "n_seqs": n_seqs, "len": length, "T": T, "rounds": rounds, "iters": iters,
               "transform_us": spread(tf), "decoder_us": spread(dc), "ffn_up_us": spread(up)}
        up_tf = 2.0 * M * 3072 * D / (rec["ffn_up_us"]["median"] * 1e-6)
        for name, flop in (("transform", 2.0 * T * D * D), ("decoder", 2.0 * T * D * V)):
            rate = flop / (rec[name + "_us"]["median"] * 1e-6)
            rec[name + "_TFps"] = round(rate / 1e12, 2)
            rec[name + "_of_ffn_up"] = round(rate / up_tf, 3)
            rec[name + "_of_peak"] = round(rate / PEAK, 4)
        rec["ffn_up_TFps"] = round(up_tf / 1e12, 2)
        Vp = (V + 127) // 128 * 128
        rec["unfused_logit_bytes"] = 4 * T * V
        # source rows, h written and read, both images once, the output filled, updated and finished
        rec["moved_bytes"] = T * D * 2 + 2 * T * D * 2 + 2 * D * D + 2 * Vp * D + 3 * 4 * n_seqs * V
        emit(rec)


def forward_part(lib, rounds, emit, model_dir):
    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, "bge-base-f16-mlm.bin")
    if not os.path.exists(path):
        bertpy.synthetic_model(path + ".plain", "bge-base-en-v1.5", "f16")
        rng = np.random.default_rng(9)
        t = {bertpy.MLM_NAMES[0]: (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32),
             bertpy.MLM_NAMES[1]: np.zeros(D, np.float32), bertpy.MLM_NAMES[2]: np.ones(D, np.float32),
             bertpy.MLM_NAMES[3]: np.zeros(D, np.float32), bertpy.MLM_NAMES[4]: np.zeros(V, np.float32)}
        bertpy.append_mlm_head(path + ".plain", path, t)
        os.remove(path + ".plain")
    os.environ["BERT_DEVICES"] = "0"
    m = bertpy.BertModel(path)
    hip = ctypes.CDLL("libamdhip64.so.7")
    vp = ctypes.c_void_p
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipStreamSynchronize.argtypes = [vp]

    def dev(a):
        p = vp()
        assert hip.hipMalloc(ctypes.byref(p), max(a.nbytes, 16)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p
    s = vp()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    for n_seqs, length in SHAPES:
        T = n_seqs * length
        rng = np.random.default_rng(1)
        ids = rng.integers(1000, V, T).astype(np.int32)
        cu = (np.arange(n_seqs + 1) * length).astype(np.int32)
        d_ids, d_cu = dev(ids), dev(cu)
        d_out = dev(np.zeros(max(T * D, n_seqs * V), np.float32))
        assert lib.bertx_reserve(m.ctx, 0, T, n_seqs) == 0
        rec = {"part": "forward", "n_seqs": n_seqs, "len": length, "rounds": rounds}
        for name, kind in (("tokens", 1), ("sparse", 4)):
            t = []
            for r in range(rounds + 3):
                t0 = time.perf_counter()
                assert m.forward_device_ex(0, d_ids, None, d_cu, n_seqs, length, T, kind, d_out, s) == 0
                assert hip.hipStreamSynchronize(s) == 0
                if r >= 3:
                    t.append((time.perf_counter() - t0) * 1e3)
            rec[name + "_ms"] = spread(t)
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--models", default=os.path.join(ROOT, "models"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_bench.jsonl"))
    a = ap.parse_args()
    lib = bertpy.load_lib()
    with open(a.out, "a") as f:
        def emit(rec):
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            f.flush()
        if a.kernel:
            kernel_part(lib, a.rounds, emit)
        if a.forward:
            forward_part(lib, a.rounds, emit, a.models)


if __name__ == "__main__":
    main()
