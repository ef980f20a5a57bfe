#!/usr/bin/env python3
"""Key counts on the attention kernels ("Key counts"): what they cost where
they are not used, what they save where they are, and what a ColBERT query forward pays.

Every figure is the median of R rounds after warm-up rounds, with its min-max spread, from
device events (the library's bench hooks, torch events around a forward) or the library's own
per-kernel device timing (bertx_kernel_stats).

--baseline PARENT_LIB  `bench.py --gpus 1` (its flagship leg alone) on this build and on the
           parent commit's libbert.so, alternating, P pairs: ms_per_step of each.  The workload
           uses no key counts: the expectation is no difference.
--kernel   bertx_bench_attention_kv at dh 64, 12 heads, 64 sentences: len 512 with keys 512,
           256, 64, 1 and len 32 with keys 32, 8; keys == len also through
           bertx_bench_attention (no counts).  Each round is one call: 3 warm-up launches,
           then the average of 10.
--query    bge-base dims, q4_0, a seeded 128-dim record, query_maxlen 32, B = 1, 64, 1,024
           queries of 10 real tokens ([CLS] [Q] 7 pieces [SEP], then 22 [MASK]): the PROJ
           forward with counts against without; the attention class of bertx_kernel_stats
           (profiled rounds) and the whole forward (torch events, graph replay).
One JSON line per point into --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bertpy  # noqa: E402

KERNEL_POINTS = [(512, 512), (512, 256), (512, 64), (512, 1), (32, 32), (32, 8)]
N_SEQS, N_HEAD, DH, ITERS = 64, 12, 64, 10
QUERY_MAXLEN, REAL_TOKENS = 32, 10


def spread(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def baseline_part(parent_lib, pairs, steps, warmup, emit):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--no-cpu-baseline", "--no-probes", "--no-library", "--no-pmc", "--no-encode"]
    ms = {"this": [], "parent": []}
    for _ in range(pairs):
        for label in ("this", "parent"):
            env = dict(os.environ)
            env.pop("BERT_LIB", None)
            if label == "parent":
                env["BERT_LIB"] = os.path.abspath(parent_lib)
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            ms[label].append(json.loads(line)["ms_per_step"])
    emit({"part": "baseline", "workload": "bench.py --gpus 1 --steps %d --warmup %d" % (steps, warmup), "pairs": pairs,
          "ms_per_step_this": spread(ms["this"]), "ms_per_step_parent": spread(ms["parent"]),
          "runs_this": ms["this"], "runs_parent": ms["parent"]})


def kernel_part(lib, rounds, warm, emit):
    us = ctypes.c_float()

    def run(fn, *args):
        t = []
        for r in range(warm + rounds):
            rc = fn(*args, 0, ITERS, ctypes.byref(us))
            assert rc == 0, rc
            if r >= warm:
                t.append(us.value)
        return spread(t)

    for ln, keys in KERNEL_POINTS:
        rec = {"part": "kernel", "n_seqs": N_SEQS, "n_head": N_HEAD, "dh": DH, "len": ln, "keys": keys,
               "blocks": (keys + 63) // 64, "rounds": rounds, "iters": ITERS,
               "us_kv": run(lib.bertx_bench_attention_kv, N_SEQS, ln, keys, N_HEAD, DH)}
        if keys == ln:
            rec["us_plain"] = run(lib.bertx_bench_attention, N_SEQS, ln, N_HEAD, DH)
        emit(rec)


def class_ms(m, name="attention"):
    for row in m.kernel_stats():
        if row["name"] == name:
            return row["ms"], row["launches"]
    raise KeyError(name)


def query_part(torch, lib, model_dir, rounds, warm, emit):
    from project_bench import model_file
    arch, dim = "bge-base-en-v1.5", 128
    m = bertpy.BertModel(model_file(model_dir, arch, dim, lib))
    hp = bertpy.ARCHS[arch]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    L = QUERY_MAXLEN
    for B in (1, 64, 1024):
        rng = np.random.default_rng(B)
        ids = np.full((B, L), 103, np.int32)
        ids[:, 0], ids[:, 1], ids[:, REAL_TOKENS - 1] = 101, 1, 102
        ids[:, 2:REAL_TOKENS - 1] = rng.integers(1000, hp["n_vocab"], (B, REAL_TOKENS - 3))
        T = B * L
        d_ids = torch.from_numpy(ids.reshape(-1)).to(dev)
        d_cu = torch.from_numpy((np.arange(B + 1) * L).astype(np.int32)).to(dev)
        d_keys = torch.full((B,), REAL_TOKENS, dtype=torch.int32, device=dev)
        out = torch.empty((T, m.proj_width), dtype=torch.float32, device=dev)
        assert lib.bertx_reserve(m.ctx, 0, T, B) == 0
        rec = {"part": "query", "arch": arch, "ftype": "q4_0", "dim": dim, "B": B, "query_maxlen": L, "keys": REAL_TOKENS,
               "rounds": rounds}

        def forward(keys, s):
            rc = lib.bertx_forward_device_kv(m.ctx, 0, ctypes.c_void_p(d_ids.data_ptr()), None,
                                             ctypes.c_void_p(d_cu.data_ptr()),
                                             ctypes.c_void_p(d_keys.data_ptr()) if keys else None, B, L, T, 3, None, 0,
                                             ctypes.c_void_p(out.data_ptr()), s)
            assert rc == 0, rc

        for keys, label in ((False, "plain"), (True, "kv")):
            # the attention class, profiled (eager launches on the replica's stream)
            lib.bertx_set_profiling(m.ctx, 1)
            t = []
            for r in range(warm + rounds):
                lib.bertx_reset_stats(m.ctx)
                forward(keys, None)
                torch.cuda.synchronize()
                ms, launches = class_ms(m)
                assert launches == hp["n_layer"], launches
                if r >= warm:
                    t.append(ms * 1e3)
            lib.bertx_set_profiling(m.ctx, 0)
            rec["attention_us_" + label] = spread(t)
            # the whole forward, events on a caller stream (captured on its second use)
            t = []
            with torch.cuda.stream(stream):
                for r in range(warm + rounds):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    forward(keys, ctypes.c_void_p(stream.cuda_stream))
                    b.record(stream)
                    b.synchronize()
                    if r >= warm:
                        t.append(a.elapsed_time(b) * 1e3)
            rec["forward_us_" + label] = spread(t)
        emit(rec)
        del d_ids, d_cu, d_keys, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_keys_bench.jsonl"))
    ap.add_argument("--baseline", metavar="PARENT_LIB")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--query", action="store_true")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-dir", default=os.path.join(ROOT, "build", "models"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "mask_keys_bench.py measures on a GPU"
    os.environ.setdefault("BERT_DEVICES", "0")
    lib = bertpy.load_lib()
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    if args.kernel:
        kernel_part(lib, args.rounds, args.warmup, emit)
    if args.query:
        query_part(torch, lib, args.model_dir, args.rounds, args.warmup, emit)
    if args.baseline:
        baseline_part(args.baseline, args.pairs, args.steps, args.warmup, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
