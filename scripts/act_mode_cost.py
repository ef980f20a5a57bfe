#!/usr/bin/env python3
"""What the q8-activation mode costs: the same file, the same build, one
process, f16 activations (the default) against the reference's q8 activations
(BertModel(act="q8"), csrc/q8act.hip), at

    c3   bge-base-en-v1.5 q4_0, 64 sentences of 512 tokens (the flagship batch)
    b1   one sentence of 32 tokens (latency)

through bert_forward_batch (host ids in, host embeddings out, synchronous: the call ends in
a device synchronise).  Per shape: warm-up calls of both modes (the graph is captured on the
second use of a shape), then `--rounds` alternating windows of `--iters` calls per mode; the
figure is the median window with the min-max spread.  Then one profiled pass per mode
(bertx_set_profiling: device events around every launch, no graph) for the per-class times
of bertx_kernel_stats -- in the q8 mode each projection's class includes its quantize launch.
One JSON line per (shape, mode) into --out.  There is no target: the number is what a user
choosing the mode pays.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))

import bertpy  # noqa: E402

SHAPES = {"c3": (64, 512), "b1": (1, 32)}


def window(m, ids, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        m.forward_batch(ids)
    return (time.perf_counter() - t0) / iters


def profiled(m, ids, iters):
    m.lib.bertx_set_profiling(m.ctx, 1)
    m.forward_batch(ids)
    m.lib.bertx_reset_stats(m.ctx)
    for _ in range(iters):
        m.forward_batch(ids)
    st = m.kernel_stats()
    m.lib.bertx_set_profiling(m.ctx, 0)
    return {k["name"]: round(k["ms"] / iters, 4) for k in st if k["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="bge-base-en-v1.5")
    ap.add_argument("--ftype", default="q4_0")
    ap.add_argument("--shapes", default="c3,b1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", default="c3=8,b1=300")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q8act_cost.jsonl"))
    ap.add_argument("--model-dir", default="/tmp/act_mode_cost")
    a = ap.parse_args()
    os.makedirs(a.model_dir, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    os.environ.setdefault("BERT_DEVICES", "0")
    os.environ.pop("BERT_ACT", None)
    iters = {k: int(v) for k, v in (x.split("=") for x in a.iters.split(","))}
    hp = bertpy.ARCHS[a.arch]
    path = os.path.join(a.model_dir, f"{a.arch}-{a.ftype}.bin")
    if not os.path.exists(path):
        bertpy.synthetic_model(path, a.arch, a.ftype, seed=1234)
    models = {"f16": bertpy.BertModel(path, act="f16"), "q8": bertpy.BertModel(path, act="q8")}
    assert models["f16"].activation_mode == 0 and models["q8"].activation_mode == 1
    with open(a.out, "a") as f:
        for shape in a.shapes.split(","):
            n, L = SHAPES[shape]
            ids = bertpy.synthetic_ids(n, L, hp["n_vocab"], seed=7)
            outs = {}
            for name, m in models.items():
                for _ in range(3):
                    outs[name] = m.forward_batch(ids)
            cosv = np.sum(outs["f16"] * outs["q8"], axis=1)
            times = {name: [] for name in models}
            for _ in range(a.rounds):
                for name, m in models.items():      # alternating windows
                    times[name].append(window(m, ids, iters[shape]))
            for name, m in models.items():
                t = np.array(times[name])
                rec = {"shape": shape, "sentences": n, "len": L, "arch": a.arch, "ftype": a.ftype, "act": name,
                       "call_ms_median": round(float(np.median(t)) * 1e3, 4),
                       "call_ms_min": round(float(t.min()) * 1e3, 4), "call_ms_max": round(float(t.max()) * 1e3, 4),
                       "sentences_per_s": round(n / float(np.median(t)), 1),
                       "rounds": a.rounds, "iters": iters[shape],
                       "class_ms_per_call": profiled(m, ids, max(2, iters[shape] // 4)),
                       "min_cos_f16_vs_q8": round(float(cosv.min()), 7)}
                f.write(json.dumps(rec) + "\n")
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
