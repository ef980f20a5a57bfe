#!/usr/bin/env python3
"""What the pooling modes cost, and what pruning the last layer buys.

One process, one context, graph-replayed bertx_forward_device on token ids already in
HBM, three configurations of the same batch:

    mean           the default (masked mean pool + L2)
    cls_unpruned   [CLS] pooling, full last layer (bertx_set_cls_pruning 0)
    cls_pruned     [CLS] pooling, last layer on the sentences' first rows only

at c3 (bge-base-en-v1.5 q4_0, 64 sentences of 512 tokens) and b1 (one sentence of 32
tokens).  Per shape: warm-up replays of every configuration (a shape is captured on its
second use), then `--rounds` rounds, each timing one window of `--iters` replays per
configuration between two device events, the configurations taken in turn so that
clock drift falls on all three alike.  Reported: the median window per replay with its
min-max spread, the launches per forward, and (one profiled pass, events around every
launch, no graph) the per-class times of bertx_kernel_stats.

The last layer's launches on their own: the same passes on a one-layer model of the same
dimensions ("layers": 1 in the record), whose only layer is the last one, so its
per-class times are those of the pruned (or full) last-layer launches.
One JSON line per (model, shape, configuration) into --out.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))

import bertpy  # noqa: E402

SHAPES = {"c3": (64, 512), "b1": (1, 32)}
CONFIGS = {"mean": (0, 1), "cls_unpruned": (1, 0), "cls_pruned": (1, 1)}


def measure(torch, m, hp, shape, rounds, iters, stream, extra):
    L = m.lib
    dev = torch.device("cuda", 0)
    sp = ctypes.c_void_p(stream.cuda_stream)
    n, ln = SHAPES[shape]
    ids_list = bertpy.synthetic_ids(n, ln, hp["n_vocab"], seed=7)
    T = n * ln
    ids = torch.from_numpy(np.concatenate(ids_list).astype(np.int32)).to(dev)
    cu = torch.from_numpy((np.arange(n + 1) * ln).astype(np.int32)).to(dev)
    out = torch.empty((n, m.n_embd), dtype=torch.float32, device=dev)
    assert L.bertx_reserve(m.ctx, 0, T, n) == 0
    args = (m.ctx, 0, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(cu.data_ptr()), n, ln, T,
            ctypes.c_void_p(out.data_ptr()), sp)

    def configure(name):
        pool, prune = CONFIGS[name]
        assert L.bertx_set_pooling(m.ctx, pool) == 0
        assert L.bertx_set_cls_pruning(m.ctx, prune) == 0

    def step():
        rc = L.bertx_forward_device(*args)
        if rc != 0:
            raise RuntimeError("bertx_forward_device failed: %d" % rc)

    res = {}
    for name in CONFIGS:
        configure(name)
        for _ in range(4):
            step()
        torch.cuda.synchronize(dev)
        res[name] = out.cpu().numpy().copy()
    times = {name: [] for name in CONFIGS}
    for _ in range(rounds):
        for name in CONFIGS:
            configure(name)
            step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(iters):
                step()
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    recs = []
    for name in CONFIGS:
        configure(name)
        L.bertx_set_profiling(m.ctx, 1)
        step()
        torch.cuda.synchronize(dev)
        L.bertx_reset_stats(m.ctx)
        k = max(2, iters // 4)
        for _ in range(k):
            step()
        torch.cuda.synchronize(dev)
        st = m.kernel_stats()
        L.bertx_set_profiling(m.ctx, 0)
        t = np.array(times[name])
        cosv = np.sum(res["cls_pruned"].astype(np.float64) * res["cls_unpruned"], axis=1)
        rec = dict(extra, shape=shape, sentences=n, len=ln, config=name,
                   ms_median=round(float(np.median(t)), 5), ms_min=round(float(t.min()), 5),
                   ms_max=round(float(t.max()), 5), rounds=rounds, iters=iters,
                   launches_per_forward=sum(s["launches"] for s in st) / k,
                   class_us_per_forward={s["name"]: round(s["ms"] * 1e3 / k, 2) for s in st if s["launches"]},
                   class_launches_per_forward={s["name"]: s["launches"] / k for s in st if s["launches"]},
                   class_work_per_forward={s["name"]: s["work"] / k for s in st if s["launches"]},
                   max_1_minus_cos_pruned_vs_unpruned=float((1.0 - cosv).max()))
        recs.append(rec)
    configure("mean")
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="bge-base-en-v1.5")
    ap.add_argument("--ftype", default="q4_0")
    ap.add_argument("--shapes", default="c3,b1")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", default="c3=20,b1=300")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_cost.jsonl"))
    ap.add_argument("--model-dir", default=os.path.join(ROOT, "build", "models"))
    a = ap.parse_args()
    import torch
    os.makedirs(a.model_dir, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    os.environ.setdefault("BERT_DEVICES", "0")
    os.environ.pop("BERT_POOL", None)
    iters = {k: int(v) for k, v in (x.split("=") for x in a.iters.split(","))}
    hp = bertpy.ARCHS[a.arch]
    stream = torch.cuda.Stream(torch.device("cuda", 0))   # a non-default stream: the library captures the forward
    torch.cuda.set_stream(stream)
    with open(a.out, "a") as f:
        for layers in (hp["n_layer"], 1):
            hpl = dict(hp, n_layer=layers)
            path = os.path.join(a.model_dir, f"{a.arch}-{a.ftype}-{layers}l.bin")
            if not os.path.exists(path):
                bertpy.synthetic_model(path, hpl, a.ftype, seed=1234)
            m = bertpy.BertModel(path)
            for shape in a.shapes.split(","):
                extra = {"arch": a.arch, "ftype": a.ftype, "layers": layers}
                for rec in measure(torch, m, hpl, shape, a.rounds, iters[shape], stream, extra):
                    f.write(json.dumps(rec) + "\n")
                    print(json.dumps(rec), flush=True)
            del m


if __name__ == "__main__":
    main()
