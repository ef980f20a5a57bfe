#!/usr/bin/env python3
"""What scoring costs next to embedding.

One process, one context per model, graph-replayed bertx_forward_device_ex on token ids
and token types already in HBM, three configurations of the same batch:

    pooled_cls_pruned   POOLED under [CLS] pooling with the pruned last layer: the code
                        that existed before the head, the baseline of the comparison
    logits_pruned       LOGITS, last layer on the sentences' first rows only
    logits_unpruned     LOGITS, full last layer (bertx_set_cls_pruning 0)

on bge-base-en-v1.5 dims in q4_0 and all-MiniLM-L6-v2 dims in f16 (d 384, dh 32: the
shape of the common MiniLM rerankers), each with a synthetic one-label head, at c3 (64
pairs of 512 tokens) and b1 (one pair of 32 tokens).  Per shape: warm-up replays of every
configuration (a shape is captured on its second use), then `--rounds` rounds, each
timing one window of `--iters` replays per configuration between two device events, the
configurations taken in turn so that clock drift falls on all three alike.  Reported:
the median window per replay with its min-max spread and (one profiled pass, events
around every launch, no graph) the per-class times of bertx_kernel_stats: the output
stage's class, pool_l2, holds the head's launches (gather, pooler, classifier) under
LOGITS and the [CLS] pool under POOLED.  One JSON line per (model, shape, configuration)
into --out.
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
# name: (out kind, pruning)
CONFIGS = {"pooled_cls_pruned": (0, 1), "logits_pruned": (2, 1), "logits_unpruned": (2, 0)}
MODELS = [("bge-base-en-v1.5", "q4_0"), ("all-MiniLM-L6-v2", "f16")]
GEMMS = ("gemm_qkv", "gemm_attn_out", "gemm_ffn_up", "gemm_ffn_down")


def head_model(path, arch, ftype, seed=1234):
    """A synthetic model of `arch` with a one-label head drawn from N(0, 1/d)."""
    hp = bertpy.ARCHS[arch]
    d = hp["n_embd"]
    rng = np.random.default_rng(seed + 1)
    tensors = bertpy.synthetic_tensors(hp, seed)
    s = np.float32(1.0 / np.sqrt(d))
    tensors["pooler.dense.weight"] = rng.standard_normal((d, d), dtype=np.float32) * s
    tensors["pooler.dense.bias"] = rng.standard_normal(d, dtype=np.float32) * np.float32(0.1)
    tensors["classifier.weight"] = rng.standard_normal((1, d), dtype=np.float32) * s
    tensors["classifier.bias"] = rng.standard_normal(1, dtype=np.float32) * np.float32(0.1)
    vocab = bertpy.synthetic_vocab(hp["n_vocab"])
    if ftype in ("f32", "f16"):
        bertpy.write_model(path, hp, vocab, tensors, bertpy.FTYPE[ftype], head=True)
        return path
    tmp = path + ".f16.tmp"
    bertpy.write_model(tmp, hp, vocab, tensors, 1, head=True)
    rc = bertpy.load_lib().bertx_quantize_file(tmp.encode(), path.encode(), bertpy.FTYPE[ftype])
    os.remove(tmp)
    if rc != 0:
        raise RuntimeError("quantize failed")
    return path


def measure(torch, m, hp, shape, rounds, iters, stream, extra):
    L = m.lib
    dev = torch.device("cuda", 0)
    sp = ctypes.c_void_p(stream.cuda_stream)
    n, ln = SHAPES[shape]
    T = n * ln
    ids = torch.from_numpy(np.concatenate(bertpy.synthetic_ids(n, ln, hp["n_vocab"], seed=7)).astype(np.int32)).to(dev)
    ty = (np.arange(ln) >= (2 * ln) // 5).astype(np.int32)          # A: the first two fifths of a pair
    types = torch.from_numpy(np.tile(ty, n)).to(dev)
    cu = torch.from_numpy((np.arange(n + 1) * ln).astype(np.int32)).to(dev)
    out = torch.empty((n, m.n_embd), dtype=torch.float32, device=dev)
    assert L.bertx_reserve(m.ctx, 0, T, n) == 0
    assert L.bertx_set_pooling(m.ctx, 1) == 0

    def step(name):
        kind, prune = CONFIGS[name]
        L.bertx_set_cls_pruning(m.ctx, prune)
        rc = L.bertx_forward_device_ex(m.ctx, 0, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(types.data_ptr()),
                                       ctypes.c_void_p(cu.data_ptr()), n, ln, T, kind, ctypes.c_void_p(out.data_ptr()),
                                       sp)
        if rc != 0:
            raise RuntimeError("bertx_forward_device_ex failed: %d" % rc)

    for name in CONFIGS:
        for _ in range(4):
            step(name)
        torch.cuda.synchronize(dev)
    times = {name: [] for name in CONFIGS}
    for _ in range(rounds):
        for name in CONFIGS:
            step(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(iters):
                step(name)
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    recs = []
    for name in CONFIGS:
        L.bertx_set_profiling(m.ctx, 1)
        step(name)
        torch.cuda.synchronize(dev)
        L.bertx_reset_stats(m.ctx)
        k = max(2, iters // 4)
        for _ in range(k):
            step(name)
        torch.cuda.synchronize(dev)
        st = m.kernel_stats()
        L.bertx_set_profiling(m.ctx, 0)
        t = np.array(times[name])
        per_launch = {s["name"]: s["ms"] * 1e3 / s["launches"] for s in st if s["launches"]}
        recs.append(dict(extra, shape=shape, pairs=n, len=ln, config=name,
                         ms_median=round(float(np.median(t)), 5), ms_min=round(float(t.min()), 5),
                         ms_max=round(float(t.max()), 5), rounds=rounds, iters=iters,
                         launches_per_forward=sum(s["launches"] for s in st) / k,
                         output_stage_us=round(next(s["ms"] for s in st if s["name"] == "pool_l2") * 1e3 / k, 2),
                         output_stage_launches=next(s["launches"] for s in st if s["name"] == "pool_l2") / k,
                         smallest_gemm_launch_us=round(min(per_launch[g] for g in GEMMS if g in per_launch), 2),
                         class_us_per_forward={s["name"]: round(s["ms"] * 1e3 / k, 2) for s in st if s["launches"]}))
    L.bertx_set_cls_pruning(m.ctx, 1)
    L.bertx_set_pooling(m.ctx, 0)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,b1")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", default="c3=20,b1=300")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_cost.jsonl"))
    ap.add_argument("--model-dir", default=os.path.join(ROOT, "build", "models"))
    a = ap.parse_args()
    import torch
    os.makedirs(a.model_dir, exist_ok=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    os.environ.setdefault("BERT_DEVICES", "0")
    os.environ.pop("BERT_POOL", None)
    iters = {k: int(v) for k, v in (x.split("=") for x in a.iters.split(","))}
    stream = torch.cuda.Stream(torch.device("cuda", 0))   # a non-default stream: the library captures the forward
    torch.cuda.set_stream(stream)
    with open(a.out, "a") as f:
        for arch, ftype in MODELS:
            path = os.path.join(a.model_dir, f"{arch}-{ftype}-head.bin")
            if not os.path.exists(path):
                head_model(path, arch, ftype)
            m = bertpy.BertModel(path)
            assert m.n_labels == 1
            for shape in a.shapes.split(","):
                extra = {"arch": arch, "ftype": ftype}
                for rec in measure(torch, m, bertpy.ARCHS[arch], shape, a.rounds, iters[shape], stream, extra):
                    f.write(json.dumps(rec) + "\n")
                    print(json.dumps(rec), flush=True)
            del m


if __name__ == "__main__":
    main()
