#!/usr/bin/env python3
"""The pruned MaxSim search (centroid interaction, then the scorer on the candidates) against
the full scan on the same store.  The method is maxsim_search_bench.py's: one
process, a store past the Infinity Cache built by maxsim_bench.build(), device events, warm-ups,
then rounds that time the two contenders in turn so that clock drift falls on both alike.

Per (width, document shape, storage kind) one store; per centroid count C the centroids are C
stored rows chosen by a multiplicative hash (bertx_mvindex_set_centroids codes the store); per
(B, Lq, k), with n_cand = min(128, 4 k):
  (a) bertx_mvindex_search_pruned_device;
  (b) bertx_mvindex_search_device, the full scan.
Reported: medians with min-max, (b) / (a), how many of the full scan's k best the pruned search
returned (random rows: not a statement about text), and the split of (a) into the table
kernels, the scans with their selections and the rest (scorer and final order) by
bertx_bench_maxsim_pruned, the library's own loop over its own rows (--no-hook skips it).
One JSON line per point into --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bertpy  # noqa: E402
from maxsim_bench import build, timed  # noqa: E402
from maxsim_search_bench import N_DOCS, POINTS, spread  # noqa: E402


def point(torch, lib, mv, stream, kind, w, shape, n_docs, C, B, Lq, k, rounds, warm, hook):
    n_cand = min(128, 4 * k)
    g = torch.Generator(device="cuda")
    g.manual_seed(100 * B + Lq)
    q = torch.randn(B, Lq, w, generator=g, device="cuda", dtype=torch.float32)
    sc = [torch.empty(B, k, device="cuda", dtype=torch.float32) for _ in range(2)]
    ids = [torch.empty(B, k, device="cuda", dtype=torch.int32) for _ in range(2)]
    sp = ctypes.c_void_p(stream.cuda_stream)

    def pruned():
        rc = lib.bertx_mvindex_search_pruned_device(mv.mv, q.data_ptr(), B, Lq, k, n_cand, sc[0].data_ptr(),
                                                    ids[0].data_ptr(), sp)
        assert rc == 0, rc

    def full():
        rc = lib.bertx_mvindex_search_device(mv.mv, q.data_ptr(), B, Lq, k, sc[1].data_ptr(), ids[1].data_ptr(), sp)
        assert rc == 0, rc

    with torch.cuda.stream(stream):
        for _ in range(warm):
            pruned()
            full()
        stream.synchronize()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timed(torch, stream, pruned))
            tb.append(timed(torch, stream, full))
        stream.synchronize()
    pi, fi = ids[0].cpu().numpy(), ids[1].cpu().numpy()
    found = float(np.mean([len(set(pi[b]) & set(fi[b])) / k for b in range(B)]))
    ma, mb = statistics.median(ta), statistics.median(tb)
    rec = {"w": w, "docs": shape, "n_docs": n_docs, "storage": kind, "C": C, "B": B, "Lq": Lq, "k": k, "n_cand": n_cand,
           "rounds": rounds, "pruned": spread(ta), "full_scan": spread(tb), "full_over_pruned": round(mb / ma, 2),
           "pruned_beats_full_scan": bool(ma < mb), "full_scan_topk_found": round(found, 3),
           "table_form": {1: "lds", 2: "global", 3: "both"}.get(lib.bertx_test_approx_ran(1), "none")}
    if hook:
        us = (ctypes.c_float * 3)()
        rc = lib.bertx_bench_maxsim_pruned(w, n_docs, 128 if shape == "uniform" else 0, C, Lq, B, k, n_cand,
                                           bertpy.BertTokenIndex.STORAGE[kind], rounds, us)
        if rc == 0:
            rec["hook_avg_us"] = {"table": round(us[0], 1), "scan_select": round(us[1], 1), "pruned": round(us[2], 1),
                                  "rerank": round(us[2] - us[0] - us[1], 1)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_pruned_bench.jsonl"))
    ap.add_argument("--widths", default="128")
    ap.add_argument("--shapes", default="uniform")
    ap.add_argument("--storage", default="f16,int8")
    ap.add_argument("--centroids", default="256,1024,4096")
    ap.add_argument("--ks", default="10,128")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-hook", action="store_true", help="skip bertx_bench_maxsim_pruned (it builds a store per point)")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "maxsim_pruned_bench.py measures on a GPU"
    os.environ.setdefault("BERT_DEVICES", "0")
    lib = bertpy.load_lib()
    stream = torch.cuda.Stream()
    model = bertpy.BertModel(os.path.join(ROOT, "tests", "golden", "tiny64", "ggml-model-f16.bin"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        for w in [int(x) for x in args.widths.split(",")]:
            for shape in args.shapes.split(","):
                n_docs = N_DOCS.get((w, shape), 16384)
                for kind in args.storage.split(","):
                    mvs, _, _, _ = build(torch, lib, model, stream, w, shape, n_docs, 17 * w + len(shape), (kind,), False)
                    mv = mvs[kind]
                    for C in [int(x) for x in args.centroids.split(",")]:
                        cent = np.stack([mv.doc(int((c * 2654435761 + 777) % n_docs))[c % 16] for c in range(C)])
                        mv.set_centroids(cent)
                        for k in [int(x) for x in args.ks.split(",")]:
                            for B, Lq in POINTS:
                                rec = point(torch, lib, mv, stream, kind, w, shape, n_docs, C, B, Lq, k, args.rounds,
                                            args.warmup, not args.no_hook)
                                rec["device"] = torch.cuda.get_device_name(0)
                                line = json.dumps(rec)
                                print(line, flush=True)
                                f.write(line + "\n")
                                f.flush()
                    del mvs, mv
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
