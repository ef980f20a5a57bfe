#!/usr/bin/env python3
"""The full-scan MaxSim top-k search against what the scorer offered for the same job
(DESIGN.md 9g-3).  The method is maxsim_bench.py's: one process, stores past the 256 MiB
Infinity Cache built by its build(), device events, warm-ups, then rounds that time the
contenders in turn so that clock drift falls on all alike.

Per (width, document shape, storage kind) one store; per (B, Lq, k):
  (a) bertx_mvindex_search_device for the B queries: ceil(B / floor(4 / ceil(Lq / 16)))
      passes over the store, each followed by the merge kernel;
  (b) B launches of bertx_mvindex_score_device(ids = NULL), each followed by torch.topk on
      the device: one pass over the store per query.
Reported: the median with its min-max spread; the store's group bytes (what one pass
reads) over the median and its share of the 6.3 TB/s the HBM sustains, and the same per
pass of (a); (b) / (a); at the end of a store, the time per query of the packed points
over the B = 1 point of the same Lq and k.  The scores of (a) are checked against the
sorted scores of (b).  bertx_bench_maxsim_search (the library's own loop on its own rows)
runs once per point as a cross-check unless --no-hook.  One JSON line per point into --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bertpy  # noqa: E402
from maxsim_bench import ROOF, build, timed  # noqa: E402

N_DOCS = {(128, "uniform"): 100000, (768, "uniform"): 16384, (128, "ragged"): 32768, (768, "ragged"): 8192}
POINTS = [(1, 32), (2, 32), (1, 16), (4, 16), (8, 32)]   # (B, Lq)


def spread(t):
    return {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def point(torch, lib, mv, stream, kind, w, shape, n_docs, B, Lq, k, rounds, warm, hook):
    g = torch.Generator(device="cuda")
    g.manual_seed(100 * B + Lq)
    q = torch.randn(B, Lq, w, generator=g, device="cuda", dtype=torch.float32)
    sc = torch.empty(B, k, device="cuda", dtype=torch.float32)
    ids = torch.empty(B, k, device="cuda", dtype=torch.int32)
    full = torch.empty(n_docs, device="cuda", dtype=torch.float32)
    sp = ctypes.c_void_p(stream.cuda_stream)
    best = {}

    def ours():
        rc = lib.bertx_mvindex_search_device(mv.mv, q.data_ptr(), B, Lq, k, sc.data_ptr(), ids.data_ptr(), sp)
        assert rc == 0, rc

    def theirs():
        for b in range(B):
            rc = lib.bertx_mvindex_score_device(mv.mv, q[b].data_ptr(), Lq, None, n_docs, full.data_ptr(), sp)
            assert rc == 0, rc
            best[b] = torch.topk(full, k)

    with torch.cuda.stream(stream):
        for _ in range(warm):
            ours()
            theirs()
        stream.synchronize()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timed(torch, stream, ours))
            tb.append(timed(torch, stream, theirs))
        same = all(torch.equal(sc[b], best[b].values) for b in range(B))
    per_pass = 4 // ((Lq + 15) // 16)
    passes = -(-B // per_pass)
    store_bytes = mv.token_slots * (w * 2 if kind == "f16" else w + 4)
    rec = {"w": w, "docs": shape, "n_docs": n_docs, "storage": kind, "B": B, "Lq": Lq, "k": k, "rounds": rounds,
           "store_MiB": round(store_bytes / 2 ** 20), "roof_us_per_pass": round(store_bytes / ROOF * 1e6, 1),
           "passes": passes, "scores_equal_scorer_topk": bool(same), "search": spread(ta), "score_topk": spread(tb)}
    ma, mb = statistics.median(ta), statistics.median(tb)
    rec["search"]["store_bytes_over_median_roof_share"] = round(store_bytes / (ma * 1e-6) / ROOF, 3)
    rec["search"]["per_pass_roof_share"] = round(passes * store_bytes / (ma * 1e-6) / ROOF, 3)
    rec["score_topk"]["per_pass_roof_share"] = round(B * store_bytes / (mb * 1e-6) / ROOF, 3)
    rec["score_topk_over_search"] = round(mb / ma, 2)
    rec["search_us_per_query"] = round(ma / B, 1)
    if hook:
        us = ctypes.c_float()
        rc = lib.bertx_bench_maxsim_search(w, n_docs, 128 if shape == "uniform" else 0, Lq, B, k,
                                           bertpy.BertTokenIndex.STORAGE[kind], rounds, ctypes.byref(us))
        rec["bench_maxsim_search_avg_us"] = round(us.value, 1) if rc == 0 else None
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_search_bench.jsonl"))
    ap.add_argument("--widths", default="128,768")
    ap.add_argument("--shapes", default="uniform,ragged")
    ap.add_argument("--storage", default="f16,int8")
    ap.add_argument("--ks", default="10,128")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-hook", action="store_true", help="skip bertx_bench_maxsim_search (it builds a store per point)")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "maxsim_search_bench.py measures on a GPU"
    os.environ.setdefault("BERT_DEVICES", "0")
    lib = bertpy.load_lib()
    stream = torch.cuda.Stream()
    model = bertpy.BertModel(os.path.join(ROOT, "tests", "golden", "tiny64", "ggml-model-f16.bin"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        def emit(rec):
            rec["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for w in [int(x) for x in args.widths.split(",")]:
            for shape in args.shapes.split(","):
                n_docs = N_DOCS.get((w, shape), 16384)
                for kind in args.storage.split(","):
                    mvs, _, _, _ = build(torch, lib, model, stream, w, shape, n_docs, 17 * w + len(shape), (kind,), False)
                    per_query = {}
                    for k in [int(x) for x in args.ks.split(",")]:
                        for B, Lq in POINTS:
                            rec = point(torch, lib, mvs[kind], stream, kind, w, shape, n_docs, B, Lq, k, args.rounds,
                                        args.warmup, not args.no_hook)
                            per_query[(B, Lq, k)] = rec["search"]["median_us"] / B
                            emit(rec)
                    # the time per query of a call whose queries share passes, over one query alone
                    ratios = {"B%d_Lq%d_k%d_over_B1" % (B, Lq, k): round(t / per_query[(1, Lq, k)], 3)
                              for (B, Lq, k), t in per_query.items() if B > 1}
                    emit({"w": w, "docs": shape, "storage": kind, "what": "search time per query over the B = 1 point",
                          "ratios": ratios})
                    del mvs
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
