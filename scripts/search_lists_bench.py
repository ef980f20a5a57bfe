#!/usr/bin/env python3
"""Lists and the probed search of the embedding index beside the flat search.

One bertx_bench_search_lists call per point (N, storage, C, B): one synthetic index with planted
cluster structure, the lists set from the planted centroids, then per round `iters` flat searches
and `iters` probed searches for every n_probe, alternating, between device events after 3 warm-up
calls of every form.  Every time is the median of the rounds with its min-max spread.  Also per
point: the host time of bertx_index_set_lists per million rows, the image's bytes, and recall@k of
the probed ids against the flat ones on this synthetic set.  d 768, k 10.  One JSON line per point
into --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))

import bertpy  # noqa: E402

D, K = 768, 10


def spread(t):
    return {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 8400000])
    ap.add_argument("--storage", nargs="+", default=["f16", "int8"])
    ap.add_argument("--lists", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_lists_bench.jsonl"))
    a = ap.parse_args()
    lib = bertpy.load_lib()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    n_np = len(a.probes)
    probes = (ctypes.c_int32 * n_np)(*a.probes)
    with open(a.out, "a") as f:
        for N, kind, C, B in [(N, s, C, B) for N in a.rows for s in a.storage for C in a.lists for B in a.batches]:
            iters = 20 if B == 1 else 5
            flat = (ctypes.c_float * a.rounds)()
            probed = (ctypes.c_float * (n_np * a.rounds))()
            recall = (ctypes.c_float * n_np)()
            build_ms, image = ctypes.c_double(), ctypes.c_int64()
            rc = lib.bertx_bench_search_lists(D, N, B, K, bertpy.BertIndex.STORAGE[kind], C, probes, n_np, a.rounds, iters, flat,
                                              probed, recall, ctypes.byref(build_ms), ctypes.byref(image))
            assert rc == 0, rc
            rec = {"d": D, "N": N, "storage": kind, "C": C, "B": B, "k": K, "rounds": a.rounds, "iters": iters,
                   "flat_us": spread(list(flat)), "build_ms_per_million_rows": round(build_ms.value * 1e6 / N, 1),
                   "image_bytes": image.value, "flat_bytes": N * D * (1 if kind == "int8" else 2), "synthetic": True}
            for i, n_probe in enumerate(a.probes):
                t = list(probed[i * a.rounds:(i + 1) * a.rounds])
                rec["probe%d" % n_probe] = dict(spread(t), recall=round(recall[i], 4),
                                                flat_over_probed=round(rec["flat_us"]["median"] / statistics.median(t), 2),
                                                slowest_probed_beats_fastest_flat=max(t) < min(flat))
            rec["time"] = time.strftime("%Y-%m-%dT%H:%M:%S")
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
