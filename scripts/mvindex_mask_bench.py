#!/usr/bin/env python3
"""What document masks cost the token store's scans, in the manner of
search_mask_bench.py: several libraries in one session by the same code, medians with their
min-max spread.

Per library (--libs label=path[,label=path ...]; a fresh child process each, through ctypes
alone, so that a library from before the masks existed is measured by the same code), per
storage kind and B, at the shape DESIGN.md 9g-3 / 9g-4 tabulate (width 128, ragged documents,
Lq 32, k 10): R rounds, each one call of the library's own bench entry, which builds the store,
warms up with three calls and returns the mean of --iters calls between two device events:
  plain             bertx_bench_maxsim_search: the untouched store, no filter (the unmasked kernels);
and, where the library has bertx_bench_maxsim_masked, its patterns
  ones shared       one all-ones filter for every query;
  ones per query    B all-ones filters;
  random 1/16       one shared filter that admits a hashed sixteenth of the documents;
  range 1/16        one shared filter that admits the first sixteenth;
  deleted 1/16      no filter, a hashed sixteenth of the documents removed.
--centroids C > 0 measures the candidate scan with its selection instead (avg_us[1] of the
pruned entry, C hash-chosen stored rows as centroids) under the same patterns.  The rounds go
pattern by pattern in turn, so that clock drift falls on all alike.  One JSON line per (library, what, kind, B, pattern) is appended to --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGE = {"f16": 0, "int8": 1}
PATTERNS = ["plain", "ones shared", "ones per query", "random 1/16", "range 1/16", "deleted 1/16"]


def summary(t):
    return {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def child(args):
    os.environ.setdefault("BERT_DEVICES", "0")
    L = ctypes.CDLL(args.lib)
    i32, fp = ctypes.c_int32, ctypes.POINTER(ctypes.c_float)
    L.bertx_bench_maxsim_search.restype = i32
    L.bertx_bench_maxsim_search.argtypes = [i32] * 8 + [fp]
    L.bertx_bench_maxsim_pruned.restype = i32
    L.bertx_bench_maxsim_pruned.argtypes = [i32] * 10 + [fp]
    masked = hasattr(L, "bertx_bench_maxsim_masked")
    if masked:
        L.bertx_bench_maxsim_masked.restype = i32
        L.bertx_bench_maxsim_masked.argtypes = [i32] * 11 + [fp]
    w, n, Lq, k, C, n_cand = args.width, args.docs, args.lq, args.k, args.centroids, args.n_cand
    us = (ctypes.c_float * 3)()

    def run(kind, B, pattern, cents):
        st = STORAGE[kind]
        if pattern == 0 and not cents:
            rc = L.bertx_bench_maxsim_search(w, n, 0, Lq, B, k, st, args.iters, us)
        elif pattern == 0:
            rc = L.bertx_bench_maxsim_pruned(w, n, 0, cents, Lq, B, k, n_cand, st, args.iters, us)
        else:
            rc = L.bertx_bench_maxsim_masked(w, n, 0, cents, Lq, B, k, n_cand, st, pattern, args.iters, us)
        assert rc == 0, (kind, B, pattern, cents, rc)
        return us[1] if cents else us[0]

    with open(args.out, "a") as f:
        for what, cents in ((("candidate scan", C),) if C else (("search", 0),)):   # --centroids: the candidate scan alone
            for kind in args.storage.split(","):
                for B in [int(x) for x in args.batches.split(",")]:
                    pats = range(len(PATTERNS)) if masked else [0]
                    times = {p: [] for p in pats}
                    for _ in range(args.rounds):
                        for p in pats:
                            times[p].append(run(kind, B, p, cents))
                    for p in pats:
                        rec = {"lib": args.label, "what": what, "storage": kind, "B": B, "pattern": PATTERNS[p], "w": w,
                               "n_docs": n, "docs": "ragged", "Lq": Lq, "k": k, "rounds": args.rounds, "iters": args.iters}
                        if cents:
                            rec.update({"C": cents, "n_cand": n_cand})
                        rec.update(summary(times[p]))
                        line = json.dumps(rec)
                        print(line, flush=True)
                        f.write(line + "\n")
                        f.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="this build=" + os.path.join(ROOT, "build", "libbert.so"),
                    help="label=path[,label=path ...]: measured one after the other, each in a child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvindex_mask_bench.jsonl"))
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--docs", type=int, default=32768)
    ap.add_argument("--lq", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", default="1,4,32")
    ap.add_argument("--storage", default="f16,int8")
    ap.add_argument("--centroids", type=int, default=0)
    ap.add_argument("--n-cand", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--label", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.lib:
        return child(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for item in args.libs.split(","):
        label, path = item.split("=", 1)
        cmd = [sys.executable, os.path.abspath(__file__), "--lib", path, "--label", label, "--out", args.out]
        for name in ("width", "docs", "lq", "k", "batches", "storage", "centroids", "n_cand", "rounds", "iters"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(args, name))]
        rc = subprocess.run(cmd).returncode
        if rc != 0:   # a library that failed is not followed by another on the same device
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
