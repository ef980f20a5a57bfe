#!/usr/bin/env python3
"""Host-visible cost of the token store's text forms on this build against another
libbert.so ("How a text form is assembled"): bge-base dims, q4_0, a seeded
128-dim projection record (project_bench.model_file), a ColBERT store.

  score   one score_text call, a ColBERT query (query_maxlen 32) over 1,000 candidates
  search  one search_texts call of 64 ColBERT queries, k 10
  add     one add_texts call of 4,000 texts of 6 .. 20 words, doc_maxlen 32 (a fresh store)

Each figure is a host clock around one call (every call ends in a stream synchronise).  A
child process per library (BERT_LIB) reports the median of its calls; the two libraries
alternate, --pairs children each, and the line per point carries the median and min-max of
the children's medians.  One JSON line per point into --out.  (The `baseline` lines of
profiles/text_forms_bench.jsonl are bench.py runs of the two libraries alternated in the
same way, as mask_keys_bench.py --baseline alternates them.)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N_DOCS, N_CAND, N_QUERIES, K, QUERY_MAXLEN, DOC_MAXLEN = 4000, 1000, 64, 10, 32, 32


def texts_of(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return [" ".join("w%d" % w for w in rng.integers(0, 20000, int(k))) for k in rng.integers(lo, hi + 1, n)]


def child(model_dir, calls):
    import bertpy
    from project_bench import model_file
    os.environ.setdefault("BERT_DEVICES", "0")
    lib = bertpy.load_lib()
    m = bertpy.BertModel(model_file(model_dir, "bge-base-en-v1.5", 128, lib))
    docs, queries = texts_of(N_DOCS, 6, 20, 1), texts_of(N_QUERIES, 3, 8, 2)
    cand = np.random.default_rng(3).integers(0, N_DOCS, N_CAND).astype(np.int32)

    def timed(fn, n):
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t[2:])                         # the first two calls warm up

    def add():
        ix = bertpy.BertTokenIndex(m, N_DOCS, N_DOCS * DOC_MAXLEN, width=m.proj_width)
        t0 = time.perf_counter()
        assert ix.add_texts(docs, colbert=DOC_MAXLEN) == 0
        return ix, (time.perf_counter() - t0) * 1e3

    adds = [add()[1] for _ in range(2 + max(3, calls // 4))]
    ix, _ = add()
    out = {"add_ms": statistics.median(adds[2:]),
           "score_ms": timed(lambda: ix.score_text(queries[0], cand, colbert=QUERY_MAXLEN), 2 + calls),
           "search_ms": timed(lambda: ix.search_texts(queries, K, colbert=QUERY_MAXLEN), 2 + calls)}
    print(json.dumps(out), flush=True)


def spread(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", metavar="PARENT_LIB")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--model-dir", default=os.path.join(ROOT, "build", "models"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_forms_bench.jsonl"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.model_dir, args.calls)
    assert args.baseline, "--baseline PARENT_LIB"
    runs = {"this": [], "parent": []}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--model-dir", args.model_dir]
    for _ in range(args.pairs):
        for label in ("this", "parent"):
            env = dict(os.environ)
            env.pop("BERT_LIB", None)
            if label == "parent":
                env["BERT_LIB"] = os.path.abspath(args.baseline)
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[label].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for point, what in (("score_ms", "score_text, ColBERT query, %d candidates" % N_CAND),
                            ("search_ms", "search_texts, %d ColBERT queries, k %d" % (N_QUERIES, K)),
                            ("add_ms", "add_texts, %d texts, doc_maxlen %d" % (N_DOCS, DOC_MAXLEN))):
            rec = {"part": point, "workload": what, "pairs": args.pairs, "calls": args.calls,
                   "this": spread([r[point] for r in runs["this"]]), "parent": spread([r[point] for r in runs["parent"]]),
                   "runs_this": [round(r[point], 3) for r in runs["this"]],
                   "runs_parent": [round(r[point], 3) for r in runs["parent"]]}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
