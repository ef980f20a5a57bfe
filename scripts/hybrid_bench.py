#!/usr/bin/env python3
"""The hybrid search beside its stages: bertx_bench_hybrid once per (B, fusion) in this
one process, median (min - max) of the repetitions per leg; the lines go to stdout and, with a path
as the first argument, to that file (profiles/hybrid_9i6_bench.txt was made so)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))
import bertpy  # noqa: E402

L = bertpy.load_lib()
LEGS = ["dense search n_cand", "sparse-query search n_cand", "inverted search n_cand", "hybrid (sparse-query stage)",
        "hybrid (inverted stage)", "spindex score_ids n=128", "index score_ids n=128"]
V, d, n_docs, doc_len, q_len, k, n_cand, iters, reps = 30522, 768, 1000000, 128, 32, 10, 64, 20, 5
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
for B in (1, 64):
    for mode, name in ((0, "linear"), (1, "rrf")):
        us = np.zeros((7, reps), np.float32)
        rc = L.bertx_bench_hybrid(V, d, n_docs, doc_len, B, q_len, k, n_cand, mode, iters, reps,
                                  us.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        for leg, row in zip(LEGS, us):
            line = "B %2d %-6s %-28s rc %d  median %8.1f us (min %8.1f - max %8.1f)" % (
                B, name, leg, rc, np.median(row), row.min(), row.max())
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        if rc != 0:
            sys.exit(1)
