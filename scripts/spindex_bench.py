#!/usr/bin/env python3
"""The sparse index: the selection, the pack and the fused scan.

Every figure is the median of R rounds with its min-max spread; a round is one
bertx_bench_spindex call (3 warm-up launches, then `iters` timed launches between two device
events per stage).  V 30,522, 128 postings per document (512 stored bytes), k 10.

Per point (n_docs, B): the scan's microseconds and its stored bytes per second, beside
bertx_bench_search_ex's f16 scan of the same number of stored bytes in the same process (d 256:
512 bytes per row, the same n_docs rows); the selection's microseconds per row beside the time
of reading the row's V * 4 bytes once at that dense scan's byte rate; the pack and append per row.
One JSON line per point into --out.

--batch-leg measures bertx_bench_spindex_batch instead: per point (n_docs, B) the
query-image kernel, the whole sparse-query search of B queries of --q-len terms and the dense-query
search of the same queries densified, in the same process and round.

--inverted-leg measures bertx_bench_spindex_inverted: per point (n_docs, B, skew) the
build of the inverted image, the inverted search, the sparse-query search and the dense-query search
of the same queries, in the same process and round; skew 1 plants heavy terms in documents and queries.
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

V, DOC_LEN, K, DENSE_D = 30522, 128, 10, 256


def spread(t):
    return {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1 << 20, 1 << 23])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-leg", action="store_true")
    ap.add_argument("--inverted-leg", action="store_true")
    ap.add_argument("--skews", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spindex_bench.jsonl"))
    a = ap.parse_args()
    lib = bertpy.load_lib()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for n_docs, B, skew in [(n, B, s) for n in a.docs for B in a.batches for s in a.skews] if a.inverted_leg else []:
            iters = 20 if B <= 2 else 5
            legs = {"build_us": [], "inverted_us": [], "sparse_query_us": [], "dense_query_us": []}
            us4 = (ctypes.c_float * 4)()
            for _ in range(a.rounds):
                assert lib.bertx_bench_spindex_inverted(V, n_docs, DOC_LEN, B, a.q_len, K, skew, iters, us4) == 0
                for name, us in zip(legs, us4):
                    legs[name].append(us)
            rec = {"leg": "inverted", "V": V, "n_docs": n_docs, "doc_len": DOC_LEN, "B": B, "q_len": a.q_len, "k": K,
                   "skew": skew, "rounds": a.rounds, "iters": iters, **{name: spread(t) for name, t in legs.items()}}
            rec["build_us_per_million_docs"] = round(rec["build_us"]["median"] * 1e6 / n_docs, 1)
            rec["inverted_bytes_added"] = n_docs * DOC_LEN * 4 + -(-n_docs // 16384) * (V + 1) * 4
            rec["slowest_inverted_beats_fastest_dense"] = max(legs["inverted_us"]) < min(legs["dense_query_us"])
            rec["slowest_inverted_beats_fastest_sparse"] = max(legs["inverted_us"]) < min(legs["sparse_query_us"])
            rec["time"] = time.strftime("%Y-%m-%dT%H:%M:%S")
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        if a.inverted_leg:
            return
        for n_docs in a.docs if a.batch_leg else []:
            for B in a.batches:
                iters = 20 if B <= 2 else 5
                image, sparse, dense = [], [], []
                us3 = (ctypes.c_float * 3)()
                for _ in range(a.rounds):
                    assert lib.bertx_bench_spindex_batch(V, n_docs, DOC_LEN, B, a.q_len, K, iters, us3) == 0
                    image.append(us3[0])
                    sparse.append(us3[1])
                    dense.append(us3[2])
                rec = {"leg": "batch", "V": V, "n_docs": n_docs, "doc_len": DOC_LEN, "B": B, "q_len": a.q_len, "k": K,
                       "rounds": a.rounds, "iters": iters, "image_us": spread(image), "sparse_query_us": spread(sparse),
                       "dense_query_us": spread(dense)}
                rec["dense_of_sparse"] = round(rec["dense_query_us"]["median"] / rec["sparse_query_us"]["median"], 2)
                rec["slowest_sparse_beats_fastest_dense"] = max(sparse) < min(dense)
                rec["time"] = time.strftime("%Y-%m-%dT%H:%M:%S")
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
        for n_docs in [] if a.batch_leg else a.docs:
            for B in a.batches:
                iters = 20 if B <= 2 else 3
                sel, pack, scan, dense = [], [], [], []
                us3, us = (ctypes.c_float * 3)(), ctypes.c_float()
                for _ in range(a.rounds):
                    assert lib.bertx_bench_spindex(V, n_docs, DOC_LEN, B, K, iters, us3) == 0
                    sel.append(us3[0])
                    pack.append(us3[1])
                    scan.append(us3[2])
                    assert lib.bertx_bench_search_ex(DENSE_D, n_docs, B, K, 0, iters, ctypes.byref(us)) == 0
                    dense.append(us.value)
                rows = min(1024, n_docs)
                stored = n_docs * DOC_LEN * 4
                rec = {"V": V, "n_docs": n_docs, "doc_len": DOC_LEN, "B": B, "k": K, "rounds": a.rounds, "iters": iters,
                       "stored_bytes": stored, "select_us": spread(sel), "pack_us": spread(pack), "scan_us": spread(scan),
                       "dense_f16_scan_us": spread(dense), "select_rows": rows}
                rec["scan_GBps"] = round(stored / (rec["scan_us"]["median"] * 1e-6) / 1e9, 1)
                rec["dense_GBps"] = round(stored / (rec["dense_f16_scan_us"]["median"] * 1e-6) / 1e9, 1)
                rec["scan_of_dense"] = round(rec["scan_GBps"] / rec["dense_GBps"], 3)
                rec["select_us_per_row"] = round(rec["select_us"]["median"] / rows, 3)
                rec["row_read_once_us"] = round(V * 4 / (rec["dense_GBps"] * 1e9) * 1e6, 3)
                rec["pack_us_per_row"] = round(rec["pack_us"]["median"] / rows, 4)
                rec["time"] = time.strftime("%Y-%m-%dT%H:%M:%S")
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
