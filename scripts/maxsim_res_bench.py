#!/usr/bin/env python3
"""The residual-coded token stores against the f16 and int8 stores.  The
method is maxsim_pruned_bench.py's: one process, stores of 9g's shape (100,000 documents of
128 tokens, width 128) filled with the same rows, device events, warm-ups, then rounds that
time the contenders in turn so that clock drift falls on all alike.

Per centroid count C the centroids are C rows of the f16 store chosen by a multiplicative
hash, the buckets are trained on the f16 store (bertx_mvindex_train_residual_buckets), and
the res2 and res4 stores are built with both.  Timed, Lq 32:
  (a) bertx_mvindex_score_device over n_cand candidates spread over the store, per kind;
  (b) bertx_mvindex_search_pruned_device, one query, the 10 best of 128 candidates, per kind.
Reported: medians with min-max, each kind over f16, the bytes per token slot of each kind.
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
from maxsim_bench import timed  # noqa: E402
from maxsim_search_bench import spread  # noqa: E402

DOC_LEN = 128
KINDS = ("res2", "res4", "f16", "int8")


def slot_bytes(kind, w):
    return {"f16": 2 * w + 2, "int8": w + 4 + 2, "res2": w // 4 + 6, "res4": w // 2 + 6}[kind]   # with the 2-byte code


def fill(torch, lib, stores, stream, w, n_docs, seed):
    """The same unit rows into every store, maxsim_bench.build()'s way."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    sp = ctypes.c_void_p(stream.cuda_stream)
    chunk = max(1, (1 << 28) // (DOC_LEN * w * 4))
    with torch.cuda.stream(stream):
        for i in range(0, n_docs, chunk):
            j = min(n_docs, i + chunk)
            x = torch.randn(j - i, DOC_LEN, w, generator=g, device="cuda", dtype=torch.float32)
            rows = (x / x.norm(dim=2, keepdim=True)).reshape(-1, w).contiguous()
            stream.synchronize()
            lens = np.full(j - i, DOC_LEN, np.int32)
            for mv in stores:
                assert lib.bertx_mvindex_add_device(mv.mv, rows.data_ptr(), lens.ctypes.data, j - i, sp) == i
            stream.synchronize()


def contest(torch, stream, runs, rounds, warm):
    """{name: [us]}: the contenders in turn, `rounds` times after `warm` untimed turns."""
    with torch.cuda.stream(stream):
        for _ in range(warm):
            for fn in runs.values():
                fn()
        stream.synchronize()
        t = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                t[k].append(timed(torch, stream, fn))
        stream.synchronize()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_res_bench.jsonl"))
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--centroids", default="256,4096")
    ap.add_argument("--cands", default="128,4096")
    ap.add_argument("--lq", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "maxsim_res_bench.py measures on a GPU"
    os.environ.setdefault("BERT_DEVICES", "0")
    lib = bertpy.load_lib()
    stream = torch.cuda.Stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    model = bertpy.BertModel(os.path.join(ROOT, "tests", "golden", "tiny64", "ggml-model-f16.bin"))
    w, n_docs, Lq = args.width, args.docs, args.lq
    slots = n_docs * DOC_LEN
    seed = 17 * w + len("uniform")
    mvs = {k: bertpy.BertTokenIndex(model, n_docs, slots, width=w, storage=k) for k in ("f16", "int8")}
    fill(torch, lib, list(mvs.values()), stream, w, n_docs, seed)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            rec.update({"w": w, "n_docs": n_docs, "doc_len": DOC_LEN, "Lq": Lq, "rounds": args.rounds,
                        "slot_bytes": {k: slot_bytes(k, w) for k in KINDS}, "device": torch.cuda.get_device_name(0)})
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for C in [int(x) for x in args.centroids.split(",")]:
            cent = np.stack([mvs["f16"].doc(int((c * 2654435761 + 777) % n_docs))[c % 16] for c in range(C)])
            mvs["f16"].set_centroids(cent)
            mvs["int8"].set_centroids(cent)
            for kind, nb in (("res2", 2), ("res4", 4)):
                mvs.pop(kind, None)
                torch.cuda.empty_cache()
                mv = bertpy.BertTokenIndex(model, n_docs, slots, width=w, storage=kind)
                mv.set_centroids(cent)
                mv.set_residual_buckets(*mvs["f16"].train_residual_buckets(nb))
                fill(torch, lib, [mv], stream, w, n_docs, seed)
                mvs[kind] = mv
            g = torch.Generator(device="cuda")
            g.manual_seed(C)
            q = torch.randn(Lq, w, generator=g, device="cuda", dtype=torch.float32)
            for n_cand in [int(x) for x in args.cands.split(",")]:
                ids = torch.randint(0, n_docs, (n_cand,), generator=g, device="cuda", dtype=torch.int32)
                outs = {k: torch.empty(n_cand, device="cuda", dtype=torch.float32) for k in KINDS}

                def scorer(k):
                    def run():
                        rc = lib.bertx_mvindex_score_device(mvs[k].mv, q.data_ptr(), Lq, ids.data_ptr(), n_cand,
                                                            outs[k].data_ptr(), sp)
                        assert rc == 0, rc
                    return run
                t = contest(torch, stream, {k: scorer(k) for k in KINDS}, args.rounds, args.warmup)
                med = {k: statistics.median(v) for k, v in t.items()}
                emit({"what": "scorer", "C": C, "n_cand": n_cand, **{k: spread(v) for k, v in t.items()},
                      "over_f16": {k: round(med[k] / med["f16"], 2) for k in KINDS},
                      "mean_abs_score_diff_vs_f16": {k: float((outs[k] - outs["f16"]).abs().mean().item()) for k in KINDS}})
            k_best, n_cand = 10, 128
            sc = {k: torch.empty(1, k_best, device="cuda", dtype=torch.float32) for k in KINDS}
            oi = {k: torch.empty(1, k_best, device="cuda", dtype=torch.int32) for k in KINDS}

            def pruned(k):
                def run():
                    rc = lib.bertx_mvindex_search_pruned_device(mvs[k].mv, q.data_ptr(), 1, Lq, k_best, n_cand,
                                                                sc[k].data_ptr(), oi[k].data_ptr(), sp)
                    assert rc == 0, rc
                return run
            t = contest(torch, stream, {k: pruned(k) for k in KINDS}, args.rounds, args.warmup)
            med = {k: statistics.median(v) for k, v in t.items()}
            f16_ids = set(oi["f16"].cpu().numpy()[0].tolist())
            emit({"what": "search_pruned", "C": C, "B": 1, "k": k_best, "n_cand": n_cand, **{k: spread(v) for k, v in t.items()},
                  "over_f16": {k: round(med[k] / med["f16"], 2) for k in KINDS},
                  "f16_topk_found": {k: len(f16_ids & set(oi[k].cpu().numpy()[0].tolist())) / k_best for k in KINDS}})


if __name__ == "__main__":
    main()
