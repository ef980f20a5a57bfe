#!/usr/bin/env python3
"""The ColBERT projector and the indexing path it serves.

One process per library build (BERT_LIB selects another build, e.g. the parent commit's,
for the two comparison parts).  Every figure is the median of R rounds after warm-up
rounds, with its min-max spread, from device events or the library's own per-kernel
device timing (bertx_kernel_stats); wall times end in a device synchronise.

--kernel   bertx_bench_project (the projector alone on random operands, one launch per
           round) at d 768 / dim 128 and d 384 / dim 96, T 2,048 and 131,072: microseconds,
           the bytes it moves, T (2 d + 8 + 4 width), and their share of 6.3 TB/s.
--tokens   the output-stage class (pool_l2) of a BERTX_OUT_TOKENS forward at the same d
           and T (sentences of 128 tokens): the kernel that reads the same z and writes
           4 d instead of 4 width bytes per row.  With a build that has the projector,
           also the class time of a BERTX_OUT_PROJ forward of the same batch.
--index    4,096 texts of about 128 tokens on bge-base dims q4_0 with a seeded 128-dim
           record: bertx_mvindex_add_texts into a width-768 store and (a build that has
           it) bertx_mvindex_add_texts_colbert into a width-128 store: wall time, the
           output-stage class time of a profiled repeat, store bytes per document.
One JSON line per point into --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))

import bertpy  # noqa: E402

ROOF = 6.3e12   # achievable HBM bytes/s
POINTS = [("bge-base-en-v1.5", 768, 128), ("all-MiniLM-L6-v2", 384, 96)]
TS = [2048, 131072]


def spread(t):
    return {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}


def kernel_part(lib, rounds, emit):
    for _, d, dim in POINTS:
        width = (dim + 63) // 64 * 64
        for T in TS:
            us = ctypes.c_float()
            t = []
            for _ in range(rounds):          # each call: 3 warm-up launches, then one timed launch
                rc = lib.bertx_bench_project(d, dim, T, 1, ctypes.byref(us))
                assert rc == 0, rc
                t.append(us.value)
            nbytes = T * (2 * d + 8 + 4 * width)
            rec = {"part": "kernel", "d": d, "dim": dim, "width": width, "T": T, "rounds": rounds, "us": spread(t),
                   "bytes": nbytes}
            rec["TBps"] = round(nbytes / (rec["us"]["median"] * 1e-6) / 1e12, 3)
            rec["roof_share"] = round(nbytes / (rec["us"]["median"] * 1e-6) / ROOF, 3)
            emit(rec)


def model_file(model_dir, arch, dim, lib, vocab=None):
    """arch in q4_0 with a seeded dim-row projection record (quantized with the rest)."""
    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, "%s-q4_0-proj%d%s.bin" % (arch, dim, "-text" if vocab else ""))
    if not os.path.exists(path):
        f16 = path + ".f16.tmp"
        bertpy.synthetic_model(f16 + ".plain", arch, "f16", vocab=vocab)
        d = bertpy.ARCHS[arch]["n_embd"]
        W = (np.random.default_rng(9).standard_normal((dim, d)) / np.sqrt(d)).astype(np.float32)
        bertpy.append_projection(f16 + ".plain", f16, W)
        os.remove(f16 + ".plain")
        assert lib.bertx_quantize_file(f16.encode(), path.encode(), bertpy.FTYPE["q4_0"]) == 0
        os.remove(f16)
    return path


def class_ms(m, name="pool_l2"):
    for row in m.kernel_stats():
        if row["name"] == name:
            return row["ms"], row["launches"]
    raise KeyError(name)


def tokens_part(torch, lib, model_dir, rounds, warm, has_proj, emit):
    dev = torch.device("cuda", 0)
    for arch, d, dim in POINTS:
        path = model_file(model_dir, arch, dim, lib)
        if not has_proj:   # an older build does not load the record: the same file without it
            import struct
            plain = path[:-4] + "-norecord.bin"
            if not os.path.exists(plain):
                data = open(path, "rb").read()
                key = struct.pack("<3i", 2, len(b"linear.weight"), bertpy.FTYPE["q4_0"])
                at = data.rfind(key)
                assert at > 0 and data[at + 20:at + 33] == b"linear.weight"
                open(plain, "wb").write(data[:at])
            path = plain
        m = bertpy.BertModel(path)
        hp = bertpy.ARCHS[arch]
        for T in TS:
            n, ln = T // 128, 128
            ids = torch.from_numpy(np.concatenate(bertpy.synthetic_ids(n, ln, hp["n_vocab"], seed=7)).astype(np.int32)).to(dev)
            cu = torch.from_numpy((np.arange(n + 1) * ln).astype(np.int32)).to(dev)
            out = torch.empty((T, d), dtype=torch.float32, device=dev)
            assert lib.bertx_reserve(m.ctx, 0, T, n) == 0
            for kind, label in ((1, "tokens"), (3, "proj")):
                if kind == 3 and not has_proj:
                    continue
                lib.bertx_set_profiling(m.ctx, 1)
                t = []
                for r in range(warm + rounds):
                    lib.bertx_reset_stats(m.ctx)
                    rc = lib.bertx_forward_device_ex(m.ctx, 0, ctypes.c_void_p(ids.data_ptr()), None,
                                                     ctypes.c_void_p(cu.data_ptr()), n, ln, T, kind,
                                                     ctypes.c_void_p(out.data_ptr()), None)
                    assert rc == 0, rc
                    torch.cuda.synchronize()
                    ms, launches = class_ms(m)
                    assert launches == 1, launches
                    if r >= warm:
                        t.append(ms * 1e3)
                lib.bertx_set_profiling(m.ctx, 0)
                emit({"part": "forward_output_stage", "output": label, "arch": arch, "d": d, "dim": dim, "T": T,
                      "rounds": rounds, "pool_l2_us": spread(t)})
            del ids, cu, out
        del m
        torch.cuda.empty_cache()


def index_part(torch, lib, model_dir, has_proj, emit):
    arch, dim, n = "bge-base-en-v1.5", 128, 4096
    vocab = bertpy.bert_like_vocab(bertpy.ARCHS[arch]["n_vocab"])
    path = model_file(model_dir, arch, dim, lib, vocab=vocab)
    texts = bertpy.bert_like_texts(vocab, n, 69, seed=3)
    if not has_proj:
        raise SystemExit("--index needs a build that loads the projection record; for the parent's _add_texts use "
                         "--index-plain")
    m = bertpy.BertModel(path)
    lens = [m.tokenize(t)[1] for t in texts[:256]]
    for label, width, colbert in (("add_texts", 768, None), ("add_texts_colbert", m.proj_width, 180)):
        walls, cls = [], []
        for rep in range(4):                      # 0: warm-up; 1, 2: wall; 3: profiled
            mv = bertpy.BertTokenIndex(m, n, n * 192, width=width)
            lib.bertx_set_profiling(m.ctx, 1 if rep == 3 else 0)
            lib.bertx_reset_stats(m.ctx)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert mv.add_texts(texts, colbert=colbert) == 0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep in (1, 2):
                walls.append(dt * 1e3)
            if rep == 3:
                cls = class_ms(m)
            slots, docs = mv.token_slots, len(mv)
            del mv
        lib.bertx_set_profiling(m.ctx, 0)
        emit({"part": "index", "entry": label, "arch": arch, "ftype": "q4_0", "texts": n,
              "mean_tokens_first_256": round(float(np.mean(lens)), 1), "width": width, "wall_ms": [round(w, 1) for w in walls],
              "pool_l2_ms_profiled": round(cls[0], 3), "pool_l2_launches": cls[1],
              "store_bytes_per_doc": round(slots * width * 2 / docs, 1), "token_slots": slots})


def index_plain_part(torch, lib, model_dir, emit):
    """The same corpus through _add_texts alone, for a build without the projection (the parent)."""
    arch, n = "bge-base-en-v1.5", 4096
    vocab = bertpy.bert_like_vocab(bertpy.ARCHS[arch]["n_vocab"])
    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, "%s-q4_0-text.bin" % arch)
    if not os.path.exists(path):
        bertpy.synthetic_model(path, arch, "q4_0", lib=lib, vocab=vocab)
    texts = bertpy.bert_like_texts(vocab, n, 69, seed=3)
    m = bertpy.BertModel(path)
    walls, cls = [], None
    for rep in range(4):
        mv = bertpy.BertTokenIndex(m, n, n * 192, width=768)
        lib.bertx_set_profiling(m.ctx, 1 if rep == 3 else 0)
        lib.bertx_reset_stats(m.ctx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert mv.add_texts(texts) == 0
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep in (1, 2):
            walls.append(dt * 1e3)
        if rep == 3:
            cls = class_ms(m)
        slots, docs = mv.token_slots, len(mv)
        del mv
    emit({"part": "index", "entry": "add_texts", "arch": arch, "ftype": "q4_0", "texts": n, "width": 768,
          "wall_ms": [round(w, 1) for w in walls], "pool_l2_ms_profiled": round(cls[0], 3), "pool_l2_launches": cls[1],
          "store_bytes_per_doc": round(slots * 768 * 2 / docs, 1), "token_slots": slots})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_bench.jsonl"))
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--tokens", action="store_true")
    ap.add_argument("--index", action="store_true")
    ap.add_argument("--index-plain", action="store_true")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-dir", default=os.path.join(ROOT, "build", "models"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "project_bench.py measures on a GPU"
    os.environ.setdefault("BERT_DEVICES", "0")
    lib = bertpy.load_lib()
    has_proj = hasattr(lib, "bertx_bench_project")
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        rec["lib"] = bertpy.LIB_PATH
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    if args.kernel:
        kernel_part(lib, args.rounds, emit)
    if args.tokens:
        tokens_part(torch, lib, args.model_dir, args.rounds, args.warmup, has_proj, emit)
    if args.index:
        index_part(torch, lib, args.model_dir, has_proj, emit)
    if args.index_plain:
        index_plain_part(torch, lib, args.model_dir, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
