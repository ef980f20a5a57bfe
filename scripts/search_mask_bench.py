#!/usr/bin/env python3
"""What row masks cost the embedding index's search, by the method of
search_bench.py: device events, R rounds after warm-up launches, median (min-max).

One process measures one libbert.so (--lib, default the build's; --label names it in the
records), through ctypes alone, so that a library from before the masks existed can be
measured by the same code in the same session.  Per storage kind an index of N random unit
rows of width d is filled from HBM (bertx_index_add_device).  Per B, in every round one launch
of each of these in turn on one stream, each between its own pair of device events:
  plain             bertx_index_search_device on the untouched index (the unmasked kernels);
and, where the library has them,
  ones shared       bertx_index_search_filtered_device, one all-ones filter for every query;
  ones per query    ... B all-ones filters;
  random 1/16       ... one shared filter that admits a random sixteenth of the rows;
  range 1/16        ... one shared filter that admits rows [N / 2, N / 2 + N / 16).
Then a random sixteenth of the rows is removed (bertx_index_remove_device) and
  deleted 1/16      bertx_index_search_device on the index with deletions
is measured the same way.  One JSON line per (kind, B) is appended to --out (default
profiles/search_mask_bench.jsonl).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "embeddings.cpp_amd"))

STORAGE = {"f16": 0, "int8": 1, "binary": 8}
BYTES = {"f16": lambda N, d: N * d * 2, "int8": lambda N, d: N * (d + 4), "binary": lambda N, d: N * d // 8}


def load(path):
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.bert_load_from_file.restype = vp
    L.bert_load_from_file.argtypes = [ctypes.c_char_p]
    L.bert_free.argtypes = [vp]
    L.bertx_index_create_ex.restype = vp
    L.bertx_index_create_ex.argtypes = [vp, i32, i32, i32]
    L.bertx_index_free.argtypes = [vp]
    L.bertx_index_add_device.restype = i32
    L.bertx_index_add_device.argtypes = [vp, vp, i32, vp]
    L.bertx_index_search_device.restype = i32
    L.bertx_index_search_device.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    masks = hasattr(L, "bertx_index_search_filtered_device")
    if masks:
        L.bertx_index_search_filtered_device.restype = i32
        L.bertx_index_search_filtered_device.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp, vp, vp]
        L.bertx_index_remove_device.restype = i32
        L.bertx_index_remove_device.argtypes = [vp, vp, i32, vp]
        L.bertx_index_live.restype = i32
        L.bertx_index_live.argtypes = [vp]
    return L, masks


def unit_rows(torch, n, d, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(n, d, generator=g, device="cuda", dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def pack(torch, allow):
    """bool [.., N] on the device -> int32 words [.., N / 32]: row r = bit r % 32 of word r / 32."""
    w = allow.reshape(*allow.shape[:-1], -1, 32).to(torch.int64) << torch.arange(32, device="cuda")
    v = w.sum(dim=-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).contiguous()


def summary(t):
    return {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def timed(torch, stream, calls, rounds, warm):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in calls}
    with torch.cuda.stream(stream):
        for _ in range(warm):
            for fn in calls.values():
                assert fn() == 0
        stream.synchronize()
        for _ in range(rounds):
            for name, fn in calls.items():
                a.record(stream)
                rc = fn()
                b.record(stream)
                b.synchronize()
                assert rc == 0, (name, rc)
                times[name].append(a.elapsed_time(b) * 1e3)
    return {name: summary(t) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "build", "libbert.so"))
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_mask_bench.jsonl"))
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "search_mask_bench.py measures on a GPU"
    os.environ.setdefault("BERT_DEVICES", "0")
    import bertpy   # (for the synthetic model file only: the library under test is loaded here)
    lib, masks = load(args.lib)
    N, d, k = args.rows, args.width, args.k
    assert N % 32 == 0
    batches = [int(x) for x in args.batches.split(",")]
    stream = torch.cuda.Stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    f = open(args.out, "a")

    def emit(rec):
        rec.update({"lib": args.label, "device": torch.cuda.get_device_name(0), "d": d, "N": N, "k": k, "rounds": args.rounds})
        f.write(json.dumps(rec) + "\n")
        f.flush()
        print(json.dumps(rec), flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w%d.bin" % d)
        hp = dict(n_vocab=256, n_max_tokens=32, n_embd=d, n_intermediate=128, n_head=d // 64, n_layer=1)
        bertpy.synthetic_model(path, hp, "f16")
        ctx = lib.bert_load_from_file(path.encode())
        assert ctx
        g = torch.Generator(device="cuda")
        g.manual_seed(99)
        sixteenth = torch.rand(N, generator=g, device="cuda") < 1.0 / 16
        in_range = torch.zeros(N, dtype=torch.bool, device="cuda")
        in_range[N // 2:N // 2 + N // 16] = True
        gone = torch.nonzero(torch.rand(N, generator=g, device="cuda") < 1.0 / 16).to(torch.int32).reshape(-1).contiguous()
        B_max, words = max(batches), N // 32
        ones = torch.full((B_max, words), -1, dtype=torch.int32, device="cuda")
        f_random, f_range = pack(torch, sixteenth), pack(torch, in_range)
        sc = torch.empty(B_max, k, device="cuda", dtype=torch.float32)
        ids = torch.empty(B_max, k, device="cuda", dtype=torch.int32)
        for kind, storage in STORAGE.items():
            ix = lib.bertx_index_create_ex(ctx, 0, N, storage)
            assert ix
            with torch.cuda.stream(stream):
                for i in range(0, N, 1 << 16):
                    rows = unit_rows(torch, min(1 << 16, N - i), d, i)
                    stream.synchronize()
                    assert lib.bertx_index_add_device(ix, rows.data_ptr(), rows.shape[0], sp) == i
                    stream.synchronize()
            results = {}
            for B in batches:
                Q = unit_rows(torch, B, d, 1000 + B)
                results[B] = Q
                calls = {"plain": lambda: lib.bertx_index_search_device(ix, Q.data_ptr(), B, k, sc.data_ptr(), ids.data_ptr(), sp)}
                if masks:
                    def filt(buf, n):
                        return lambda: lib.bertx_index_search_filtered_device(ix, Q.data_ptr(), B, k, buf.data_ptr(), n, words,
                                                                              sc.data_ptr(), ids.data_ptr(), sp)
                    calls["ones shared"] = filt(ones, 1)
                    calls["ones per query"] = filt(ones, B)
                    calls["random 1/16"] = filt(f_random, 1)
                    calls["range 1/16"] = filt(f_range, 1)
                rec = {"kind": kind, "B": B, "stored_bytes": BYTES[kind](N, d)}
                rec.update(timed(torch, stream, calls, args.rounds, args.warmup))
                emit(rec)
            if masks:
                assert lib.bertx_index_remove_device(ix, gone.data_ptr(), gone.numel(), sp) == 0
                stream.synchronize()
                live = lib.bertx_index_live(ix)
                assert live == N - gone.numel()
                for B in batches:
                    Q = results[B]
                    calls = {"deleted 1/16": lambda: lib.bertx_index_search_device(ix, Q.data_ptr(), B, k, sc.data_ptr(),
                                                                                   ids.data_ptr(), sp)}
                    rec = {"kind": kind, "B": B, "live": live}
                    rec.update(timed(torch, stream, calls, args.rounds, args.warmup))
                    emit(rec)
            lib.bertx_index_free(ix)
        lib.bert_free(ctx)
    f.close()


if __name__ == "__main__":
    main()
