"""Lookups per second of the device index (rmi_amd/index.py) against torch.searchsorted on the same device, keys and queries.

One JSON line per (index, query order):
  M   200 M uniform u64 keys, linear,linear, 2^20 leaves
  C2  200 M books-shaped u64 keys (datagen.books_u64_torch), linear,linear, 262 144 leaves
  U32 400 M uniform u32 keys, radix,linear_spline, 2^22 leaves
Query orders (2^26 queries each): "sorted" (the key set in order, evenly strided), "random" (present keys in random order),
"absent" (uniformly drawn keys, almost all absent).  Every figure is MEASURED with device events: `warmup` untimed calls,
then `reps` timed ones; median, min and max are reported.  `bytes_per_query_est` is ESTIMATED from shapes: one row, the
bisection probes of the mean window (one 64-byte sector each) and the last 128-byte line.  u64 keys go to torch as int64 with
x ^ (1 << 63), which keeps their order.

    python tools/lookup_bench.py [--only M,C2,U32] [--queries 26] [--reps 10] [--warmup 3] [--variant lane|coop|both]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


class _DevArray:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def key_tensor(tr):
    import ctypes as C
    import torch
    ptr, n, dt = C.c_void_p(), C.c_uint64(), C.c_int()
    assert tr._lib.rmi_hip_key_buffer(tr._h, C.byref(ptr), C.byref(n), C.byref(dt)) == 0
    return torch.as_tensor(_DevArray(ptr.value, n.value, "<i4" if dt.value == 1 else "<i8"), device="cuda:0")


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return ts


def spread(ts, nq):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"median_s": med, "min_s": ts[0], "max_s": ts[-1], "lookups_per_s": nq / med}


def setup(name, torch, trainer_cls):
    from rmi_amd import datagen
    tr = trainer_cls()
    if name == "M":
        tr.generate_keys("uniform", np.uint64, 200_000_000)
        spec, L, u32 = "linear,linear", 1 << 20, False
    elif name == "C2":
        kt = datagen.books_u64_torch(200_000_000, device="cuda:0")
        torch.cuda.synchronize()
        tr.set_keys(kt)
        tr._bench_keep = kt
        spec, L, u32 = "linear,linear", 262_144, False
    else:
        tr.generate_keys("uniform", np.uint32, 400_000_000)
        spec, L, u32 = "radix,linear_spline", 1 << 22, True
    rmi = tr.train(spec, L)
    return tr, rmi, spec, L, u32


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", default="M,C2,U32")
    ap.add_argument("--queries", type=int, default=26, help="log2 of the batch size")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default="both", choices=["lane", "coop", "both"])
    args = ap.parse_args(argv)
    import torch
    torch.cuda.init()                      # torch's HIP runtime first (it brings its own), then the library's
    from rmi_amd import train
    nq = 1 << args.queries
    variants = ["lane", "coop"] if args.variant == "both" else [args.variant]
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    for name in args.only.split(","):
        tr, rmi, spec, L, u32 = setup(name, torch, train.Trainer)
        ix = rmi.index()
        keys = key_tensor(tr)
        n = keys.numel()
        flip = torch.iinfo(torch.int64).min
        skeys = keys.to(torch.int64) & 0xFFFFFFFF if u32 else keys ^ flip          # order-preserving int64 image
        qs = {
            "sorted": keys[torch.arange(nq, device="cuda:0", dtype=torch.int64) * (n // nq)].contiguous(),
            "random": keys[torch.randint(0, n, (nq,), device="cuda:0", generator=g)].contiguous(),
        }
        if u32:
            qs["absent"] = torch.randint(-(1 << 31), 1 << 31, (nq,), device="cuda:0", generator=g, dtype=torch.int32)
        else:
            qs["absent"] = torch.randint(-(1 << 63), (1 << 63) - 1, (nq,), device="cuda:0", generator=g, dtype=torch.int64)
        ksz = 4 if u32 else 8
        row = rmi.params_per_leaf * 8 + 8
        for order, q in qs.items():
            sq = q.to(torch.int64) & 0xFFFFFFFF if u32 else q ^ flip
            out = {"index": name, "spec": spec, "leaves": L, "n": n, "key_bytes": ksz, "order": order, "queries": nq}
            _, e = ix.lookup(q)
            win = float((2 * e.double() + 1).mean())
            out["mean_window_keys"] = win
            probes = max(0, math.ceil(math.log2(max(1.0, (win + 2) / (128 / ksz)))))
            out["bytes_per_query_est"] = row + 64 * probes + 128
            out["lookup"] = spread(timed(lambda: ix.lookup(q), args.warmup, args.reps), nq)
            out["lookup"]["kernel_s"] = ix.last_stats.device_ns * 1e-9
            for v in variants:
                ix.set_variant(v)
                pos = ix.search(q)
                ref = torch.searchsorted(skeys, sq, side="left")
                out[f"search_{v}"] = spread(timed(lambda: ix.search(q), args.warmup, args.reps), nq)
                out[f"search_{v}"]["kernel_s"] = ix.last_stats.device_ns * 1e-9
                out[f"search_{v}"]["fallbacks"] = int(ix.last_stats.fallbacks)
                out[f"search_{v}"]["equal_to_searchsorted"] = bool((pos == ref).all())
                del pos
            ix.set_variant("lane")
            out["torch_searchsorted"] = spread(timed(lambda: torch.searchsorted(skeys, sq, side="left"), args.warmup, args.reps), nq)
            best = min(out[f"search_{v}"]["median_s"] for v in variants)
            out["search_speedup_vs_searchsorted"] = out["torch_searchsorted"]["median_s"] / best
            print(json.dumps(out), flush=True)
        ix.close()
        del keys, skeys, qs
        tr.close()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
