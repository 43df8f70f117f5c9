#!/usr/bin/env python3
"""k-source fold of 64 MiB per source: sum_wide beside sum (developer tool).

gloo_hip_reduce_multi at k = 4 and k = 8 for f8e4m3 and bf16, both ops on the
same buffers, interleaved over `--reps` repetitions in one process, device
events around `--steps` launches after a warm-up.  The yardstick is `sum` in the
same run: its kernels are untouched by the wide sum.  The sources hold finite
values of magnitude below 32 (every packet takes the packed narrowing path of
either op) and dst is a buffer of its own, so every launch does the same work.
Prints one JSON line: per case both medians, their ratio, the ratio of every
repetition and sum's own spread.
  python tools/sum_wide_bench.py [--reps 5] [--steps 100]

--collective: the allreduce latency of sum_wide between rank processes on one
GPU, this tree's library beside another build's (--parent-lib, loaded through
GLOO_AMD_LIB: the yardstick) and beside `sum` on this tree, alternating over
`--reps` repetitions.  bf16; halving_doubling and ring_chunked; P = 2 with
three pointers (the wide pass is the LOCAL_REDUCE) and P = 4 with one; 1 KiB,
64 KiB, 1 MiB and 4 MiB per rank.  A repetition of a variant is one set of rank
processes that times every case: `--iters` run()s on the algorithm's own stream
(run() returns with the outputs complete) after a warm-up, host clock.  Prints
one JSON line: per case and variant the p50 of the slower rank per repetition,
the median and range of those, the launch mode reported, and whether the two
libraries' sum_wide outputs are the same bytes.
  python tools/sum_wide_bench.py --collective --parent-lib PATH [--reps 5] [--iters 400]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


SHAPES = ((2, 3), (4, 1))  # (ranks, pointers per rank)
ALGOS = ("halving_doubling", "ring_chunked")
SIZES = (1 << 10, 64 << 10, 1 << 20, 4 << 20)  # bytes per rank


def rank_main(rank, P, k, op, store, iters, warmup):
    """One rank process of a repetition: every (algo, size) case on a fresh context."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gloo_amd
    import hip_rt
    hip_rt.set_device(0)
    import time
    out = {}
    for algo in ALGOS:
        for size in SIZES:
            n = size // 2
            rng = np.random.default_rng([rank, size])
            x = [(rng.standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16) for _ in range(k)]
            bufs = [hip_rt.malloc(size) for _ in range(k)]
            ctx = gloo_amd.Context(rank, P, f"{store}_{algo}_{size}", device=0, timeout_ms=20000)
            a = gloo_amd.Algorithm(ctx, algo, op, "bf16", bufs, n)
            for b, xi in zip(bufs, x):
                hip_rt.h2d(b, xi)
            a.run()
            crc = zlib.crc32(hip_rt.d2h(bufs[0], x[0]).tobytes())  # the first run's result, for the A/B of the libraries
            for b in bufs:  # zeros from here on: the timed runs stay finite
                hip_rt.memset(b, 0, size)
            for _ in range(warmup):
                a.run()
            ts = []
            for _ in range(iters):
                t0 = time.perf_counter()
                a.run()
                ts.append((time.perf_counter() - t0) * 1e6)
            m = a.mode()
            out[f"{algo}/{size}"] = {"p50": sorted(ts)[iters // 2], "crc": crc,
                                     "mode": "interp%d" % m["interp_slices"] if m["interp"] else "graph" if m["graph"] else "eager"}
            a.close()
            ctx.close()
            for b in bufs:
                hip_rt.free(b)
    print(json.dumps(out))


def collective(args):
    variants = [("new_wide", "sum_wide", None), ("parent_wide", "sum_wide", args.parent_lib), ("new_sum", "sum", None)]
    res = {}
    for P, k in SHAPES:
        for rep in range(args.reps):
            for name, op, lib in variants:
                env = dict(os.environ, **({"GLOO_AMD_LIB": lib} if lib else {}))
                with tempfile.TemporaryDirectory() as d:
                    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--rank"]
                    procs = [subprocess.Popen(cmd + [str(r), "--size", str(P), "--ptrs", str(k), "--op", op, "--store",
                                                     "file:" + os.path.join(d, "s"), "--iters", str(args.iters), "--warmup",
                                                     str(args.warmup)], env=env, stdout=subprocess.PIPE, text=True)
                             for r in range(P)]
                    outs = [pr.communicate()[0] for pr in procs]
                    if any(pr.returncode for pr in procs):  # nothing more is started after a rank that failed
                        sys.exit(f"P{P} k{k} {name} rep {rep}: rank exits {[pr.returncode for pr in procs]}")
                ranks = [json.loads(o.strip().splitlines()[-1]) for o in outs]
                for case in ranks[0]:
                    c = res.setdefault(f"P{P}k{k}/{case}", {}).setdefault(name, {"p50_us": [], "crc": set(), "mode": set()})
                    c["p50_us"].append(round(max(r[case]["p50"] for r in ranks), 2))  # the slower rank
                    c["crc"].add(ranks[0][case]["crc"])
                    c["mode"].add(ranks[0][case]["mode"])
    for case, c in res.items():
        c["same_bytes"] = c["new_wide"]["crc"] == c["parent_wide"]["crc"] and len(c["new_wide"]["crc"]) == 1
        for v in [x for x in c.values() if isinstance(x, dict)]:
            ts = sorted(v["p50_us"])
            v.update(median_us=ts[len(ts) // 2], range_us=[ts[0], ts[-1]], mode=sorted(v["mode"]))
            del v["crc"]
    print(json.dumps({"reps": args.reps, "iters": args.iters, "cases": res}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--collective", action="store_true")
    p.add_argument("--parent-lib")
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--rank", type=int, default=-1)  # (a rank process of --collective)
    p.add_argument("--size", type=int)
    p.add_argument("--ptrs", type=int)
    p.add_argument("--op")
    p.add_argument("--store")
    p.add_argument("--src-mib", type=int, default=64)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    if args.rank >= 0:
        return rank_main(args.rank, args.size, args.ptrs, args.op, args.store, args.iters, args.warmup)
    if args.collective:
        return collective(args)
    import torch

    import gloo_amd
    assert torch.cuda.is_available(), "needs a GPU"
    nbytes = args.src_mib * (1 << 20)
    g = torch.Generator(device="cuda").manual_seed(1)

    def rand(lo, hi, n):
        return torch.randint(lo, hi, (n,), dtype=torch.uint8, device="cuda", generator=g)

    def finite(dtype):  # sign | magnitude: e4m3 up to 16, bf16 2^-7 up to 32
        if dtype == "f8e4m3":
            return rand(0, 0x59, nbytes) | (rand(0, 2, nbytes) << 7)
        hi = rand(0x3C, 0x42, nbytes // 2) | (rand(0, 2, nbytes // 2) << 7)  # bf16 high byte: 2^-7 .. 2^4
        return torch.stack([rand(0, 256, nbytes // 2), hi], dim=1).reshape(-1)

    s = torch.cuda.current_stream()
    out = {"src_mib": args.src_mib, "steps": args.steps, "reps": args.reps}
    for dtype in ("f8e4m3", "bf16"):
        srcs = [finite(dtype) for _ in range(8)]
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        n = nbytes // gloo_amd.dtype_size(dtype)
        for k in (4, 8):
            ptrs = [t.data_ptr() for t in srcs[:k]]
            res = {"sum": [], "sum_wide": []}
            for _ in range(args.reps):
                for op in ("sum", "sum_wide"):
                    for _ in range(args.warmup):
                        gloo_amd.reduce_multi_ptr(op, dtype, dst.data_ptr(), ptrs, n, s.cuda_stream)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(args.steps):
                        gloo_amd.reduce_multi_ptr(op, dtype, dst.data_ptr(), ptrs, n, s.cuda_stream)
                    e1.record(s)
                    e1.synchronize()
                    res[op].append(e0.elapsed_time(e1) * 1e3 / args.steps)
            med = {op: sorted(ts)[len(ts) // 2] for op, ts in res.items()}
            out[f"{dtype}_k{k}"] = {
                "sum_us": [round(t, 2) for t in res["sum"]], "sum_wide_us": [round(t, 2) for t in res["sum_wide"]],
                "sum_median_us": round(med["sum"], 2), "sum_wide_median_us": round(med["sum_wide"], 2),
                "wide_over_sum_median": round(med["sum_wide"] / med["sum"], 4),
                "wide_over_sum_per_rep": [round(a / b, 4) for a, b in zip(res["sum_wide"], res["sum"])],
                "sum_spread": round((max(res["sum"]) - min(res["sum"])) / med["sum"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
