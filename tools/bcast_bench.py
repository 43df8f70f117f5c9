#!/usr/bin/env python3
"""One 64 MiB source to 7 destinations on one GPU: the broadcast root's
one-pass fan-out (gloo_hip_fanout_kernel, each tile loaded once and stored 7
times: 8n bytes of traffic) beside what the executor had before it,
gloo_hip_copy_kernel_multi (7 copies in one launch, the source read 7 times:
14n bytes) — developer tool.

How much of the repeated read the Infinity Cache absorbs decides the gain, so
both run from a footprint larger than it: `--sets` sets of (source, 7
destinations) are rotated (2 x 8 x 64 MiB = 1 GiB, 4x the cache), the bytes
are random, a warm-up precedes each timed window, device events bracket
`--steps` launches, and the variants alternate over `--reps` repetitions in
one process.  Each kernel runs at several grid sizes; the ratio is taken
between the best medians, and the spread of each (min .. max over the
repetitions) is printed with it.  Destinations start one byte apart in their
16-byte misalignment, as inbox regions may.  Prints one JSON line.
  python tools/bcast_bench.py [--reps 5] [--steps 40]
Nothing here goes over xGMI: every buffer is in the one GPU's HBM.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NDST = 7


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--src-mib", type=int, default=64)
    p.add_argument("--sets", type=int, default=2)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    import torch

    import gloo_amd
    assert torch.cuda.is_available(), "needs a GPU"
    n = args.src_mib << 20
    g = torch.Generator(device="cuda").manual_seed(1)
    sets = []
    for _ in range(args.sets):
        src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        dsts = [torch.empty(n + 16, dtype=torch.uint8, device="cuda") for _ in range(NDST)]
        sets.append((src, dsts, [d.data_ptr() + j for j, d in enumerate(dsts)]))
    s = torch.cuda.current_stream()

    def fanout(blocks):
        def go(i):
            src, _, dp = sets[i % args.sets]
            gloo_amd.fanout_kernel(dp, src.data_ptr(), n, blocks, s.cuda_stream)
        return go

    def multi(blocks):
        def go(i):
            src, _, dp = sets[i % args.sets]
            gloo_amd.copy_kernel_multi(dp, [src.data_ptr()] * NDST, n, blocks, s.cuda_stream)
        return go

    variants = {f"fanout_{b}": fanout(b) for b in (256, 512, 1024)}
    variants.update({f"multi_{b}": multi(b) for b in (64, 128, 256)})
    # both give the source's bytes in every destination
    for name, go in variants.items():
        for _, dsts, _ in sets:
            for d in dsts:
                d.zero_()
        for i in range(args.sets):
            go(i)
        torch.cuda.synchronize()
        for src, dsts, _ in sets:
            for j, d in enumerate(dsts):
                assert torch.equal(d[j:j + n], src), (name, j)
    res = {k: [] for k in variants}
    for _ in range(args.reps):
        for name, go in variants.items():
            for i in range(args.warmup):
                go(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(args.steps):
                go(i)
            e1.record(s)
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e-3 / args.steps)
    out = {"src_mib": args.src_mib, "destinations": NDST, "sets": args.sets, "steps": args.steps, "reps": args.reps}
    med = {}
    for name, ts in res.items():
        med[name] = sorted(ts)[len(ts) // 2]
        out[name] = {"us_per_launch": [round(t * 1e6, 1) for t in ts],
                     "median_us": round(med[name] * 1e6, 1),
                     "spread": round((max(ts) - min(ts)) / med[name], 4),
                     "stored_TBps": round(NDST * n / med[name] / 1e12, 3)}
    bf = min((k for k in med if k.startswith("fanout")), key=med.get)
    bm = min((k for k in med if k.startswith("multi")), key=med.get)
    out["best"] = {"fanout": bf, "multi": bm}
    out["multi_over_fanout_median_time"] = round(med[bm] / med[bf], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
