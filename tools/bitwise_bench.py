#!/usr/bin/env python3
"""64 MiB u32 in-place chunk reduction: built-in bxor beside sum (developer tool).

The memory stream of the two kernels is identical (2 reads + 1 write per
element), so they should time alike.  Measured the way bench.py measures its
config 2: `--pairs` (dst, src) pairs rotated (6 x 2 x 64 MiB = 768 MiB, 3x the
Infinity Cache) so that every launch streams from HBM, a warm-up before each
timed window, device events around `--steps` launches; the two ops alternate
over `--reps` repetitions in one process.  Prints one JSON line.
  python tools/bitwise_bench.py [--reps 5] [--steps 300]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E, datasheet


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--chunk-mib", type=int, default=64)
    p.add_argument("--pairs", type=int, default=6)
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=30)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    import torch

    import gloo_amd
    assert torch.cuda.is_available(), "needs a GPU"
    n = args.chunk_mib * (1 << 20) // 4
    g = torch.Generator(device="cuda").manual_seed(1)
    pairs = [(torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device="cuda", generator=g),
              torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device="cuda", generator=g))
             for _ in range(args.pairs)]
    s = torch.cuda.current_stream()

    def launches(op, k):
        for i in range(k):
            d, x = pairs[i % args.pairs]
            gloo_amd.reduce_ptr(op, "u32", d.data_ptr(), x.data_ptr(), n, s.cuda_stream)

    res = {"sum": [], "bxor": []}
    for _ in range(args.reps):
        for op in ("sum", "bxor"):
            launches(op, args.warmup)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            launches(op, args.steps)
            e1.record(s)
            e1.synchronize()
            res[op].append(e0.elapsed_time(e1) * 1e-3 / args.steps)
    nbytes = 3 * n * 4
    out = {"chunk_mib": args.chunk_mib, "dtype": "u32", "pairs": args.pairs, "steps": args.steps, "reps": args.reps}
    for op, ts in res.items():
        out[op] = {"us_per_launch": [round(t * 1e6, 3) for t in ts],
                   "fraction_of_8TBps": [round(nbytes / t / PEAK_BYTES_PER_S, 4) for t in ts]}
    med = {op: sorted(ts)[len(ts) // 2] for op, ts in res.items()}
    out["bxor_over_sum_median_time"] = round(med["bxor"] / med["sum"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
