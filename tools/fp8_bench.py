#!/usr/bin/env python3
"""64 MiB in-place chunk reduction: f8e4m3 sum and f8e5m2 sum beside u8 sum
(developer tool).

The memory stream of the three kernels is identical (2 reads + 1 write per
byte); the FP8 kernels add 12 convert / packed-f32 instructions and 4 compares
per dword, so the question is whether they stay memory-bound.  Measured the way
bench.py measures its config 2: `--pairs` (dst, src) pairs rotated (6 x 2 x
64 MiB = 768 MiB, 3x the Infinity Cache) so that every launch streams from HBM,
a warm-up before each timed window, device events around `--steps` launches;
the cases alternate over `--reps` repetitions in one process.

dst holds finite values with |v| <= 16 and src holds +0 / -0, so the in-place
sums leave dst as it is however often they run and every packet takes the
packed path.  The case "f8e4m3_nan" is the other extreme: dst all NaN, every
packet redone element by element (the rare path's cost, not a bucket anybody
reduces).  Prints one JSON line.
  python tools/fp8_bench.py [--reps 5] [--steps 300]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E, datasheet
CASES = [("u8", "u8"), ("f8e4m3", "f8e4m3"), ("f8e5m2", "f8e5m2"), ("f8e4m3_nan", "f8e4m3")]


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
    n = args.chunk_mib * (1 << 20)
    g = torch.Generator(device="cuda").manual_seed(1)

    def rand(lo, hi):
        return torch.randint(lo, hi, (n,), dtype=torch.uint8, device="cuda", generator=g)

    # sign bit | magnitude byte below 0x58 (e4m3fn 16.0) / 0x4C (e5m2 16.0): finite, |v| <= 16
    finite = {"u8": lambda: rand(0, 256), "f8e4m3": lambda: rand(0, 0x59) | (rand(0, 2) << 7),
              "f8e5m2": lambda: rand(0, 0x4D) | (rand(0, 2) << 7),
              "f8e4m3_nan": lambda: torch.full((n,), 0x7F, dtype=torch.uint8, device="cuda")}
    zeros = lambda: rand(0, 2) << 7  # noqa: E731  (+0 / -0; for u8: 0 / 128)
    pairs = {name: [(finite[name](), zeros()) for _ in range(args.pairs)] for name, _ in CASES}
    s = torch.cuda.current_stream()

    def launches(name, dtype, k):
        for i in range(k):
            d, x = pairs[name][i % args.pairs]
            gloo_amd.reduce_ptr("sum", dtype, d.data_ptr(), x.data_ptr(), n, s.cuda_stream)

    res = {name: [] for name, _ in CASES}
    for _ in range(args.reps):
        for name, dtype in CASES:
            launches(name, dtype, args.warmup)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            launches(name, dtype, args.steps)
            e1.record(s)
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e-3 / args.steps)
    nbytes = 3 * n
    out = {"chunk_mib": args.chunk_mib, "op": "sum", "pairs": args.pairs, "steps": args.steps, "reps": args.reps}
    for name, ts in res.items():
        out[name] = {"us_per_launch": [round(t * 1e6, 3) for t in ts],
                     "fraction_of_8TBps": [round(nbytes / t / PEAK_BYTES_PER_S, 4) for t in ts]}
    med = {name: sorted(ts)[len(ts) // 2] for name, ts in res.items()}
    for name in ("f8e4m3", "f8e5m2", "f8e4m3_nan"):
        out[name + "_over_u8_median_time"] = round(med[name] / med["u8"], 4)
        out[name + "_over_u8_per_rep"] = [round(a / b, 4) for a, b in zip(res[name], res["u8"])]
    out["u8_spread"] = round((max(res["u8"]) - min(res["u8"])) / med["u8"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
