#!/usr/bin/env python3
"""MX block-scaled sum of 64 MiB of element bytes per source beside the wide
sum (developer tool).

gloo_amd.reduce_mx for MXFP8 e4m3 and MXFP4 at k = 2 and k = 8, each in both
rounding modes (`*_sr`: stochastic, a new seed per launch), interleaved
with gloo_hip_reduce_multi SUM_WIDE on F8E4M3 at the same k and the same
element bytes (the existing fold with the same traffic minus the 1/32 of scale
bytes; at k = 2 that op is SUM), over `--reps` repetitions in one process:
device events around `--steps` launches after a warm-up.  Sources rotate
through a pool of twelve buffers (768 MiB, 3x the Infinity Cache), so every
launch streams from HBM; dst is a buffer of its own.  The elements are finite
and the scales lie in [120, 134], so no block is a NaN block.  Prints one JSON
line: per case the times of every repetition, the median, GiB/s over
(k + 1) * 33/32 * element bytes (the wide sum: (k + 1) * element bytes), the
ratio of the rates to the wide sum's, the wide sum's own spread, and for a
stochastic row its ratio to the round-to-nearest row of the same format.
  python tools/mx_reduce_bench.py [--reps 5] [--steps 60] [--warmup 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POOL = 12


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--src-mib", type=int, default=64)
    p.add_argument("--steps", type=int, default=60)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    import torch

    import gloo_amd
    assert torch.cuda.is_available(), "needs a GPU"
    nbytes = args.src_mib << 20
    g = torch.Generator(device="cuda").manual_seed(1)

    def rand(lo, hi, n):
        return torch.randint(lo, hi, (n,), dtype=torch.uint8, device="cuda", generator=g)

    # e4m3 magnitudes up to 16 under either reading of the bytes; every e2m1 nibble is finite
    elems = [rand(0, 0x59, nbytes) | (rand(0, 2, nbytes) << 7) for _ in range(POOL)]
    scales = {fmt: [rand(120, 135, nbytes // bb) for _ in range(POOL)] for fmt, bb in (("mxfp8_e4m3", 32), ("mxfp4_e2m1", 16))}
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst_scales = torch.empty(nbytes // 16, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()

    def launch(name, k, step):
        pick = [(step * k + j) % POOL for j in range(k)]
        if name == "sum_wide":
            gloo_amd.reduce_multi_ptr("sum_wide", "f8e4m3", dst.data_ptr(), [elems[i].data_ptr() for i in pick], nbytes,
                                      s.cuda_stream)
        else:
            fmt = name[:-3] if name.endswith("_sr") else name
            nblocks = scales[fmt][0].numel()
            gloo_amd.reduce_mx_ptr(fmt, dst.data_ptr(), dst_scales.data_ptr(), [elems[i].data_ptr() for i in pick],
                                   [scales[fmt][i].data_ptr() for i in pick], nblocks, s.cuda_stream,
                                   seed=step if fmt != name else None)

    out = {"src_mib": args.src_mib, "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "lib": gloo_amd.LIB_PATH}
    names = ("sum_wide", "mxfp8_e4m3", "mxfp8_e4m3_sr", "mxfp4_e2m1", "mxfp4_e2m1_sr")
    for k in (2, 8):
        us = {n: [] for n in names}
        for _ in range(args.reps):
            for name in names:
                for i in range(args.warmup):
                    launch(name, k, i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for i in range(args.steps):
                    launch(name, k, i)
                e1.record(s)
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
        med = {n: sorted(t)[len(t) // 2] for n, t in us.items()}
        moved = {n: (k + 1) * nbytes * (1 if n == "sum_wide" else 33 / 32) for n in names}
        rate = {n: moved[n] / (med[n] * 1e-6) / 2 ** 30 for n in names}
        case = {"sum_wide_spread": round((max(us["sum_wide"]) - min(us["sum_wide"])) / med["sum_wide"], 4)}
        for n in names:
            case[n] = {"us": [round(t, 2) for t in us[n]], "median_us": round(med[n], 2), "gib_s": round(rate[n], 1),
                       "spread": round((max(us[n]) - min(us[n])) / med[n], 4),
                       "rate_over_sum_wide": round(rate[n] / rate["sum_wide"], 4)}
        for n in names:
            if n.endswith("_sr"):
                case[n]["rate_over_nearest"] = round(rate[n] / rate[n[:-3]], 4)
        out[f"k{k}"] = case
    print(json.dumps(out))


if __name__ == "__main__":
    main()
