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
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--src-mib", type=int, default=64)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
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
