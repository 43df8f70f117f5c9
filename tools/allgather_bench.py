#!/usr/bin/env python3
"""The allgather sender's pass on one GPU: k = 2 inputs of 32 MiB laid side by
side into the rank's own slot and into 7 inbox-like destinations — developer
tool.

  fused:  gloo_hip_gather_fanout_kernel, ONE launch that reads every input
          tile once and stores it 8 times (2 reads + 16 writes of 32 MiB);
  split:  what the kernels before it can do: gloo_hip_copy_kernel_multi of the
          two inputs into the slot (2 reads + 2 writes), then
          gloo_hip_fanout_kernel of the slot to the 7 destinations (2 reads +
          14 writes): about 10 % more bytes and one launch more.

Both run from a footprint larger than the Infinity Cache: `--sets` sets of
(2 inputs, 8 destinations) are rotated (2 x 576 MiB), the bytes are random, a
warm-up precedes each timed window, device events bracket `--steps` launches,
and the variants alternate over `--reps` repetitions in one process.  Each
runs at several grid sizes; the ratio is taken between the best medians, and
the spread of each (min .. max over the repetitions) is printed with it.
Destinations start one byte apart in their 16-byte misalignment, as inbox
regions may.  Prints one JSON line.
  python tools/allgather_bench.py [--reps 5] [--steps 40]
Nothing here goes over xGMI: every buffer is in the one GPU's HBM.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NDST, K = 8, 2  # the own slot + 7 inboxes; inputs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--input-mib", type=int, default=32)
    p.add_argument("--sets", type=int, default=2)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args()
    import torch

    import gloo_amd
    assert torch.cuda.is_available(), "needs a GPU"
    n = args.input_mib << 20
    g = torch.Generator(device="cuda").manual_seed(1)
    sets = []
    for _ in range(args.sets):
        ins = [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(K)]
        dsts = [torch.empty(K * n + 16, dtype=torch.uint8, device="cuda") for _ in range(NDST)]
        sets.append((ins, dsts, [d.data_ptr() + j for j, d in enumerate(dsts)]))
    s = torch.cuda.current_stream()

    def fused(blocks):
        def go(i):
            ins, _, dp = sets[i % args.sets]
            gloo_amd.gather_fanout_kernel(dp, [t.data_ptr() for t in ins], n, blocks, s.cuda_stream)
        return go

    def split(blocks):
        def go(i):
            ins, _, dp = sets[i % args.sets]
            gloo_amd.copy_kernel_multi([dp[0] + j * n for j in range(K)], [t.data_ptr() for t in ins], n, blocks,
                                       s.cuda_stream)
            gloo_amd.fanout_kernel(dp[1:], dp[0], K * n, blocks, s.cuda_stream)
        return go

    variants = {f"fused_{b}": fused(b) for b in (256, 512, 1024)}
    variants.update({f"split_{b}": split(b) for b in (256, 512, 1024)})
    # both leave the inputs side by side in every destination
    for name, go in variants.items():
        for _, dsts, _ in sets:
            for d in dsts:
                d.zero_()
        for i in range(args.sets):
            go(i)
        torch.cuda.synchronize()
        for ins, dsts, _ in sets:
            for j, d in enumerate(dsts):
                for q in range(K):
                    assert torch.equal(d[j + q * n:j + (q + 1) * n], ins[q]), (name, j, q)
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
    out = {"input_mib": args.input_mib, "inputs": K, "destinations": NDST, "sets": args.sets, "steps": args.steps,
           "reps": args.reps}
    med = {}
    for name, ts in res.items():
        med[name] = sorted(ts)[len(ts) // 2]
        out[name] = {"us_per_pass": [round(t * 1e6, 1) for t in ts],
                     "median_us": round(med[name] * 1e6, 1),
                     "spread": round((max(ts) - min(ts)) / med[name], 4),
                     "stored_TBps": round(NDST * K * n / med[name] / 1e12, 3)}
    bf = min((k for k in med if k.startswith("fused")), key=med.get)
    bs = min((k for k in med if k.startswith("split")), key=med.get)
    out["best"] = {"fused": bf, "split": bs}
    out["split_over_fused_median_time"] = round(med[bs] / med[bf], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
