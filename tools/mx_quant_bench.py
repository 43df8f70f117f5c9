#!/usr/bin/env python3
"""MX quantise and wide-output MX fold of 64 MiB of wide bytes beside the MX
sum (developer tool).

For bf16 and f32 into MXFP8 e4m3 and MXFP4: gloo_amd.quantise_mx_ptr beside
reduce_mx at k = 1, and reduce_mx_wide_ptr at k = 2 and k = 8 beside reduce_mx
at the same format and k (the existing kernel, the yardstick), interleaved
over `--reps` repetitions in one process: device events around `--steps`
launches after a warm-up.  The wide tensor is `--wide-mib` MiB, so the MX side
is 1/2 to 1/8 of that.  Wide sources rotate through six tensors (384 MiB) and
MX sources through the slots of a 384 MiB arena, 1.5x the Infinity Cache, so
every launch streams from HBM; destinations are buffers of their own.  All
values are finite and the scales lie in [120, 134].  The quantise runs in both
rounding modes, round to nearest even and stochastic (`quantise_sr`, a new seed
per launch), in the same interleaving.  Prints one JSON line: per case the
times of every repetition, the median, the spread (max - min) / median, GiB/s
over the bytes read plus the bytes written, the ratio of that rate to
reduce_mx's, and for the stochastic row its ratio to the round-to-nearest one.
  --alt-lib PATH: a second build of the library (for instance one compiled with
  -DGLOO_MX_WIDE_STORE=1) whose wide fold is timed in the same interleaving.
  python tools/mx_quant_bench.py [--reps 5] [--steps 60] [--warmup 10] [--alt-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDE_POOL, ARENA_MIB = 6, 384


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--wide-mib", type=int, default=64)
    p.add_argument("--steps", type=int, default=60)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--alt-lib", default=None)
    args = p.parse_args()
    import torch

    import gloo_amd
    assert torch.cuda.is_available(), "needs a GPU"
    wbytes, arena_bytes = args.wide_mib << 20, ARENA_MIB << 20
    g = torch.Generator(device="cuda").manual_seed(1)

    def rand(lo, hi, n):
        return torch.randint(lo, hi, (n,), dtype=torch.uint8, device="cuda", generator=g)

    # e4m3 magnitudes up to 16 under either reading of the bytes; every e2m1 nibble is finite
    arena = rand(0, 0x59, arena_bytes) | (rand(0, 2, arena_bytes) << 7)
    scale_arena = rand(120, 135, arena_bytes // 16)
    wide = {dt: [torch.randn(wbytes // sz, dtype=td, device="cuda", generator=g) for _ in range(WIDE_POOL)]
            for dt, td, sz in (("bf16", torch.bfloat16, 2), ("f32", torch.float32, 4))}
    wide_dst = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    mx_dst, mx_dst_scales = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (wbytes // 2, wbytes // 64))
    s = torch.cuda.current_stream().cuda_stream
    alt = None
    if args.alt_lib:
        alt = ctypes.CDLL(args.alt_lib)
        alt.gloo_hip_reduce_mx_wide.argtypes = gloo_amd.lib.gloo_hip_reduce_mx_wide.argtypes

    out = {"wide_mib": args.wide_mib, "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "lib": gloo_amd.LIB_PATH,
           "alt_lib": args.alt_lib}
    for dt in ("bf16", "f32"):
        for fmt, bb in (("mxfp8_e4m3", 32), ("mxfp4_e2m1", 16)):
            nblocks = wbytes // (2 if dt == "bf16" else 4) // 32
            eb, nslots = nblocks * bb, arena_bytes // (nblocks * bb)

            def sources(k, step):
                slots = [(step * k + j) % nslots for j in range(k)]
                return [arena.data_ptr() + i * eb for i in slots], [scale_arena.data_ptr() + i * nblocks for i in slots]

            def launch(name, k, step):
                if name in ("quantise", "quantise_sr"):
                    gloo_amd.quantise_mx_ptr(fmt, dt, mx_dst.data_ptr(), mx_dst_scales.data_ptr(),
                                             wide[dt][step % WIDE_POOL].data_ptr(), nblocks, s,
                                             seed=step if name == "quantise_sr" else None)
                elif name == "reduce_mx":
                    gloo_amd.reduce_mx_ptr(fmt, mx_dst.data_ptr(), mx_dst_scales.data_ptr(), *sources(k, step), nblocks, s)
                elif name == "wide":
                    gloo_amd.reduce_mx_wide_ptr(fmt, dt, wide_dst.data_ptr(), *sources(k, step), nblocks, s)
                else:
                    vp = ctypes.c_void_p
                    e, x = sources(k, step)
                    rc = alt.gloo_hip_reduce_mx_wide(int(gloo_amd.MX_FORMAT_NAMES[fmt]), int(gloo_amd.DTYPE_NAMES[dt]),
                                                     wide_dst.data_ptr(), (vp * k)(*e), (vp * k)(*x), k, nblocks, s)
                    assert rc == 0, rc

            for k, new in ((1, "quantise"), (2, "wide"), (8, "wide")):
                names = (new,) + (("quantise_sr",) if new == "quantise" else ()) + ("reduce_mx",)
                names += ("wide_alt",) if alt and new == "wide" else ()
                moved = {"quantise": wbytes + eb + nblocks, "reduce_mx": (k + 1) * (eb + nblocks)}
                moved["quantise_sr"] = moved["quantise"]
                moved["wide"] = moved["wide_alt"] = k * (eb + nblocks) + wbytes
                us = {n: [] for n in names}
                for _ in range(args.reps):
                    for name in names:
                        for i in range(args.warmup):
                            launch(name, k, i)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(args.steps):
                            launch(name, k, i)
                        e1.record()
                        e1.synchronize()
                        us[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
                med = {n: sorted(t)[len(t) // 2] for n, t in us.items()}
                rate = {n: moved[n] / (med[n] * 1e-6) / 2 ** 30 for n in names}
                out[f"{dt}_{fmt}_{new}_k{k}"] = {
                    n: {"us": [round(t, 2) for t in us[n]], "median_us": round(med[n], 2), "gib_s": round(rate[n], 1),
                        "spread": round((max(us[n]) - min(us[n])) / med[n], 4),
                        "rate_over_reduce_mx": round(rate[n] / rate["reduce_mx"], 4)} for n in names}
                if new == "quantise":
                    out[f"{dt}_{fmt}_{new}_k{k}"]["quantise_sr"]["rate_over_nearest"] = round(rate["quantise_sr"] / rate[new], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
