#!/usr/bin/env python3
"""One allgather beside the P broadcasts that emulate it (developer tool).

P rank processes on GPU 0, `--elems` u8 per rank.  Every rank alternates
  (a) one gloo_amd.allgather of its input into the output, and
  (b) P gloo_amd.broadcast calls with rotating root, each rank's input going
      to the same output slot the allgather fills (root r's slot r),
`--reps` times each after `--warmup` of each, and reports the mean and least
host time per collective for both.  Calls run on the library's own stream and
return with the output complete, so the host clock covers the device work.
Both forms are checked against each other once before the timing.  Prints one
JSON line per rank and a summary.
  python tools/allgather_vs_bcast.py [--ranks 4] [--elems 16777216] [--reps 20]
All ranks share one GPU: nothing here goes over xGMI.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, os, sys, time
sys.path.insert(0, os.environ["GLOO_AMD_ROOT"])
import torch, gloo_amd
rank, P, store, n, reps, warmup = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
torch.cuda.set_device(0)
g = torch.Generator(device="cuda").manual_seed(rank + 1)
inp = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
out_a = torch.zeros(P * n, dtype=torch.uint8, device="cuda")
out_b = torch.zeros(P * n, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ctx = gloo_amd.Context(rank, P, store, device=0, timeout_ms=60000)
def allgather():
    gloo_amd.allgather(ctx, out_a.data_ptr(), n, "u8", input=inp.data_ptr())
def broadcasts():
    for root in range(P):
        gloo_amd.broadcast(ctx, out_b.data_ptr() + root * n, n, "u8", root, input=inp.data_ptr() if root == rank else None,
                           tag=1 + root)
allgather(); broadcasts()
torch.cuda.synchronize()
assert torch.equal(out_a, out_b), "the two forms disagree"
assert torch.equal(out_a[rank * n:(rank + 1) * n], inp)
for _ in range(warmup):
    allgather(); broadcasts()
ta, tb = [], []
for _ in range(reps):
    t = time.perf_counter(); allgather(); ta.append(time.perf_counter() - t)
    t = time.perf_counter(); broadcasts(); tb.append(time.perf_counter() - t)
print(json.dumps({"rank": rank, "allgather_mean_us": round(1e6 * sum(ta) / reps, 1), "allgather_least_us": round(1e6 * min(ta), 1),
                  "broadcasts_mean_us": round(1e6 * sum(tb) / reps, 1), "broadcasts_least_us": round(1e6 * min(tb), 1)}), flush=True)
ctx.close()
'''


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ranks", type=int, default=4)
    p.add_argument("--elems", type=int, default=16 << 20)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(WORKER)
        env = dict(os.environ, GLOO_AMD_ROOT=ROOT)
        procs = [subprocess.Popen([sys.executable, "-u", w, str(r), str(args.ranks), "file:" + os.path.join(d, "s"),
                                   str(args.elems), str(args.reps), str(args.warmup)], env=env, stdout=subprocess.PIPE,
                                  text=True) for r in range(args.ranks)]
        outs = []
        rcs = []
        for q in procs:
            try:
                o, _ = q.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for k in procs:
                    k.kill()
                raise
            outs.append(o)
            rcs.append(q.returncode)
    rows = [json.loads(o.strip().splitlines()[-1]) for o, rc in zip(outs, rcs) if rc == 0 and o.strip()]
    for r in rows:
        print(json.dumps(r))
    if len(rows) != args.ranks:
        print("exit codes", rcs)
        sys.exit(1)
    ag = sum(r["allgather_mean_us"] for r in rows) / len(rows)
    bc = sum(r["broadcasts_mean_us"] for r in rows) / len(rows)
    print(json.dumps({"ranks": args.ranks, "elems_per_rank": args.elems, "reps": args.reps,
                      "allgather_mean_us": round(ag, 1), "broadcasts_mean_us": round(bc, 1),
                      "broadcasts_over_allgather": round(bc / ag, 3)}))


if __name__ == "__main__":
    main()
