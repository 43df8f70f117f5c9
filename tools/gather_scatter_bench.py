#!/usr/bin/env python3
"""Gather and scatter beside the collectives that emulate them (developer tool).

P rank processes on GPU 0, `--elems` u8 per block, root 0.  Every rank times
  gather     one gloo_amd.gather into the root's output,
  allgather  the gloo_amd.allgather that emulates it (P times the bytes, and a
             P * n output on every rank),
  scatter    one gloo_amd.scatter of the root's P inputs,
  bcasts     the P gloo_amd.broadcast calls that emulate it (input q to every
             rank, rank q keeping it),
in `--rounds` alternating rounds of `--reps` calls each (after `--warmup` of
each), on the same build and in the same processes.  Calls run on the
library's own stream and return with the output complete, so the host clock
covers the device work; the figure per round is the mean over the ranks of
each rank's mean time per call.  Every form is checked against its model once
before the timing.  Prints one JSON line per rank and a summary with the
rounds' values and their spread ((max - min) / mean over the rounds).
  python tools/gather_scatter_bench.py [--ranks 4] [--elems 16777216] [--reps 20] [--rounds 3]
All ranks share one GPU: nothing here goes over xGMI.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("gather", "allgather", "scatter", "bcasts")

WORKER = r'''
import json, os, sys, time
sys.path.insert(0, os.environ["GLOO_AMD_ROOT"])
import torch, gloo_amd
rank, P, store, n, reps, warmup, rounds = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], *map(int, sys.argv[4:8])
root = 0
torch.cuda.set_device(0)
def rand(seed, m):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (m,), dtype=torch.uint8, device="cuda", generator=g)
inp = rand(rank + 1, n)                                   # this rank's gather block
blocks = [rand(100 + q, n) for q in range(P)]              # the scatter root's inputs (every rank can model them)
g_out = torch.zeros(P * n if rank == root else 1, dtype=torch.uint8, device="cuda")
ag_out = torch.zeros(P * n, dtype=torch.uint8, device="cuda")
s_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
b_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
tmp = torch.zeros(n, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ctx = gloo_amd.Context(rank, P, store, device=0, timeout_ms=60000)
def gather():
    gloo_amd.gather(ctx, inp.data_ptr(), n, "u8", root, output=g_out.data_ptr() if rank == root else None)
def allgather():
    gloo_amd.allgather(ctx, ag_out.data_ptr(), n, "u8", input=inp.data_ptr())
def scatter():
    gloo_amd.scatter(ctx, s_out.data_ptr(), n, "u8", root,
                     inputs=[b.data_ptr() for b in blocks] if rank == root else None)
def bcasts():
    for q in range(P):
        dst = b_out if q == rank else tmp
        gloo_amd.broadcast(ctx, dst.data_ptr(), n, "u8", root, input=blocks[q].data_ptr() if rank == root else None,
                           tag=1 + q)
forms = {"gather": gather, "allgather": allgather, "scatter": scatter, "bcasts": bcasts}
for f in forms.values():
    f()
torch.cuda.synchronize()
want = torch.cat([rand(q + 1, n) for q in range(P)])
assert torch.equal(ag_out, want), "allgather"
if rank == root:
    assert torch.equal(g_out, want), "gather"
assert torch.equal(s_out, blocks[rank]), "scatter"
assert torch.equal(b_out, blocks[rank]), "broadcasts"
for _ in range(warmup):
    for f in forms.values():
        f()
res = {k: [] for k in forms}
for _ in range(rounds):
    for k, f in forms.items():
        t = time.perf_counter()
        for _ in range(reps):
            f()
        res[k].append(1e6 * (time.perf_counter() - t) / reps)
print(json.dumps({"rank": rank, **{k + "_us": [round(v, 1) for v in vs] for k, vs in res.items()}}), flush=True)
ctx.close()
'''


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ranks", type=int, default=4)
    p.add_argument("--elems", type=int, default=16 << 20)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    args = p.parse_args()
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(WORKER)
        env = dict(os.environ, GLOO_AMD_ROOT=ROOT)
        procs = [subprocess.Popen([sys.executable, "-u", w, str(r), str(args.ranks), "file:" + os.path.join(d, "s"),
                                   str(args.elems), str(args.reps), str(args.warmup), str(args.rounds)], env=env,
                                  stdout=subprocess.PIPE, text=True) for r in range(args.ranks)]
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
    summary = {"ranks": args.ranks, "elems_per_block": args.elems, "reps": args.reps, "rounds": args.rounds}
    mean = {}
    for k in FORMS:
        per_round = [sum(r[k + "_us"][i] for r in rows) / len(rows) for i in range(args.rounds)]
        mean[k] = sum(per_round) / len(per_round)
        summary[k + "_us"] = [round(v, 1) for v in per_round]
        summary[k + "_spread"] = round((max(per_round) - min(per_round)) / mean[k], 4)
    summary["allgather_over_gather"] = round(mean["allgather"] / mean["gather"], 3)
    summary["bcasts_over_scatter"] = round(mean["bcasts"] / mean["scatter"], 3)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
