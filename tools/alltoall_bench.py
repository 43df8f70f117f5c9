#!/usr/bin/env python3
"""Alltoall beside the P scatters that emulate it, and the own-lists form
beside the matrix form (developer tool, after tools/gather_scatter_bench.py).

P rank processes on GPU 0, `--elems` u8 per block.  Every rank times
  alltoall   one gloo_amd.alltoall, even form,
  scatters   the P gloo_amd.scatter calls that emulate it (root q scatters the
             P blocks of its input, rank r keeping block q of its output),
  matrix     one gloo_amd.alltoall with the P x P matrix given (every block
             `--elems`, so the same bytes as the even form),
  lists      the same call with this rank's in_counts / out_counts only: it
             exchanges the counts on the host in EVERY call, then runs the
             matrix form's cached schedule; lists - matrix is that exchange,
in `--rounds` alternating rounds of `--reps` calls each (after `--warmup` of
each), on the same build and in the same processes.  Calls run on the
library's own stream and return with the output complete, so the host clock
covers the device work; the figure per round is the mean over the ranks of
each rank's mean time per call.  Every form is checked against its model once
before the timing.  Prints one JSON line per rank and a summary with the
rounds' values, their median and their spread ((max - min) / mean).
  python tools/alltoall_bench.py [--ranks 4] [--elems 16777216] [--reps 20] [--rounds 3]
All ranks share one GPU: nothing here goes over xGMI.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("alltoall", "scatters", "matrix", "lists")

WORKER = r'''
import json, os, sys, time
sys.path.insert(0, os.environ["GLOO_AMD_ROOT"])
import torch, gloo_amd
rank, P, store, n, reps, warmup, rounds = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], *map(int, sys.argv[4:8])
torch.cuda.set_device(0)
def rand(seed, m):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (m,), dtype=torch.uint8, device="cuda", generator=g)
inp = rand(rank + 1, P * n)                                # block r goes to rank r
outs = {k: torch.zeros(P * n, dtype=torch.uint8, device="cuda") for k in ("alltoall", "scatters", "matrix", "lists")}
torch.cuda.synchronize()
ctx = gloo_amd.Context(rank, P, store, device=0, timeout_ms=60000)
M = [[n] * P for _ in range(P)]
def alltoall():
    gloo_amd.alltoall(ctx, inp.data_ptr(), outs["alltoall"].data_ptr(), n, "u8")
def scatters():
    o = outs["scatters"].data_ptr()
    for q in range(P):
        gloo_amd.scatter(ctx, o + q * n, n, "u8", q,
                         inputs=[inp.data_ptr() + r * n for r in range(P)] if rank == q else None, tag=1 + q)
def matrix():
    gloo_amd.alltoall(ctx, inp.data_ptr(), outs["matrix"].data_ptr(), 0, "u8", matrix=M, tag=1)
def lists():
    gloo_amd.alltoall(ctx, inp.data_ptr(), outs["lists"].data_ptr(), 0, "u8", in_counts=[n] * P, out_counts=[n] * P,
                      tag=1)
forms = {"alltoall": alltoall, "scatters": scatters, "matrix": matrix, "lists": lists}
for f in forms.values():
    f()
torch.cuda.synchronize()
want = torch.cat([rand(q + 1, P * n)[rank * n:(rank + 1) * n] for q in range(P)])
for k, o in outs.items():
    assert torch.equal(o, want), k
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
        summary[k + "_median_us"] = round(statistics.median(per_round), 1)
        summary[k + "_spread"] = round((max(per_round) - min(per_round)) / mean[k], 4)
    summary["scatters_over_alltoall"] = round(mean["scatters"] / mean["alltoall"], 3)
    summary["lists_minus_matrix_us"] = round(mean["lists"] - mean["matrix"], 1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
