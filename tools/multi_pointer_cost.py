"""MEASUREMENT: what pipelineBroadcastAndReduce could hide (VERDICT r5
"missing" 3).

The reference's CudaAllreduceHalvingDoubling with several device pointers per
rank can pipeline its local reduce and broadcast with the exchange
(pipelineBroadcastAndReduce, gloo/cuda_allreduce_halving_doubling.cc:253-279,
376-394).  The plain algorithm runs the local parts as one fused pass each (a
k-source left fold before the exchange, a broadcast after it).  The most a
pipeline could save is the time of those local passes, so the first leg times
the same halving-doubling allreduce (fp32 sum, n elements per pointer, P rank
processes on the box's GPU) with k = 1 pointer and with k pointers per rank:
(t_k - t_1) / t_k bounds the pipeline's gain.

    python tools/multi_pointer_cost.py RANK P STORE_DIR N K ITERS
(launched by tools/multi_pointer_cost.sh); rank 0 prints one JSON line.

--pipelined leg (a 7th argument, then optionally the number of alternations,
default 7): the plain algorithm and "halving_doubling_pipelined" with K
pointers, both alive in one session over the same buffers, timed in
alternation (ITERS calls each per alternation, the p50 of each block).  Run it
with GLOO_AMD_MESH=0, so that the plain algorithm stays on the reference's
route like the pipelined one.  Rank 0 prints one JSON line per alternation and
a summary line (median and range of the block p50s, their ratio).  Before the
timing both run once on the same rank-dependent inputs and every pointer's
bytes are compared.  On one GPU the local passes share HBM with the exchange,
so this shows the bytes the fused passes save, not any overlap."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import gloo_amd  # noqa: E402
import hip_rt  # noqa: E402


def pipelined_leg(ctx, rank, P, n, K, iters, alternations):
    algos = ("halving_doubling", "halving_doubling_pipelined")
    bufs = [hip_rt.malloc(4 * n) for _ in range(K)]
    a = {name: gloo_amd.Algorithm(ctx, name, "sum", "f32", bufs, n) for name in algos}
    barrier = gloo_amd.Algorithm(ctx, "halving_doubling", "sum", "f32", [hip_rt.malloc(64)], 1)
    # same inputs through both: the bytes of every pointer must agree
    rng = np.random.default_rng(rank)
    xs = [rng.integers(-64, 65, n).astype(np.float32) for _ in range(K)]
    got = {}
    for name in algos:
        for b, x in zip(bufs, xs):
            hip_rt.h2d(b, x)
        a[name].run()
        got[name] = [hip_rt.d2h(b, xs[0]) for b in bufs]
    same = all((p.view(np.uint32) == q.view(np.uint32)).all() for p, q in zip(got[algos[0]], got[algos[1]]))
    zero = np.zeros(n, np.float32)  # timed runs reduce their own outputs: zeros stay finite
    for b in bufs:
        hip_rt.h2d(b, zero)
    for name in algos:
        for _ in range(3):
            a[name].run()
    p50 = {name: [] for name in algos}
    for alt in range(alternations):
        line = {"P": P, "n_per_pointer": n, "K": K, "iters": iters, "alternation": alt,
                "mesh": os.environ.get("GLOO_AMD_MESH", "")}
        for name in algos:
            ts = []
            for _ in range(iters):
                barrier.run()  # line the ranks up
                t0 = time.perf_counter()
                a[name].run()
                ts.append(time.perf_counter() - t0)
            ts.sort()
            p50[name].append(ts[len(ts) // 2] * 1e6)
            line[name + "_us_p50"] = round(p50[name][-1], 1)
        if rank == 0:
            print(json.dumps(line), flush=True)
    out = {"P": P, "n_per_pointer": n, "K": K, "iters": iters, "alternations": alternations, "same_bytes": bool(same),
           "mesh": os.environ.get("GLOO_AMD_MESH", ""), "modes": {name: a[name].mode() for name in algos}}
    for name in algos:
        v = sorted(p50[name])
        out[name] = {"us_median": round(v[len(v) // 2], 1), "us_min": round(v[0], 1), "us_max": round(v[-1], 1)}
    out["pipelined_over_plain"] = round(out[algos[1]]["us_median"] / out[algos[0]]["us_median"], 4)
    if rank == 0:
        print(json.dumps(out), flush=True)
    barrier.close()
    for name in algos:
        a[name].close()
    for b in bufs:
        hip_rt.free(b)
    ctx.close()


def main():
    rank, P, d, n, K, iters = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]),
                               int(sys.argv[5]), int(sys.argv[6]))
    hip_rt.set_device(0)
    ctx = gloo_amd.Context(rank, P, "file:" + d, device=0, timeout_ms=60000)
    if len(sys.argv) > 7 and sys.argv[7] == "--pipelined":
        return pipelined_leg(ctx, rank, P, n, K, iters, int(sys.argv[8]) if len(sys.argv) > 8 else 7)
    out = {"P": P, "n_per_pointer": n, "iters": iters}
    x = np.full(n, 1.0, np.float32)
    for k in (1, K):
        bufs = [hip_rt.malloc(4 * n) for _ in range(k)]
        for b in bufs:
            hip_rt.h2d(b, x)
        a = gloo_amd.Algorithm(ctx, "halving_doubling", "sum", "f32", bufs, n)
        for _ in range(3):
            a.run()
        ctx_barrier = gloo_amd.Algorithm(ctx, "halving_doubling", "sum", "f32", [bufs[0]], 1)
        ts = []
        for _ in range(iters):
            ctx_barrier.run()  # line the ranks up
            t0 = time.perf_counter()
            a.run()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        out["k%d_us_p50" % k] = round(ts[len(ts) // 2] * 1e6, 1)
        y = hip_rt.d2h(bufs[-1], x)
        out["k%d_finite" % k] = bool(np.isfinite(y).all())
        ctx_barrier.close()
        a.close()
        for b in bufs:
            hip_rt.free(b)
    out["K"] = K
    out["local_share_bound"] = round((out["k%d_us_p50" % K] - out["k1_us_p50"]) / out["k%d_us_p50" % K], 4)
    ctx.close()
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
