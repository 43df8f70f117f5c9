"""One rank of a batch of pipelined halving-doubling jobs — test
infrastructure of tests/test_hd_pipelined_gpu.py, following sched_worker.py.

run_rank() is the rank body; main() runs it as one rank process ("file:"
store, argv: RANK P DIR JOBS_JSON) or as P rank threads of one child process
("mem:" store, argv: threads P DIR JOBS_JSON), so the test process itself
never holds the GPU while rank processes run.  A job
is {algo, op, dtype, k, n, runs, offsets}: k pointers of n elements, pointer j
starting offsets[j] elements into its allocation.  Every job is a fresh
algorithm on the rank's context, run `runs` times back to back with the
inputs of make_inputs() loaded before each run.  Device memory comes from
tests/hip_rt.py, so a process starts quickly.
"""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NPT = {"f32": np.float32, "bf16": np.uint16, "i32": np.int32}


def make_inputs(op, dtype, P, k, n, run):
    """[P][k][n] inputs of run `run`: the run-0 values scaled by 2^run (sum,
    max, min), so a value left over from another run cannot pass for this
    run's.  Products keep their inputs (small integers, wrapping)."""
    rng = np.random.default_rng(P * 1009 + k * 101 + n)
    if dtype == "f32":
        x = rng.integers(-64, 65, (P, k, n)).astype(np.float32) / 8
        return x * np.float32(2.0 ** run) if op != "product" else x
    if dtype == "bf16":  # finite positive patterns; + 0x80 doubles the value
        x = rng.integers(0x3C00, 0x4200, (P, k, n)).astype(np.uint16)
        return x + np.uint16(0x80 * run) if op != "product" else x
    x = rng.integers(-3, 4, (P, k, n)).astype(np.int32)
    return x * (1 << run) if op != "product" else x


def run_rank(rank, P, url, jobs, device=0, timeout_ms=60000):
    """-> per job {"outs": [runs][k][n], "modes": [runs]} or {"err": text}."""
    import gloo_amd
    import hip_rt
    hip_rt.set_device(device)
    ctx = gloo_amd.Context(rank, P, url, device=device, timeout_ms=timeout_ms)
    res = []
    for job in jobs:
        try:
            op, dtype, k, n = job["op"], job["dtype"], job["k"], job["n"]
            es = np.dtype(NPT[dtype]).itemsize
            offs = job.get("offsets") or [0] * k
            raw = [hip_rt.malloc((n + offs[j]) * es + 64) for j in range(k)]
            ptrs = [raw[j] + offs[j] * es for j in range(k)]
            a = gloo_amd.Algorithm(ctx, job["algo"], op, dtype, ptrs, n)
            outs, modes = [], []
            for run in range(job["runs"]):
                x = make_inputs(op, dtype, P, k, n, run)[rank]
                for j in range(k):
                    if n:
                        hip_rt.h2d(ptrs[j], x[j])
                a.run()
                modes.append(a.mode())
                outs.append(np.array([hip_rt.d2h(ptrs[j], x[j]) if n else x[j] for j in range(k)]))
            a.close()
            for p in raw:
                hip_rt.free(p)
            res.append({"outs": np.array(outs), "modes": modes})
        except Exception:  # noqa: BLE001 — recorded for the test of this job
            res.append({"err": traceback.format_exc()})
            break  # the peers' next collective would only time out
    ctx.close()
    return res


def save(d, rank, res):
    for j, r in enumerate(res):
        if "err" in r:
            with open(os.path.join(d, f"e{rank}_{j}.txt"), "w") as f:
                f.write(r["err"])
            continue
        np.save(os.path.join(d, f"o{rank}_{j}.npy"), r["outs"])
        with open(os.path.join(d, f"m{rank}_{j}.json"), "w") as f:
            json.dump(r["modes"], f)


def main():
    """argv: RANK P DIR JOBS_JSON (one rank process, "file:" store), or
    threads P DIR JOBS_JSON (all P ranks as threads of this process, "mem:"
    store: they share the GPU inside one process and wait on the host)."""
    P, d = int(sys.argv[2]), sys.argv[3]
    jobs = json.loads(open(sys.argv[4]).read())
    if sys.argv[1] != "threads":
        rank = int(sys.argv[1])
        return save(d, rank, run_rank(rank, P, "file:" + os.path.join(d, "store"), jobs))
    import threading
    import uuid
    url = "mem:" + uuid.uuid4().hex

    def body(r):
        try:
            save(d, r, run_rank(r, P, url, jobs))
        except Exception:  # noqa: BLE001
            with open(os.path.join(d, f"e{r}_0.txt"), "w") as f:
                f.write(traceback.format_exc())

    ts = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()


if __name__ == "__main__":
    main()
