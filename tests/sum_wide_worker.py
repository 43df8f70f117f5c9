"""One rank of a batch of SUM_WIDE allreduce jobs (tests/test_sum_wide_interp_gpu.py)
— test infrastructure.  argv: RANK P DIR JOBS_JSON.  A job is {algo, dtype, n,
k, draw, seed, runs}: a fresh context (store file:DIR/s<j>, timeout 20 s) and one
algorithm object over k pointers, run `runs` times (each run reduces the
previous run's outputs); it saves every pointer after every run (o<rank>_<j>.npy,
[runs, k, n]) and the mode of every run (m<rank>_<j>.json), or the error
(e<rank>_<j>.txt).  Device memory comes from tests/hip_rt.py, not torch."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def draw(job, P):
    """[P, k, n] storage values.  ints: bf16 integers in [-256, 256]; small: e4m3
    up to 2.0 (both: every f32 partial sum is exact); normal: bf16 normal values."""
    import fp8_model
    rng, shape = np.random.default_rng(job["seed"]), (P, job["k"], job["n"])
    if job["draw"] == "small":
        return fp8_model.draw_small(rng, job["dtype"], shape, bound=2.0)
    f = rng.integers(-256, 257, shape) if job["draw"] == "ints" else rng.standard_normal(shape)
    return (f.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def main():
    import gloo_amd
    import hip_rt
    rank, P, d, jobs = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], json.loads(open(sys.argv[4]).read())
    hip_rt.set_device(0)
    for j, job in enumerate(jobs):
        try:
            x = draw(job, P)[rank]
            bufs = [hip_rt.malloc(xi.nbytes) for xi in x]
            for b, xi in zip(bufs, x):
                hip_rt.h2d(b, xi)
            ctx = gloo_amd.Context(rank, P, "file:" + os.path.join(d, f"s{j}"), device=0, timeout_ms=20000)
            a = gloo_amd.Algorithm(ctx, job["algo"], "sum_wide", job["dtype"], bufs, job["n"])
            outs, modes = [], []
            for _ in range(job["runs"]):
                a.run()
                modes.append(a.mode())
                outs.append([hip_rt.d2h(b, xi) for b, xi in zip(bufs, x)])
            a.close()
            ctx.close()
            for b in bufs:
                hip_rt.free(b)
            np.save(os.path.join(d, f"o{rank}_{j}.npy"), np.array(outs))
            with open(os.path.join(d, f"m{rank}_{j}.json"), "w") as f:
                json.dump(modes, f)
        except Exception:  # noqa: BLE001 — recorded for the test of this job
            with open(os.path.join(d, f"e{rank}_{j}.txt"), "w") as f:
                f.write(traceback.format_exc())


if __name__ == "__main__":
    main()
