"""GPU: the pipelined halving-doubling (GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED,
pipelineBroadcastAndReduce of gloo/cuda_allreduce_halving_doubling.cc) on the
executor, byte for byte against the CPU simulation of the PLAIN plan with the
oracle reduction: the product never computes its own expectation.

Every case runs three times back to back with inputs scaled by 2^run, so a
stale inbox or a range broadcast before it was finished shows.

Rank threads on the "mem:" store (of one child process, so that this
process never holds the GPU) share one GPU and wait on the host (executor.h),
which runs the plan's own steps: the sub-range local reduces and broadcasts,
and none of the fused passes.  The launch modes with device signalling (eager
with the three fused passes, hipGraph replay, the one-launch interpreter with
its multi-destination step) need one process per rank: the same grid runs
there on rank processes on the "file:" store, one worker set per (mode, P)
running all its jobs (tests/hd_pipelined_worker.py).
"""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import plan_sim
from hd_pipelined_worker import make_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "hd_pipelined_worker.py")
HDP = "halving_doubling_pipelined"
PAIRS = [("sum", "f32"), ("max", "bf16"), ("product", "i32")]
KS = (2, 4, 8, 9)   # copy-kernel broadcast; every fusion; receive-reduce unfused (k + 1 > 8); chained fold
NS = (1, 1000, 100_003)
RUNS = 3


@pytest.fixture(scope="module")
def gpu():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@functools.lru_cache(maxsize=None)
def expected(op, dtype, P, k, n, run):
    """[P][k][n]: the plain plan simulated on the CPU with the oracle."""
    return plan_sim.simulate("halving_doubling", op, dtype, make_inputs(op, dtype, P, k, n, run), seed=run)


def job(op, dtype, k, n, algo=HDP, offsets=None):
    return {"algo": algo, "op": op, "dtype": dtype, "k": k, "n": n, "runs": RUNS, "offsets": offsets}


def check(jobs, results, P):
    """results[rank][job]; every run of every pointer of every rank."""
    for r in range(P):
        for j, res in enumerate(results[r]):
            assert "err" not in res, (jobs[j], r, res["err"])
    for j, jb in enumerate(jobs):
        for run in range(RUNS):
            want = expected(jb["op"], jb["dtype"], P, jb["k"], jb["n"], run)
            for r in range(P):
                got = results[r][j]["outs"][run]
                assert got.shape == want[r].shape
                bad = np.argwhere(got.view(np.uint8) != want[r].view(np.uint8))
                assert bad.size == 0, (jb, "rank", r, "run", run, "first differing (pointer, byte)", bad[0])


def run_threads(P, jobs):
    """All P ranks as threads of ONE child process on the "mem:" store."""
    return run_processes(P, {}, jobs, threads=True)


@pytest.mark.parametrize("P", [2, 3, 4, 6, 8])
@pytest.mark.parametrize("op,dtype", PAIRS)
def test_threads_match_plain_simulation(gpu, op, dtype, P):
    jobs = [job(op, dtype, k, n) for k in KS for n in NS]
    check(jobs, run_threads(P, jobs), P)


@pytest.mark.parametrize("dtype,op", [("f32", "sum"), ("bf16", "max")])
def test_threads_misaligned_pointers(gpu, dtype, op):
    """Each pointer starts at another element offset of its allocation, so
    the broadcast stores to destinations of different 16-byte misalignment."""
    jobs = [job(op, dtype, 4, n, offsets=[0, 1, 3, 5]) for n in (1000, 100_003)]
    check(jobs, run_threads(4, jobs), 4)


# ---- launch modes: rank processes (device signalling) ----------------------

MODES = {
    "eager": {"GLOO_AMD_GRAPH": "0", "GLOO_AMD_INTERP": "0"},
    "graph": {"GLOO_AMD_GRAPH": "1"},
    "interp": {"GLOO_AMD_INTERP": "1"},
}


def mode_jobs(mode, P):
    # the whole grid: the fused passes and the multi-destination step run only here
    jobs = [job(op, dtype, k, n) for op, dtype in PAIRS for k in KS for n in NS]
    # destinations of different 16-byte misalignment (the multi-destination step in interpreter mode)
    jobs += [job("sum", "f32", 4, 1000, offsets=[0, 1, 3, 5]), job("max", "bf16", 4, 1000, offsets=[0, 1, 3, 5]),
             job("sum", "f32", 9, 1000, offsets=[1, 0, 2, 3, 0, 1, 2, 3, 1])]
    # the default algorithm's LOCAL_BCAST shares the multi-destination lowering
    jobs += [job("sum", "f32", 4, 1000, algo="halving_doubling")]
    if P == 2:  # even halves: the plan may run sliced (one workgroup per 32 KiB of the largest message)
        jobs += [job("sum", "f32", 4, 65536)]
    return jobs


def run_processes(P, env, jobs, threads=False):
    with tempfile.TemporaryDirectory() as d:
        jf = os.path.join(d, "jobs.json")
        with open(jf, "w") as f:
            json.dump(jobs, f)
        e = dict(os.environ, **env)
        who = ["threads"] if threads else [str(r) for r in range(P)]
        logs = [open(os.path.join(d, f"log{w}.txt"), "w") for w in who]
        procs = [subprocess.Popen([sys.executable, WORKER, w, str(P), d, jf], env=e, stdout=log,
                                  stderr=subprocess.STDOUT) for w, log in zip(who, logs)]
        try:
            rcs = [p.wait(timeout=240) for p in procs]
        except subprocess.TimeoutExpired:
            for p in procs:
                p.kill()
            for p in procs:
                p.wait()
            rcs = [p.returncode for p in procs]
        for f in logs:
            f.close()
        tails = [open(os.path.join(d, f"log{w}.txt")).read()[-2000:] for w in who] * (P if threads else 1)
        rcs = rcs * (P if threads else 1)
        out = []
        for r in range(P):
            res = []
            for j in range(len(jobs)):
                ef, of = os.path.join(d, f"e{r}_{j}.txt"), os.path.join(d, f"o{r}_{j}.npy")
                if os.path.exists(ef):
                    res.append({"err": open(ef).read()[-1500:]})
                elif not os.path.exists(of):
                    res.append({"err": f"no output (worker exit {rcs[r]}): {tails[r]}"})
                else:
                    res.append({"outs": np.load(of), "modes": json.load(open(os.path.join(d, f"m{r}_{j}.json")))})
            out.append(res)
        return out


def in_block_of_one(rank, P):
    off = P
    for b in (1 << i for i in range(P.bit_length())):
        if P & b:
            off -= b
            if off <= rank:
                return b == 1


@pytest.mark.parametrize("P", [2, 3, 4, 6, 8])
@pytest.mark.parametrize("mode", list(MODES))
def test_processes_launch_modes(gpu, mode, P):
    """Eager (the three fused passes), hipGraph replay and the interpreter
    (multi-destination steps) give the plain plan's bytes, and
    gloo_hip_algorithm_mode reports the forced mode, over the same grid as
    the thread cases (three dtype / op pairs x k x n at every P).  P = 4,
    k = 4, n = 100 003 is among the jobs of every mode."""
    jobs = mode_jobs(mode, P)
    results = run_processes(P, MODES[mode], jobs)
    check(jobs, results, P)
    for j, jb in enumerate(jobs):
        msg_bytes = jb["n"] * (2 if jb["dtype"] == "bf16" else 4)
        for r in range(P):
            m = results[r][j]["modes"][-1]
            what = (mode, jb, "rank", r, m)
            assert m["device_signal"], what
            if mode == "eager":
                assert not m["graph"] and not m["interp"], what
                # the local fold rides with the first send wherever the rank pipelines
                if jb["algo"] == HDP and jb["k"] == 4 and jb["n"] >= 1000 and not in_block_of_one(r, P):
                    assert m["fold_send"], what
            elif mode == "graph":
                assert m["graph"] and not m["interp"], what
            elif msg_bytes <= 64 << 10 or jb["n"] == 65536:
                # every step within the one-launch limit (GLOO_AMD_FUSE_BYTES), or sliced
                assert m["interp"] and not m["graph"], what
                if jb["n"] == 65536:
                    assert m["interp_slices"] > 1, what
