"""GPU: GLOO_HIP_SUM_WIDE on the plan interpreter (reduce.hip plan_interp_wide_kernel,
interp_fold_wide).  A FOLD step of k >= 3 sources is the f32 model of
tests/test_sum_wide_gpu.py (numpy float32 adds in list order, narrowed once), at
the interpreter's own pass sizes; k <= 2 is SUM; and a SUM_WIDE collective between
rank processes runs on the sliced interpreter and rounds once.  (Its one-launch form
measured slower than the eager plan and stays off for the op, DESIGN.md §2 "Wide sum":
at the one-launch size the same cases assert that, and the same bytes.)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fold_model as fm
import fp8_model
import interp_model as im
import sum_wide_worker

pytestmark = pytest.mark.gpu

from test_fp8_gpu import from_dev, to_dev, torch  # noqa: E402,F401  (the module's torch fixture)
from test_sum_wide_gpu import DTYPES, model, narrow, sources, widen  # noqa: E402


def run_fold(torch, op, dtype, srcs, mode, G=1, alias=None):
    """One FOLD step: dst one element past a 16-B boundary (or source `alias` itself, moved there),
    source j at residue (5 j + 1) % 16.  Sources and the bytes around dst must stay."""
    import gloo_amd
    es, n = fm.itemsize(dtype), srcs[0].size
    soff = [es if j == alias else (5 * j + 1) % 16 // es * es for j in range(len(srcs))]
    dev = [to_dev(torch, s.view(np.uint8), o) for s, o in zip(srcs, soff)]
    out = dev[alias][0] if alias is not None else to_dev(torch, np.zeros(n * es, np.uint8), es)[0]
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    step = gloo_amd.interp_step(gloo_amd.INTERP_FOLD, dst=out.data_ptr() + es, src=[p for _, p in dev], n=n, mode=mode)
    gloo_amd.interp_kernel(op, dtype, [step], err.data_ptr(), slices=G)
    assert int(err.item()) == 0
    for j, ((t, _), s, o) in enumerate(zip(dev, srcs, soff)):
        assert j == alias or (from_dev(torch, t, o, n * es) == s.view(np.uint8)).all(), "a source was modified"
        assert not t[:o].any() and not t[o + n * es:].any(), "wrote outside a buffer"
    assert not out[:es].any() and not out[es + n * es:].any(), "wrote outside the chunk"
    return from_dev(torch, out, es, n * es).view(srcs[0].dtype)


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_fold_step_is_the_f32_model(torch, dtype, k, mode):
    es = fm.itemsize(dtype)
    kV, F = 16 // es, im.fp_bytes(es) // es
    for n in (5, F + kV + 3, 2 * F + kV + 3, F):
        srcs = sources(dtype, k, n)
        want = model(torch, dtype, srcs)
        assert (want != fm.fold("sum", dtype, srcs, 0)).any()  # not the step-rounded SUM
        same(run_fold(torch, "sum_wide", dtype, srcs, mode), want, (n,))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_sources_are_sum(torch, dtype, k):
    es = fm.itemsize(dtype)
    srcs = fm.inputs("sum", dtype, k, im.fp_bytes(es) // es + 16 // es + 3, np.random.default_rng([3, k]))
    same(run_fold(torch, "sum_wide", dtype, srcs, 0), run_fold(torch, "sum", dtype, srcs, 0), k)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("alias", [0, 3])
@pytest.mark.parametrize("dtype", ["bf16", "f8e4m3"])
def test_in_place_and_sliced(torch, dtype, alias, G):
    """dst is src[0] (how the executor folds into output 0) or src[k - 1], on G workgroups:
    every slice's result is the model's."""
    es = fm.itemsize(dtype)
    for n in (3 * G * (16 // es) + 1, 2 * im.fp_bytes(es) // es + 1):
        srcs = [s[:n].copy() for s in sources(dtype, 4, max(n, 1005))]  # (sources() plants at 1000 from n = 100 on)
        want = model(torch, dtype, srcs)
        assert (want != fm.fold("sum", dtype, srcs, 0)).any()
        same(run_fold(torch, "sum_wide", dtype, srcs, 0, G=G, alias=alias), want, (n,))


# ---- the collective, between rank processes --------------------------------

RUNS, N = 3, 12_289
MESH = [dict(algo=a, dtype=d, n=N, k=1, draw="ints" if d == "bf16" else "small", seed=5, runs=RUNS)
        for a in ("ring_chunked", "halving_doubling") for d in ("bf16", "f8e4m3")]
# the knob tests/mode_matrix.py reaches its `sliced` cells with; three pointers at P = 2: the wide pass is the LOCAL_REDUCE
SLICED = {"GLOO_AMD_INTERP_SLICE_BYTES": "1024"}
GROUPS = {"one_launch": (4, {}, MESH), "sliced": (4, SLICED, MESH),
          "local": (2, SLICED, [dict(algo="halving_doubling", dtype="bf16", n=N, k=3, draw="normal", seed=6, runs=RUNS)])}
_results, _dead = {}, []


def group(name):
    """(outs [rank][runs, k, n], modes [rank][run]) per job of the group, run once by P
    sum_wide_worker.py processes, each under its own time limit.  After a child that died of a
    signal or a time limit nothing more is started."""
    if name not in _results:
        assert not _dead, f"not started: {_dead[0]}"
        P, env, jobs = GROUPS[name]
        with tempfile.TemporaryDirectory() as d:
            jf = os.path.join(d, "jobs.json")
            with open(jf, "w") as f:
                json.dump(jobs, f)
            cmd = ["timeout", "-k", "10", str(30 + 10 * len(jobs)), sys.executable, sum_wide_worker.__file__]
            procs = [subprocess.Popen(cmd + [str(r), str(P), d, jf], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT) for r in range(P)]
            logs = [p.communicate()[0].decode()[-1500:] for p in procs]
            rcs = [p.returncode for p in procs]
            if any(rc < 0 or rc >= 124 for rc in rcs):
                _dead.append(f"group {name}: worker exits {rcs}: {logs}")
            assert not _dead, _dead[0]
            errs = [open(os.path.join(d, f)).read()[-1500:] for f in sorted(os.listdir(d)) if f.startswith("e")]
            assert rcs == [0] * P and not errs, (rcs, errs, logs)
            _results[name] = [([np.load(os.path.join(d, f"o{r}_{j}.npy")) for r in range(P)],
                               [json.load(open(os.path.join(d, f"m{r}_{j}.json"))) for r in range(P)])
                              for j in range(len(jobs))]
    return _results[name]


@pytest.mark.parametrize("j", range(len(MESH)), ids=[f"{m['algo']}-{m['dtype']}" for m in MESH])
@pytest.mark.parametrize("form", ["one_launch", "sliced"])
def test_mesh_plans_run_on_the_interpreter_and_round_once(torch, monkeypatch, form, j):
    """P = 4 rank processes, one pointer, three runs on one algorithm object; all f32 partial sums
    are exact for these inputs, so every run is the float64 sum of its inputs converted once, on
    every rank (the construction of test_sum_wide_gpu.py test_mesh_plans_round_once)."""
    import plan_sim
    job, P = MESH[j], 4
    dtype, x = job["dtype"], sum_wide_worker.draw(job, P)
    if dtype != "bf16":
        monkeypatch.setattr(plan_sim, "oracle", fp8_model.ModelOracle)
    want, wants = x[:, 0], []
    for _ in range(RUNS):
        want = [narrow(torch, dtype, sum(widen(torch, dtype, w).astype(np.float64) for w in want))] * P
        wants.append(want[0])
    assert np.isfinite(widen(torch, dtype, wants[-1])).all()
    assert (wants[-1] != plan_sim.simulate(job["algo"], "sum", dtype, x, runs=RUNS)[0, 0]).any()
    outs, modes = group(form)[j]
    for r in range(P):
        assert all(m["interp"] == (m["interp_slices"] > 1) == (form == "sliced") for m in modes[r]), (r, modes[r])
        for run in range(RUNS):
            same(outs[r][run, 0], wants[run], (r, run))


def test_local_reduce_is_the_wide_pass(torch):
    """P = 2, three pointers: each rank's LOCAL_REDUCE is one wide pass, the exchange a
    two-source SUM; the expected value is composed pass by pass."""
    job, P = GROUPS["local"][2][0], 2
    outs, modes = group("local")[0]
    cur = sum_wide_worker.draw(job, P)
    for run in range(RUNS):
        local = [model(torch, "bf16", list(cur[r])) for r in range(P)]
        # (from the second run on a rank's pointers are equal, and v + v + v rounds once either way)
        assert run or all((local[r] != fm.fold("sum", "bf16", list(cur[r]), 0)).any() for r in range(P))
        want = fm.fold("sum", "bf16", local, 0)
        for r in range(P):
            assert modes[r][run]["interp"] and modes[r][run]["interp_slices"] > 1, (r, modes[r])
            for q in range(job["k"]):
                same(outs[r][run, q], want, (r, run, q))
        cur = np.broadcast_to(want, cur.shape)
