"""GPU: the alltoall collective (GLOO_HIP_ALGO_ALLTOALL, gloo::alltoall /
gloo::alltoallv) through the executor's launch modes and both interfaces.

The model is closed form: block q of rank r's output is block r of rank q's
input, out_r[outOff_r[q], +M[q][r]) == in_q[inOff_q[r], +M[q][r]).  Every case
does three runs back to back with no barrier and a fresh payload each run (so
the previous-run credits matter); every rank compares its WHOLE output bit for
bit every run (outputs start as a sentinel, so a stale inbox read shows), its
input must come back unmodified, and guard bytes in front of and behind every
buffer must keep their fill.  The ranks check their own buffers
(tests/alltoall_worker.py) and report; this process never holds the GPU.

Shapes: u8 blocks of 0, 1, 15, 16, 17 and 4097 bytes, so that blocks start at
odd byte offsets and straddle one 16-byte packet; one block just above 64 KiB
(the fused-small and one-launch limit); one of 1 MiB; f16, f32 and f64 once
each (only the element size matters).

Rank threads ("mem:" store) share the GPU inside one process and wait on the
host: the plan's own steps.  Rank processes ("file:" store) signal on the
device: the two multi-copy launches, hipGraph replay, the one-launch
interpreter and its sliced form at P = 2 and 4, even and ragged; and, enqueued
and replayed, at P = 8, where the 7 sends and the own block fill the 8-entry
copy batch exactly, and at P = 9, where they cross it into a second launch.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import pytest

from test_gather_scatter_gpu import INTERP_BYTES, MODES, check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "alltoall_worker.py")
RUNS = 3
SMALL = (0, 1, 15, 16, 17, 4097)
OVER_FUSE = (64 << 10) + 1
MIB = 1 << 20
ES = {"u8": 1, "f16": 2, "f32": 4, "f64": 8}
LIMIT = 40  # seconds: the cap of one case


def run_workers(P, env, jobs, threads=False, limit=LIMIT):
    """As test_gather_scatter_gpu.run_workers, over this module's worker: every
    worker under the case's time limit; the first worker that fails or reports
    an error ends the case (the others are stopped, nothing more is started).
    -> reports[rank][job]."""
    with tempfile.TemporaryDirectory() as d:
        jf = os.path.join(d, "jobs.json")
        with open(jf, "w") as f:
            json.dump(jobs, f)
        e = dict(os.environ, **env)
        who = ["threads"] if threads else [str(r) for r in range(P)]
        logs = [open(os.path.join(d, f"log{w}.txt"), "w") for w in who]
        procs = [subprocess.Popen([sys.executable, WORKER, w, str(P), d, jf], env=e, stdout=log,
                                  stderr=subprocess.STDOUT) for w, log in zip(who, logs)]
        deadline = time.monotonic() + limit
        failed = None
        while failed is None and any(p.poll() is None for p in procs):
            try:
                next(p for p in procs if p.poll() is None).wait(timeout=0.2)
            except subprocess.TimeoutExpired:
                pass
            for w, p in zip(who, procs):
                if p.poll() not in (None, 0):
                    failed = f"worker {w} exited with {p.returncode}"
            if failed is None and time.monotonic() > deadline:
                failed = f"a worker ran past its {limit} s limit"
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        for f in logs:
            f.close()
        tails = {w: open(os.path.join(d, f"log{w}.txt")).read()[-1500:] for w in who}
        reports = []
        for r in range(P):
            rf = os.path.join(d, f"r{r}.json")
            w = "threads" if threads else str(r)
            assert os.path.exists(rf), (failed, "rank", r, tails[w])
            reports.append(json.load(open(rf)))
        assert failed is None, (failed, tails)
        return reports


@pytest.fixture(scope="module")
def gpu():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def even(dtype, n, kind="algo", **kw):
    return dict(kind=kind, form="even", dtype=dtype, n=n, runs=RUNS, **kw)


def ragged(P, sizes, shift=0, kind="algo", form="matrix", dtype="u8", **kw):
    """M[q][r] walks `sizes` from `shift`, so every row and column mixes them,
    blocks start at odd offsets and, with a 0 among the sizes, some are empty."""
    m = [sizes[(q * P + r + shift) % len(sizes)] for q in range(P) for r in range(P)]
    return dict(kind=kind, form=form, dtype=dtype, matrix=m, runs=RUNS, **kw)


def grid(P, big=True):
    jobs = [even("u8", n) for n in SMALL]
    jobs += [even("f16", 15), even("f32", 17), even("f64", 4097)]
    jobs += [ragged(P, SMALL), ragged(P, SMALL, shift=3)]
    if big:
        jobs += [even("u8", OVER_FUSE), ragged(P, (17, OVER_FUSE, 0, 4097, MIB), shift=1)]
    return jobs


def plain(jb):
    """An even-form algorithm job with bytes to move: every rank has steps, all of one size."""
    return jb["kind"] == "algo" and jb["form"] == "even" and jb["n"] > 0


@pytest.mark.parametrize("P", [2, 3, 4])
def test_rank_threads(gpu, P):
    jobs = grid(P)
    reports = run_workers(P, {}, jobs, threads=True)
    check(jobs, reports, P)
    for r in range(P):
        for jb, res in zip(jobs, reports[r]):
            if plain(jb):
                assert not any(m["device_signal"] or m["graph"] or m["interp"] for m in res["modes"]), (jb, res)


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("mode", list(MODES))
def test_rank_processes_launch_modes(gpu, mode, P):
    jobs = grid(P)
    reports = run_workers(P, MODES[mode], jobs)
    check(jobs, reports, P)
    for j, jb in enumerate(jobs):
        if not plain(jb):
            continue
        nbytes = jb["n"] * ES[jb["dtype"]]
        for r in range(P):
            modes = reports[r][j]["modes"]
            what = (mode, jb, "rank", r, modes)
            assert all(m["device_signal"] and m["own_stream"] for m in modes), what
            if mode == "eager":
                assert not any(m["graph"] or m["interp"] for m in modes), what
            elif mode == "graph":
                assert not modes[0]["graph"] and all(m["graph"] for m in modes[1:]), what
            elif nbytes <= INTERP_BYTES:
                assert all(m["interp"] and not m["graph"] for m in modes), what
                if mode == "sliced":  # one workgroup per KiB of the block
                    assert all((m["interp_slices"] > 1) == (nbytes > 1024) for m in modes), what


@pytest.mark.parametrize("P", [8, 9])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_rank_processes_fill_and_cross_the_copy_batch(gpu, mode, P):
    """Blocks above the fused-launch size, so that every rank takes its
    multi-copy launches: 7 sends + the own block at P = 8, 8 + 1 at P = 9."""
    jobs = [even("u8", OVER_FUSE), even("f64", 4097), even("u8", 17),
            ragged(P, (OVER_FUSE, 17, 0, 4097, 1, 15, 16), shift=2)]
    reports = run_workers(P, MODES[mode], jobs)
    check(jobs, reports, P)
    for j, jb in enumerate(jobs):
        if not plain(jb):
            continue
        for r in range(P):
            modes = reports[r][j]["modes"]
            what = (mode, jb, "rank", r, modes)
            assert all(m["device_signal"] for m in modes), what
            if mode == "eager":
                assert not any(m["graph"] or m["interp"] for m in modes), what
            else:
                assert not modes[0]["graph"] and all(m["graph"] for m in modes[1:]), what


M2 = [3, OVER_FUSE, 17, 5]  # P = 2: rank 0 sends 3 to itself and 64 KiB + 1 to rank 1; rank 1 sends 17 and 5


@pytest.fixture(scope="module")
def interfaces(gpu):
    """One set of two rank processes for the workspace, stream, profiling and function-style cases."""
    jobs = [
        even("u8", OVER_FUSE, ws="host"),                                   # 0: CudaHostWorkspace's placement
        ragged(2, SMALL, shift=1, caller_stream=True),                      # 1: the caller's stream
        even("u8", OVER_FUSE, profile=1),                                   # 2: event profiling, the plan's own steps
        even("f32", 4097, kind="func"),                                     # 3: one cached schedule, three calls
        dict(kind="func", form="matrix", dtype="u8", matrix=M2, runs=RUNS, tag=7),   # 4, 5: the same M both ways
        dict(kind="func", form="lists", dtype="u8", matrix=M2, runs=RUNS, tag=7),
        dict(kind="func", form="lists", dtype="f16", matrix=[0, 0, 0, 0], runs=RUNS),  # 6: nothing to move
        dict(kind="func", form="lists", dtype="u8", matrix=[1, 15, 16, 17], runs=RUNS, caller_stream=True),  # 7
    ]
    reports = run_workers(2, {}, jobs)
    check(jobs, reports, 2)
    return jobs, reports


def test_host_workspace(interfaces):
    _, reports = interfaces
    for r in range(2):
        assert all(m["host_arena"] for m in reports[r][0]["modes"])


def test_caller_stream(interfaces):
    _, reports = interfaces
    for r in range(2):
        for j in (1, 7):
            assert not any(m.get("own_stream", False) for m in reports[r][j]["modes"]), (r, j)


def test_stats_report_no_reductions(interfaces):
    """Copies are not counted as reductions."""
    _, reports = interfaces
    for r in range(2):
        st = reports[r][2]["stats"]
        assert st["reductions"] == 0 and st["reduce_bytes"] == 0, st


def test_function_style_three_forms(interfaces):
    """gloo_amd.alltoall called repeatedly with different payloads in the even,
    the matrix and the own-lists form; the last two at the same M give the same
    bytes (each is compared with the one closed-form model) on one schedule's
    launch mode; Context.last_mode() is readable after each call."""
    _, reports = interfaces
    for r in range(2):
        for j in (3, 4, 5):
            modes = reports[r][j]["modes"]
            assert modes and all(m["device_signal"] and m["own_stream"] for m in modes), (j, modes)
        assert reports[r][4]["modes"] == reports[r][5]["modes"]
        assert reports[r][6]["modes"] == [{}] * RUNS


def test_own_lists_hit_and_miss_alike(gpu):
    """P = 4, own-lists form: M1, then M2 that differs from M1 only in
    M[0][1] (ranks 2 and 3 pass the lists they passed before), then M1 again.
    Every rank must miss, miss and hit together; each call completes and is
    correct inside the case's limit."""
    P = 4
    m1 = ragged(P, SMALL, shift=2)["matrix"]
    m2 = list(m1)
    m2[0 * P + 1] += 4097
    for q in (2, 3):  # the premise: ranks 2 and 3 cannot tell M2 from M1 by their own lists
        assert [m1[q * P + r] for r in range(P)] == [m2[q * P + r] for r in range(P)]
        assert [m1[r * P + q] for r in range(P)] == [m2[r * P + q] for r in range(P)]
    jobs = [dict(kind="func", form="lists", dtype="u8", seq=[m1, m2, m1], runs=3)]
    reports = run_workers(P, {}, jobs)
    check(jobs, reports, P)


def test_own_lists_disagreement_is_refused_on_both_ranks(gpu):
    """Rank 0 says it sends 5 to rank 1, rank 1 expects 6 from rank 0: both
    raise, naming the pair and both values, both outputs keep their sentinel,
    and correct calls on the same context then succeed."""
    bad = {"0": [[2, 5], [2, 3]], "1": [[3, 4], [6, 4]]}
    jobs = [dict(kind="func", form="lists", dtype="u8", matrix=[2, 5, 3, 4], runs=RUNS, bad_lists=bad,
                 expect=["rank 0 sends 5 elements to rank 1", "rank 1 expects 6 from rank 0"])]
    reports = run_workers(2, {}, jobs)
    check(jobs, reports, 2)
    assert reports[0][0]["refused"] and reports[0][0]["refused"] == reports[1][0]["refused"]


def test_another_matrix_on_one_rank_fails_the_construction_everywhere(gpu):
    """The algorithm-object form: rank 1 passes another matrix.  The call-hash
    guard refuses the construction on every rank, no byte moves, and a
    construction with one matrix then works."""
    P = 3
    m = ragged(P, SMALL, shift=4)["matrix"]
    other = list(m)
    other[0 * P + 2] += 1
    jobs = [dict(kind="algo", form="matrix", dtype="u8", matrix=m, runs=RUNS, bad_matrix={"1": other},
                 expect=["rank-inconsistent collective", "rank 1 was called with another"])]
    reports = run_workers(P, {}, jobs)
    check(jobs, reports, P)
