"""GPU: the gather and scatter collectives (GLOO_HIP_ALGO_GATHER, gloo::gather /
gloo::gatherv; GLOO_HIP_ALGO_SCATTER, gloo::scatter) through the executor's
launch modes and both interfaces.

The models are closed form: a gather root's output is block 0 ... block P-1
back to back; a scatter leaves the root's input q in rank q's output.  Every
case runs three times with a different payload per run; every rank compares
its WHOLE output every run (outputs start as a sentinel, so a stale inbox read
shows), a gather rank that is not the root passes a sentinel-filled output
that must stay untouched, inputs must come back unmodified, and guard bytes in
front of and behind every buffer must keep their fill.  The ranks check their
own buffers (tests/gather_scatter_worker.py) and report; this process never
holds the GPU.

Rank threads ("mem:" store) share the GPU inside one process and wait on the
host: the plan's own steps, at P = 2, 3, 8 and 9.  Rank processes ("file:"
store) signal on the device: the roots' multi-copy launches, hipGraph replay,
the one-launch interpreter and its sliced form at P = 2 and 4; and, enqueued
and replayed, at P = 8, where a scatter root's 7 sends and own block (and a
gather root's own block and 7 copy-outs) fill the 8-entry copy batch exactly,
and at P = 9, where they cross it into a second launch.

Blocks of 0, 1, 5 and 16 KiB + 3 elements of u8 and f64 (around one 16-byte
packet and one 16 KiB tile), every buffer at its own misalignment; gatherv
with one empty and one odd-sized block; a rotating root; the in-place forms
(a gather root's input is its slot of the output, a scatter root's output is
its own input), which keep the plan's COPY step beside the root's launch.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gather_scatter_worker.py")
RUNS = 3
TILE3 = (16 << 10) + 3
SIZES = (0, 1, 5, TILE3)
ES = {"u8": 1, "f64": 8}


@pytest.fixture(scope="module")
def gpu():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def job(coll, dtype, n, root, kind="algo", **kw):
    return dict(coll=coll, kind=kind, dtype=dtype, n=n, root=root, runs=RUNS, **kw)


def ragged(P, odd_at):
    """One odd-sized block (16 KiB + 3, at rank odd_at), one empty (the next rank), small ones elsewhere."""
    c = [3 + q for q in range(P)]
    c[odd_at] = TILE3
    c[(odd_at + 1) % P] = 0
    return c


def grid(P, small=False):
    """Both collectives x the block sizes x u8 and f64, the root moving from
    job to job; the two gatherv forms; a root that rotates from run to run."""
    jobs = []
    for coll in ("gather", "scatter"):
        for dt in ("u8", "f64"):
            for n in ((0, 5, TILE3) if small else SIZES):
                if small and dt == "f64" and n != TILE3:
                    continue
                jobs.append(job(coll, dt, n, len(jobs) % P))
    jobs.append(dict(job("gather", "u8", 0, P - 1), counts=ragged(P, 0)))
    jobs.append(dict(job("gather", "f64", 0, 0), counts=ragged(P, P - 1)))
    jobs.append(job("gather", "u8", 5, 1, kind="func", rotate=True))
    jobs.append(job("scatter", "f64", 5, 0, kind="func", rotate=True))
    return jobs


def run_workers(P, env, jobs, threads=False, limit=60):
    """Every worker under its own time limit; the first worker that fails or
    reports an error ends the case (the others are stopped, nothing more is
    started).  -> reports[rank][job]."""
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


def check(jobs, reports, P):
    for r in range(P):
        for j, res in enumerate(reports[r]):
            assert "err" not in res, (jobs[j], "rank", r, res["err"])
        assert len(reports[r]) == len(jobs), ("rank", r, "stopped after job", len(reports[r]))


def plain(jb):
    """An even-form algorithm job with bytes to move: every rank has steps."""
    return jb["kind"] == "algo" and "counts" not in jb and jb["n"] > 0


@pytest.mark.parametrize("P", [2, 3, 8, 9])
def test_rank_threads(gpu, P):
    jobs = grid(P, small=P > 3)
    reports = run_workers(P, {}, jobs, threads=True)
    check(jobs, reports, P)
    for r in range(P):
        for jb, res in zip(jobs, reports[r]):
            if plain(jb):  # (a rank without steps has no peer, so nothing makes it wait on the host)
                assert not any(m["device_signal"] or m["graph"] or m["interp"] for m in res["modes"]), (jb, res)


# the launch modes, selected as tests/mode_matrix.py selects them
MODES = {
    "eager": {"GLOO_AMD_INTERP": "0", "GLOO_AMD_GRAPH": "0"},
    "graph": {"GLOO_AMD_INTERP": "0", "GLOO_AMD_GRAPH": "1"},
    "interp": {},
    "sliced": {"GLOO_AMD_INTERP_SLICE_BYTES": "1024"},
}
INTERP_BYTES = 64 << 10  # the one-launch limit; with 1 KiB slices also the most a sliced plan's message may be


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


def batch_grid(P):
    """Blocks above the fused-launch size, so that with device signalling both
    roots take their multi-copy launches; roots at both ends and inside."""
    return [
        job("gather", "u8", 4 * TILE3, 0),
        job("gather", "f64", TILE3, P - 1),
        job("scatter", "u8", 4 * TILE3, P // 2),
        job("scatter", "f64", TILE3, 0),
        job("scatter", "u8", 5, P - 1),
        dict(job("gather", "u8", 0, 1), counts=ragged(P, 2)),
    ]


@pytest.mark.parametrize("P", [8, 9])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_rank_processes_fill_and_cross_the_copy_batch(gpu, mode, P):
    jobs = batch_grid(P)
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


@pytest.fixture(scope="module")
def interfaces(gpu):
    """One set of two rank processes for the workspace, stream, profiling and
    function-style cases."""
    jobs = [
        job("gather", "u8", TILE3, 1, ws="host"),                          # 0, 1: CudaHostWorkspace's placement
        job("scatter", "f64", TILE3, 0, ws="host"),
        job("gather", "f64", 5, 0, caller_stream=True),                    # 2, 3: the caller's stream
        job("scatter", "u8", TILE3, 1, caller_stream=True),
        job("gather", "u8", TILE3, 0, profile=1),                          # 4, 5: event profiling, the plan's own steps
        job("scatter", "u8", TILE3, 1, profile=1),
        job("gather", "f64", TILE3, 1, kind="func"),                       # 6, 7: one cached schedule, three calls
        job("scatter", "f64", TILE3, 0, kind="func"),
        dict(job("gather", "u8", 0, 0, kind="func", tag=7, caller_stream=True), counts=[5, TILE3]),  # 8: gatherv
        job("scatter", "u8", 1, 1, kind="func", tag=7, caller_stream=True),                       # 9
        job("gather", "u8", 4 * TILE3, 1, alias=True),                     # 10-13: in place, enqueued then replayed
        job("scatter", "f64", TILE3, 0, alias=True),
        job("gather", "f64", 5, 0, kind="func", alias=True),
        job("scatter", "u8", 4 * TILE3, 1, kind="func", alias=True),
    ]
    reports = run_workers(2, {}, jobs)
    check(jobs, reports, 2)
    return jobs, reports


def test_host_workspace(interfaces):
    """The rank that receives (the gather's root, the scatter's other rank) keeps its inboxes in host memory."""
    _, reports = interfaces
    assert all(m["host_arena"] for m in reports[1][0]["modes"])
    assert all(m["host_arena"] for m in reports[1][1]["modes"])


def test_caller_stream(interfaces):
    _, reports = interfaces
    for r in range(2):
        for j in (2, 3, 8, 9):
            assert not any(m.get("own_stream", False) for m in reports[r][j]["modes"]), (r, j)


@pytest.mark.parametrize("j", [4, 5])
def test_stats_report_no_reductions(interfaces, j):
    """Copies are not counted as reductions."""
    _, reports = interfaces
    for r in range(2):
        st = reports[r][j]["stats"]
        assert st["reductions"] == 0 and st["reduce_bytes"] == 0, st


def test_function_style(interfaces):
    """gloo_amd.gather / gloo_amd.scatter called repeatedly with different
    payloads on one cached schedule, Context.last_mode() readable after each."""
    _, reports = interfaces
    for r in range(2):
        for j in (6, 7, 9):
            modes = reports[r][j]["modes"]
            assert modes and all(m["device_signal"] for m in modes), (j, modes)
        assert all(m["own_stream"] for m in reports[r][6]["modes"])
