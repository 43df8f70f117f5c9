"""GPU: the broadcast collective (GLOO_HIP_ALGO_BROADCAST, CudaBroadcastOneToAll's
twin) through the executor's launch modes and both interfaces.

The model is closed form: after a run every pointer of every rank holds, byte
for byte, what the root's root pointer held.  Every case runs three times
with a different payload per run; non-root buffers start as a sentinel; guard
bytes in front of and behind every pointer must stay untouched; float
payloads carry NaN bit patterns and -0.  The ranks check their own buffers
(tests/broadcast_worker.py) and report; this process never holds the GPU.

Rank threads ("mem:" store) share the GPU inside one process and wait on the
host: the plan's own steps.  Rank processes ("file:" store) signal on the
device: the root's one-pass fan-out (fanout_kernel), the receive + broadcast
pass, hipGraph replay, the one-launch interpreter and its sliced form.

Shapes (u8 unless said): 0, 1, 15, 16, 17 (the head / tail byte path of the
16-byte packets), 16383, 16384, 16385 (one 16 KiB tile +- 1), 4 MiB + 3 (an
eager enqueue with kernel copies, more than one pass of a capped grid: 256
workgroups x 16 KiB), and 4099 elements of f32, f64 and one FP8 dtype.
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
WORKER = os.path.join(ROOT, "tests", "broadcast_worker.py")
RUNS = 3
U8_COUNTS = (0, 1, 15, 16, 17, 16383, 16384, 16385)
BIG = (4 << 20) + 3
POINTERS = ((1, 0), (3, 0), (3, 2))  # (k, root pointer)


@pytest.fixture(scope="module")
def gpu():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def job(dtype, n, k, rp, root, **kw):
    return dict(kind="algo", dtype=dtype, n=n, k=k, rp=rp, root=root, runs=RUNS, **kw)


def grid(P, big):
    """The shapes x roots 0 and P - 1 x (k, root pointer)."""
    jobs = [job("u8", n, k, rp, root) for n in U8_COUNTS for root in (0, P - 1) for k, rp in POINTERS]
    jobs += [job(dt, 4099, k, rp, root) for dt in ("f32", "f64", "f8e4m3")
             for root, (k, rp) in ((0, (3, 2)), (P - 1, (1, 0)))]
    if big:
        jobs += [job("u8", BIG, 3, 2, P - 1), job("u8", BIG, 1, 0, 0)]
    return jobs


def run_workers(P, env, jobs, threads=False, limit=150):
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


@pytest.mark.parametrize("P", [2, 3, 8])
def test_rank_threads(gpu, P):
    jobs = grid(P, big=P == 2)
    reports = run_workers(P, {}, jobs, threads=True)
    check(jobs, reports, P)
    for r in range(P):
        for jb, res in zip(jobs, reports[r]):
            if jb["n"]:  # (an empty plan has no peer, so nothing makes it wait on the host)
                assert not any(m["device_signal"] or m["graph"] or m["interp"] for m in res["modes"]), (jb, res)


# the launch modes, selected as tests/mode_matrix.py selects them
MODES = {
    "eager": {"GLOO_AMD_INTERP": "0", "GLOO_AMD_GRAPH": "0"},
    "graph": {"GLOO_AMD_INTERP": "0", "GLOO_AMD_GRAPH": "1"},
    "interp": {},
    "sliced": {"GLOO_AMD_INTERP_SLICE_BYTES": "1024"},
}


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("mode", list(MODES))
def test_rank_processes_launch_modes(gpu, mode, P):
    jobs = grid(P, big=P == 2 and mode in ("eager", "graph"))
    reports = run_workers(P, MODES[mode], jobs)
    check(jobs, reports, P)
    for j, jb in enumerate(jobs):
        if jb["n"] == 0:
            continue  # an empty plan launches nothing
        nbytes = jb["n"] * {"u8": 1, "f32": 4, "f64": 8, "f8e4m3": 1}[jb["dtype"]]
        for r in range(P):
            modes = reports[r][j]["modes"]
            what = (mode, jb, "rank", r, modes)
            assert all(m["device_signal"] and m["own_stream"] and m["fine_arena"] == (r != jb["root"])
                       for m in modes), what
            if mode == "eager":
                assert not any(m["graph"] or m["interp"] for m in modes), what
            elif mode == "graph":
                assert not modes[0]["graph"] and all(m["graph"] for m in modes[1:]), what
            elif mode == "interp":  # every message within the one-launch limit (64 KiB)
                assert all(m["interp"] and not m["graph"] for m in modes), what
            else:  # one workgroup per KiB of the message
                assert all(m["interp"] for m in modes), what
                assert all((m["interp_slices"] > 1) == (nbytes > 1024) for m in modes), what


@pytest.fixture(scope="module")
def interfaces(gpu):
    """One set of two rank processes for the workspace, stream, profiling and
    function-style cases."""
    jobs = [
        job("u8", 16385, 3, 2, 1, ws="host"),                       # 0: CudaHostWorkspace's instantiation
        job("f32", 4099, 3, 2, 0, streams=True),                    # 1: one stream per pointer
        job("u8", 16385, 1, 0, 1, caller_stream=True),              # 2: the caller's stream
        job("f32", 4099, 3, 0, 0, profile=1),                       # 3: event profiling
        job("f32", 4099, 3, 0, 1, profile=2),                       # 4: device stamps
        dict(kind="func", dtype="f32", n=4099, root=0, runs=RUNS),  # 5: the output is the input
        dict(kind="func", dtype="f32", n=4099, root=0, runs=RUNS, separate_input=True),  # 6: cached schedule of 5
        dict(kind="func", dtype="u8", n=16385, root=1, runs=RUNS, separate_input=True, caller_stream=True, tag=7),
        dict(kind="func", dtype="u8", n=BIG, root=1, runs=2),
    ]
    reports = run_workers(2, {}, jobs)
    check(jobs, reports, 2)
    return jobs, reports


def test_host_workspace(interfaces):
    _, reports = interfaces
    for r in range(2):
        assert all(m["host_arena"] for m in reports[r][0]["modes"])


def test_per_pointer_streams_and_caller_stream(interfaces):
    _, reports = interfaces
    for r in range(2):
        assert not any(m["own_stream"] for m in reports[r][1]["modes"])
        assert not any(m["own_stream"] for m in reports[r][2]["modes"])


@pytest.mark.parametrize("j", [3, 4])
def test_stats_report_no_reductions(interfaces, j):
    """Copies are not counted as reductions: stats[1] and stats[2] are 0."""
    _, reports = interfaces
    for r in range(2):
        st = reports[r][j]["stats"]
        assert st["reductions"] == 0 and st["reduce_bytes"] == 0, st


def test_function_style(interfaces):
    """gloo_amd.broadcast with and without a separate root input, called
    repeatedly with different payloads on one cached schedule (jobs 5 and 6
    share theirs), Context.last_mode() readable after each call."""
    _, reports = interfaces
    for r in range(2):
        for j in (5, 6, 7, 8):
            modes = reports[r][j]["modes"]
            assert modes and all(m["device_signal"] for m in modes), (j, modes)
        assert all(m["own_stream"] for m in reports[r][5]["modes"])
        assert not any(m["own_stream"] for m in reports[r][7]["modes"])
