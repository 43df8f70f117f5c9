"""GPU: the allgather collective (GLOO_HIP_ALGO_ALLGATHER; AllgatherRing,
gloo::allgather and gloo::allgatherv) through the executor's launch modes and
both interfaces.

The model is closed form: rank r contributes k inputs of counts[r] elements;
after a run every rank's output holds every rank's inputs, in rank order, byte
for byte.  Every case runs three times with a different payload per run; the
output starts as a sentinel (in place: but for the rank's own slot); guard
bytes in front of and behind the output and the inputs must stay untouched
and the inputs unmodified; float payloads carry NaN bit patterns and -0.  The
ranks check their own buffers (tests/allgather_worker.py) and report; this
process never holds the GPU.

Rank threads ("mem:" store) share the GPU inside one process and wait on the
host: the plan's own steps.  Rank processes ("file:" store) signal on the
device: the sender's one pass over its inputs (gather_fanout_kernel; in place
fanout_kernel), hipGraph replay, the one-launch interpreter and its sliced
form.

Shapes (u8 per-input counts): 0, 1, 15, 16, 17 (the head / tail byte path of
the 16-byte packets), 16383, 16384, 16385 (one 16 KiB tile +- 1), each with 1
and 3 inputs and in place; 4099 elements of f32, f64 and one FP8 dtype; per P
one allgatherv with a zero-count rank and ragged counts; 4 MiB + 3 per input
at two ranks (an eager enqueue with kernel copies, more than one pass of a
capped grid: 256 workgroups x 16 KiB).
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
WORKER = os.path.join(ROOT, "tests", "allgather_worker.py")
RUNS = 3
U8_COUNTS = (0, 1, 15, 16, 17, 16383, 16384, 16385)
BIG = (4 << 20) + 3
INPUTS = (1, 3, 0)  # k; 0 = in place
ES = {"u8": 1, "f32": 4, "f64": 8, "f8e4m3": 1}
RAGGED = {2: [0, 4099], 3: [17, 0, 16385], 4: [0, 16385, 1, 4099], 8: [3, 0, 1, 0, 17, 0, 16385, 5]}


@pytest.fixture(scope="module")
def gpu():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


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


# the launch modes, selected as tests/mode_matrix.py selects them
MODES = {
    "eager": {"GLOO_AMD_INTERP": "0", "GLOO_AMD_GRAPH": "0"},
    "graph": {"GLOO_AMD_INTERP": "0", "GLOO_AMD_GRAPH": "1"},
    "interp": {},
    "sliced": {"GLOO_AMD_INTERP_SLICE_BYTES": "1024"},
}


def job(dtype, n, k, **kw):
    return dict(kind="algo", dtype=dtype, n=n, k=k, runs=RUNS, **kw)


def grid(P, big):
    jobs = [job("u8", n, k) for n in U8_COUNTS for k in INPUTS]
    # (every block within the one-launch interpreter's 64 KiB)
    jobs += [job("f32", 4099, 3), job("f64", 4099, 1), job("f8e4m3", 4099, 0)]
    jobs += [dict(kind="func", dtype="u8", n=0, k=1, counts=RAGGED[P], runs=RUNS)]
    if big:
        jobs += [job("u8", BIG, 3), job("u8", BIG, 0)]
    return jobs


def block_bytes(jb, r, P):
    """Bytes of rank r's block, and of the largest block."""
    counts = jb.get("counts") or [jb["n"]] * P
    per = max(1, jb["k"]) * ES[jb["dtype"]]
    return counts[r] * per, max(counts) * per


@pytest.mark.parametrize("P", [2, 3, 8])
def test_rank_threads(gpu, P):
    jobs = grid(P, big=P == 2)
    reports = run_workers(P, {}, jobs, threads=True)
    check(jobs, reports, P)
    for r in range(P):
        for jb, res in zip(jobs, reports[r]):
            if block_bytes(jb, r, P)[1]:  # (an empty plan has no peer, so nothing makes it wait on the host)
                assert not any(m["device_signal"] or m["graph"] or m["interp"] for m in res["modes"]), (jb, res)


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("mode", list(MODES))
def test_rank_processes_launch_modes(gpu, mode, P):
    jobs = grid(P, big=P == 2 and mode in ("eager", "graph"))
    reports = run_workers(P, MODES[mode], jobs)
    check(jobs, reports, P)
    for j, jb in enumerate(jobs):
        if block_bytes(jb, 0, P)[1] == 0:
            continue  # an empty plan launches nothing
        counts = jb.get("counts") or [jb["n"]] * P
        for r in range(P):
            modes = reports[r][j]["modes"]
            what = (mode, jb, "rank", r, modes)
            receives = any(counts[q] for q in range(P) if q != r)
            assert all(m["device_signal"] and m["own_stream"] and m["fine_arena"] == receives for m in modes), what
            if mode == "eager":
                assert not any(m["graph"] or m["interp"] for m in modes), what
            elif mode == "graph":
                assert not modes[0]["graph"] and all(m["graph"] for m in modes[1:]), what
            elif mode == "interp":  # every message within the one-launch limit (64 KiB)
                assert all(m["interp"] and not m["graph"] for m in modes), what
            elif "counts" not in jb:
                # One workgroup per KiB of the block with one input or in place.  With three inputs the
                # plan is not sliceable (the SEND reads a range the LOCAL_GATHER wrote in three pieces):
                # it runs as one interpreter launch, every block being within that launch's limit.
                assert all(m["interp"] for m in modes), what
                sliced = jb["k"] <= 1 and block_bytes(jb, r, P)[1] > 1024
                assert all((m["interp_slices"] > 1) == sliced for m in modes), what


@pytest.fixture(scope="module")
def interfaces(gpu):
    """One set of two rank processes for the workspace, stream and
    function-style cases."""
    jobs = [
        job("u8", 16385, 3, ws="host"),                                              # 0: CudaHostWorkspace's placement
        job("f32", 4099, 1, caller_stream=True),                                     # 1: the caller's stream
        dict(kind="func", dtype="f32", n=4099, k=1, runs=RUNS),                      # 2: three calls, one schedule
        dict(kind="func", dtype="f32", n=4099, k=1, runs=RUNS),                      # 3: the cached schedule of 2
        dict(kind="func", dtype="f32", n=4099, k=1, counts=[5, 4099], runs=RUNS),    # 4: other counts
        dict(kind="func", dtype="u8", n=7, k=0, counts=[16385, 0], runs=RUNS, caller_stream=True, tag=7),
        dict(kind="func", dtype="u8", n=BIG, k=1, runs=2),
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
        assert not any(m["own_stream"] for m in reports[r][1]["modes"])


def test_function_style(interfaces):
    """gloo_amd.allgather with equal counts (twice: the second job hits the
    first one's cached schedule), with per-rank counts, in place on the
    caller's stream, and at 4 MiB + 3; Context.last_mode() readable after
    each call."""
    _, reports = interfaces
    for r in range(2):
        for j in (2, 3, 4, 5, 6):
            modes = reports[r][j]["modes"]
            assert modes and all(m["device_signal"] for m in modes), (j, modes)
        assert all(m["own_stream"] for m in reports[r][2]["modes"])
        assert not any(m["own_stream"] for m in reports[r][5]["modes"])
