"""One rank of a batch of broadcast jobs — test infrastructure of
tests/test_broadcast_gpu.py, following hd_pipelined_worker.py.

main() runs run_rank() as one rank process ("file:" store, argv: RANK P DIR
JOBS_JSON) or as P rank threads of one child process ("mem:" store, argv:
threads P DIR JOBS_JSON).  A broadcast's model is closed form, so every rank
checks its own buffers and writes a report (r<rank>.json): per job either
{"err": text} or {"modes": [...], "stats": {...}, "last_mode": {...}}.

A job: {kind: "algo" | "func", dtype, n, k, root, rp, runs, ws, streams,
caller_stream, separate_input, profile}.  Pointer j of rank r starts
offset(r, j) elements past a 256-byte boundary (0, 1 or 2, so source and
destinations differ in their 16-byte misalignment), with GUARD bytes in front
of it and behind its n elements.  Before every run the root's root pointer
gets the run's payload and every other byte a sentinel; after it every
pointer must hold the payload, byte for byte, and every guard its fill.
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

ES = {"u8": 1, "f32": 4, "f64": 8, "f8e4m3": 1, "f8e5m2": 1}
GUARD, SENTINEL, FILL = 64, 0xEE, 0xA5
# NaN bit patterns (quiet and signalling, both signs, with payloads) and -0
SPECIAL = {
    "f32": np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000], np.uint32).view(np.uint8),
    "f64": np.array([0x7FF8000000000001, 0xFFF0000000000123, 0x8000000000000000], np.uint64).view(np.uint8),
    "f8e4m3": np.array([0x7F, 0xFF, 0x80], np.uint8),
    "f8e5m2": np.array([0x7D, 0xFE, 0xFF, 0x80], np.uint8),
    "u8": np.array([], np.uint8),
}


def payload(job_index, job, run):
    """The bytes the root's root pointer holds before run `run`: different for
    every run and job, never the sentinel, the float specials in front."""
    nbytes = job["n"] * ES[job["dtype"]]
    rng = np.random.default_rng(1000 * job_index + run + 1)
    b = rng.integers(0, 256, nbytes, dtype=np.uint8)
    b[b == SENTINEL] = run
    sp = SPECIAL[job["dtype"]]
    m = min(len(sp), nbytes) // ES[job["dtype"]] * ES[job["dtype"]]
    b[:m] = sp[:m]
    return b


def offset(rank, j):
    return (rank + j) % 3


def run_rank(rank, P, url, jobs, device=0, timeout_ms=60000):
    import gloo_amd
    import hip_rt
    hip_rt.set_device(device)
    ctx = gloo_amd.Context(rank, P, url, device=device, timeout_ms=timeout_ms)
    res = []
    for ji, job in enumerate(jobs):
        try:
            dtype, n, root = job["dtype"], job["n"], job["root"]
            func = job["kind"] == "func"
            es = ES[dtype]
            nbytes = n * es
            # function style: pointer 0 is the output; the root may have a separate input (pointer 1)
            k = (2 if job.get("separate_input") and rank == root else 1) if func else job["k"]
            rp = (1 if k == 2 else 0) if func else job["rp"]
            raw = [hip_rt.malloc(256 + 2 * es + nbytes + GUARD) for _ in range(k)]
            ptrs = [raw[j] + 256 + offset(rank, j) * es for j in range(k)]
            streams = [hip_rt.stream_create() for _ in range(k)] if job.get("streams") else None
            stream = hip_rt.stream_create() if job.get("caller_stream") else 0
            a = None
            if not func:
                # `op` is not used: the pair the reductions refuse
                a = gloo_amd.Algorithm(ctx, "broadcast", "bxor" if dtype != "u8" else 0, dtype, ptrs, n,
                                       root=root, root_pointer=rp, workspace=job.get("ws", "device"),
                                       stream=stream, streams=streams)
                if job.get("profile"):
                    a.set_profiling(job["profile"])
            modes, stats = [], None
            for run in range(job["runs"]):
                want = payload(ji, job, run)
                for j in range(k):
                    img = np.full(GUARD + nbytes + GUARD, FILL, np.uint8)
                    img[GUARD:GUARD + nbytes] = want if (rank == root and j == rp) else SENTINEL
                    hip_rt.h2d(ptrs[j] - GUARD, img)
                if func:
                    gloo_amd.broadcast(ctx, ptrs[0], n, dtype, root, input=ptrs[1] if k == 2 else None,
                                       tag=job.get("tag", 0), stream=stream)
                    modes.append(ctx.last_mode() if n else {})
                else:
                    a.run()
                    modes.append(a.mode())
                for s in (streams or []) + ([stream] if stream else []):
                    hip_rt.stream_synchronize(s)
                if a is not None and job.get("profile"):
                    stats = a.stats()
                for j in range(k):
                    got = hip_rt.d2h(ptrs[j] - GUARD, np.empty(GUARD + nbytes + GUARD, np.uint8))
                    bad = np.flatnonzero(got[GUARD:GUARD + nbytes] != want)
                    assert bad.size == 0, f"run {run} pointer {j}: byte {bad[0]} of {nbytes} is " \
                                          f"{got[GUARD + bad[0]]:#x}, want {want[bad[0]]:#x} ({bad.size} differ)"
                    assert (got[:GUARD] == FILL).all(), f"run {run} pointer {j}: bytes in front were written"
                    assert (got[GUARD + nbytes:] == FILL).all(), f"run {run} pointer {j}: guard behind was written"
            if a is not None:
                a.close()
            for s in (streams or []) + ([stream] if stream else []):
                hip_rt.stream_destroy(s)
            for p in raw:
                hip_rt.free(p)
            res.append({"modes": modes, "stats": stats})
        except Exception:  # noqa: BLE001 — recorded for the test of this job
            res.append({"err": traceback.format_exc()[-1500:]})
            break  # the peers' next collective would only time out
    ctx.close()
    return res


def save(d, rank, res):
    with open(os.path.join(d, f"r{rank}.json.tmp"), "w") as f:
        json.dump(res, f)
    os.replace(os.path.join(d, f"r{rank}.json.tmp"), os.path.join(d, f"r{rank}.json"))


def main():
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
            save(d, r, [{"err": traceback.format_exc()[-1500:]}])

    ts = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()


if __name__ == "__main__":
    main()
