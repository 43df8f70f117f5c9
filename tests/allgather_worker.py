"""One rank of a batch of allgather jobs — test infrastructure of
tests/test_allgather_gpu.py, following broadcast_worker.py.

main() runs run_rank() as one rank process ("file:" store, argv: RANK P DIR
JOBS_JSON) or as P rank threads of one child process ("mem:" store, argv:
threads P DIR JOBS_JSON).  An allgather's model is closed form, so every rank
checks its own output and writes a report (r<rank>.json): per job either
{"err": text} or {"modes": [...]}.

A job: {kind: "algo" | "func", dtype, n, k, counts, runs, ws, caller_stream,
tag}.  k inputs per rank (0: in place) of n elements each, or of counts[rank]
(function style, k <= 1).  The output and every input start 0, 1 or 2
elements past a 256-byte boundary (so sources, the own slot and the peers'
inboxes differ in their 16-byte misalignment), with GUARD bytes in front and
behind.  Before every run the inputs get the run's payload of this rank (in
place: the rank's own slot of the output does) and every other byte of the
output a sentinel; after it the output must hold every rank's payload in rank
order, byte for byte, every guard its fill, and the inputs their payload.
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

from broadcast_worker import ES, FILL, GUARD, SENTINEL, SPECIAL, save  # noqa: E402


def payload(job_index, job, run, rank, i, count):
    """Input i of `rank` in run `run`: different for every run, job, rank and
    input, never the sentinel, the float specials in front."""
    es = ES[job["dtype"]]
    rng = np.random.default_rng(100000 * job_index + 1000 * run + 10 * rank + i + 1)
    b = rng.integers(0, 256, count * es, dtype=np.uint8)
    b[b == SENTINEL] = run
    sp = SPECIAL[job["dtype"]]
    m = min(len(sp), b.size) // es * es
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
            dtype, k = job["dtype"], job["k"]
            func = job["kind"] == "func"
            es = ES[dtype]
            kk = max(1, k)
            counts = job.get("counts") or [job["n"]] * P
            total = kk * sum(counts) * es
            mine = counts[rank] * es
            start = kk * sum(counts[:rank]) * es  # this rank's slot in the output
            raw_out = hip_rt.malloc(256 + 2 * es + total + GUARD)
            out = raw_out + 256 + offset(rank, 0) * es
            raw_in = [hip_rt.malloc(256 + 2 * es + mine + GUARD) for _ in range(k)]
            ins = [raw_in[i] + 256 + offset(rank, i + 1) * es for i in range(k)]
            stream = hip_rt.stream_create() if job.get("caller_stream") else 0
            a = None
            if not func:
                # `op` is not used: the pair the reductions refuse
                a = gloo_amd.Algorithm(ctx, "allgather", "bxor" if dtype != "u8" else 0, dtype, [out] + ins, job["n"],
                                       workspace=job.get("ws", "device"), stream=stream)
            modes = []
            for run in range(job["runs"]):
                blocks = [[payload(ji, job, run, q, i, counts[q]) for i in range(kk)] for q in range(P)]
                want = np.concatenate([b for q in range(P) for b in blocks[q]] + [np.zeros(0, np.uint8)])
                img = np.full(GUARD + total + GUARD, FILL, np.uint8)
                img[GUARD:GUARD + total] = SENTINEL
                if k == 0:
                    img[GUARD + start:GUARD + start + mine] = blocks[rank][0]
                hip_rt.h2d(out - GUARD, img)
                for i in range(k):
                    img = np.full(GUARD + mine + GUARD, FILL, np.uint8)
                    img[GUARD:GUARD + mine] = blocks[rank][i]
                    hip_rt.h2d(ins[i] - GUARD, img)
                if func:
                    gloo_amd.allgather(ctx, out, job["n"], dtype, input=ins[0] if k else None,
                                       counts=job.get("counts"), tag=job.get("tag", 0), stream=stream)
                    modes.append(ctx.last_mode() if total else {})
                else:
                    a.run()
                    modes.append(a.mode())
                if stream:
                    hip_rt.stream_synchronize(stream)
                got = hip_rt.d2h(out - GUARD, np.empty(GUARD + total + GUARD, np.uint8))
                bad = np.flatnonzero(got[GUARD:GUARD + total] != want)
                assert bad.size == 0, f"run {run}: output byte {bad[0]} of {total} is {got[GUARD + bad[0]]:#x}, " \
                                      f"want {want[bad[0]]:#x} ({bad.size} differ)"
                assert (got[:GUARD] == FILL).all(), f"run {run}: bytes in front of the output were written"
                assert (got[GUARD + total:] == FILL).all(), f"run {run}: the guard behind the output was written"
                for i in range(k):
                    got = hip_rt.d2h(ins[i] - GUARD, np.empty(GUARD + mine + GUARD, np.uint8))
                    assert (got[GUARD:GUARD + mine] == blocks[rank][i]).all(), f"run {run}: input {i} was modified"
                    assert (got[:GUARD] == FILL).all() and (got[GUARD + mine:] == FILL).all(), \
                        f"run {run}: the guards of input {i} were written"
            if a is not None:
                a.close()
            if stream:
                hip_rt.stream_destroy(stream)
            for p in [raw_out] + raw_in:
                hip_rt.free(p)
            res.append({"modes": modes})
        except Exception:  # noqa: BLE001 — recorded for the test of this job
            res.append({"err": traceback.format_exc()[-1500:]})
            break  # the peers' next collective would only time out
    ctx.close()
    return res


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
