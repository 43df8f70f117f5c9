"""One rank of a batch of alltoall jobs — test infrastructure of
tests/test_alltoall_gpu.py, following gather_scatter_worker.py.

main() runs run_rank() as one rank process ("file:" store, argv: RANK P DIR
JOBS_JSON) or as P rank threads of one child process ("mem:" store, argv:
threads P DIR JOBS_JSON).  The model is closed form,
    out_r[outOff_r[q], +M[q][r]) == in_q[inOff_q[r], +M[q][r]),
so every rank checks its own buffers and writes a report (r<rank>.json): per
job either {"err": text} or {"modes": [...], "stats": {...}, "refused": text}.

A job: {kind: "algo" | "func", form: "even" | "matrix" | "lists", dtype, n |
matrix (flat P * P, elements from rank q to rank r at [q * P + r]), runs, ws,
caller_stream, profile, tag}.  Further keys:
  seq        (func) one matrix per run instead of `matrix`: the hit / miss case.
  bad_lists  (func, lists) {rank: [in_counts, out_counts]}: a first call with
             these lists, which every rank must refuse with all of `expect`
             in the text and its output untouched; the job's runs follow on
             the same context.
  bad_matrix (algo) {rank: matrix}: a first construction in which those ranks
             pass another matrix, refused on every rank likewise.
Every buffer starts 1, 2 or 0 elements past a 256-byte boundary, with GUARD
bytes in front of it and behind it; the output starts as a sentinel every run
and the payload differs for every job, run and (sender, receiver) pair.
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

ES = {"u8": 1, "f16": 2, "f32": 4, "f64": 8}
GUARD, SENTINEL, FILL = 64, 0xEE, 0xA5


def payload(job_index, run, q, r, nbytes):
    """The block rank q sends to rank r in run `run`; never the sentinel."""
    rng = np.random.default_rng(1000003 * job_index + 10007 * run + 101 * q + r + 1)
    b = rng.integers(0, 256, nbytes, dtype=np.uint8)
    b[b == SENTINEL] = run
    return b


class Buf:
    """nbytes of device memory `shift` elements past a 256-byte boundary, guarded on both sides."""

    def __init__(self, hip_rt, nbytes, shift, es):
        self.rt, self.nbytes = hip_rt, nbytes
        self.raw = hip_rt.malloc(256 + 2 * es + nbytes + GUARD)
        self.ptr = self.raw + 256 + shift * es

    def fill(self, data):
        img = np.full(GUARD + self.nbytes + GUARD, FILL, np.uint8)
        img[GUARD:GUARD + self.nbytes] = data
        self.rt.h2d(self.ptr - GUARD, img)

    def check(self, want, what):
        got = self.rt.d2h(self.ptr - GUARD, np.empty(GUARD + self.nbytes + GUARD, np.uint8))
        body = got[GUARD:GUARD + self.nbytes]
        bad = np.flatnonzero(body != want)
        assert bad.size == 0, f"{what}: byte {bad[0]} of {self.nbytes} is {body[bad[0]]:#x}, " \
                              f"want {np.broadcast_to(want, body.shape)[bad[0]]:#x} ({bad.size} differ)"
        assert (got[:GUARD] == FILL).all(), f"{what}: bytes in front were written"
        assert (got[GUARD + self.nbytes:] == FILL).all(), f"{what}: guard behind was written"

    def free(self):
        self.rt.free(self.raw)


def cat(blocks):
    return np.concatenate(blocks + [np.zeros(0, np.uint8)])


def run_rank(rank, P, url, jobs, device=0, timeout_ms=20000):  # a lost message ends inside the test's own limit
    import gloo_amd
    import hip_rt
    hip_rt.set_device(device)
    ctx = gloo_amd.Context(rank, P, url, device=device, timeout_ms=timeout_ms)
    res = []
    for ji, job in enumerate(jobs):
        try:
            dtype, func, form = job["dtype"], job["kind"] == "func", job["form"]
            es = ES[dtype]
            even = [job.get("n", 0)] * (P * P)
            per_run = job.get("seq") or [job.get("matrix") or even] * job["runs"]
            row = lambda M: [M[rank * P + r] for r in range(P)]  # noqa: E731
            col = lambda M: [M[q * P + rank] for q in range(P)]  # noqa: E731
            most_in = max(sum(row(M)) for M in per_run)
            most_out = max(sum(col(M)) for M in per_run)
            stream = hip_rt.stream_create() if job.get("caller_stream") else 0
            fixed = "seq" not in job  # one pair of buffers for every run (an algorithm is bound to it)
            inp = Buf(hip_rt, most_in * es, (rank + 1) % 3, es)
            out = Buf(hip_rt, most_out * es, (rank + 2) % 3, es)
            refused = None

            def refusal(call):
                out.fill(SENTINEL)
                inp.fill(FILL)
                try:
                    call()
                except gloo_amd.GlooHipError as e:
                    text = str(e)
                else:
                    raise AssertionError("the call was not refused")
                for part in job["expect"]:
                    assert part in text, (part, text)
                out.check(SENTINEL, "the output of a refused call")
                return text

            if "bad_lists" in job:
                ic, oc = job["bad_lists"][str(rank)]
                refused = refusal(lambda: gloo_amd.alltoall(ctx, inp.ptr, out.ptr, 0, dtype, in_counts=ic,
                                                            out_counts=oc, stream=stream))
            if "bad_matrix" in job:
                bad = job["bad_matrix"].get(str(rank), per_run[0])
                refused = refusal(lambda: gloo_amd.Alltoall(ctx, dtype, inp.ptr, out.ptr, matrix=bad, stream=stream))
            a = None
            if not func:
                a = gloo_amd.Alltoall(ctx, dtype, inp.ptr, out.ptr, count=job.get("n", 0),
                                      matrix=None if form == "even" else per_run[0], stream=stream,
                                      workspace=job.get("ws", "device"))
                if job.get("profile"):
                    a.set_profiling(job["profile"])
            modes, stats = [], None
            for run, M in enumerate(per_run):
                if not fixed:  # the run's own sizes, so that the guard sits right behind the run's last byte
                    inp.free()
                    out.free()
                    inp = Buf(hip_rt, sum(row(M)) * es, (rank + 1 + run) % 3, es)
                    out = Buf(hip_rt, sum(col(M)) * es, (rank + 2 + run) % 3, es)
                mine = cat([payload(ji, run, rank, r, M[rank * P + r] * es) for r in range(P)])
                want = cat([payload(ji, run, q, rank, M[q * P + rank] * es) for q in range(P)])
                inp.fill(mine)
                out.fill(SENTINEL)
                if func:
                    kw = {"even": {}, "matrix": {"matrix": M},
                          "lists": {"in_counts": row(M), "out_counts": col(M)}}[form]
                    gloo_amd.alltoall(ctx, inp.ptr, out.ptr, job.get("n", 0), dtype, tag=job.get("tag", 0),
                                      stream=stream, **kw)
                    modes.append(ctx.last_mode() if any(M) else {})
                else:
                    a.run()
                    modes.append(a.mode())
                if stream:
                    hip_rt.stream_synchronize(stream)
                if a is not None and job.get("profile"):
                    stats = a.stats()
                out.check(want, f"run {run} output")
                inp.check(mine, f"run {run} input")
            if a is not None:
                a.close()
            if stream:
                hip_rt.stream_destroy(stream)
            inp.free()
            out.free()
            res.append({"modes": modes, "stats": stats, "refused": refused})
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
