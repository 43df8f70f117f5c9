"""One rank of a batch of gather / scatter jobs — test infrastructure of
tests/test_gather_scatter_gpu.py, following broadcast_worker.py.

main() runs run_rank() as one rank process ("file:" store, argv: RANK P DIR
JOBS_JSON) or as P rank threads of one child process ("mem:" store, argv:
threads P DIR JOBS_JSON).  Both models are closed form, so every rank checks
its own buffers and writes a report (r<rank>.json): per job either
{"err": text} or {"modes": [...], "stats": {...}}.

A job: {coll: "gather" | "scatter", kind: "algo" | "func", dtype, n | counts,
root, rotate, alias, runs, ws, caller_stream, profile}.  counts: the gatherv form.
alias: the in-place forms, on the root only: a gather root's input IS its own
slot of its output; a scatter root's output IS its input `root`.
rotate (func only): run i's root is (root + i) % P.  Every buffer starts 1, 2
or 0 elements past a 256-byte boundary (so sources and destinations differ in
their 16-byte misalignment), with GUARD bytes in front of it and behind it.

gather: rank q's input gets the run's payload of rank q; the root's output a
sentinel; a rank that is not the root ALSO passes an output pointer, filled
with the sentinel, which the library must ignore.  After the run the root's
whole output is block 0 ... block P-1, every other rank's "output" is still
the sentinel, and every input is unmodified.
scatter: the root's P inputs get the run's payloads (odd job indices: P
slices of one allocation, back to back; even: separate allocations); every
rank's output a sentinel.  After the run rank q's whole output is payload q.
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

ES = {"u8": 1, "f64": 8}
GUARD, SENTINEL, FILL = 64, 0xEE, 0xA5
# NaN bit patterns (quiet and signalling, with payloads) and -0 in front of a float payload
SPECIAL = {
    "f64": np.array([0x7FF8000000000001, 0xFFF0000000000123, 0x8000000000000000], np.uint64).view(np.uint8),
    "u8": np.array([], np.uint8),
}


def payload(job_index, job, run, q, nbytes):
    """Block q of run `run`: different for every job, run and rank, never the sentinel."""
    rng = np.random.default_rng(100000 * job_index + 100 * run + q + 1)
    b = rng.integers(0, 256, nbytes, dtype=np.uint8)
    b[b == SENTINEL] = run
    es = ES[job["dtype"]]
    sp = SPECIAL[job["dtype"]]
    m = min(len(sp), nbytes) // es * es
    b[:m] = sp[:m]
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


def run_rank(rank, P, url, jobs, device=0, timeout_ms=20000):  # a lost message ends inside the test's own limit
    import gloo_amd
    import hip_rt
    hip_rt.set_device(device)
    ctx = gloo_amd.Context(rank, P, url, device=device, timeout_ms=timeout_ms)
    res = []
    for ji, job in enumerate(jobs):
        try:
            dtype, root0 = job["dtype"], job["root"]
            gather, func = job["coll"] == "gather", job["kind"] == "func"
            es = ES[dtype]
            counts = job.get("counts")
            cnt = list(counts) if counts is not None else [job["n"]] * P
            total = sum(cnt)
            stream = hip_rt.stream_create() if job.get("caller_stream") else 0
            bufs = []
            if gather:
                inp = Buf(hip_rt, cnt[rank] * es, (rank + 1) % 3, es)
                out = Buf(hip_rt, total * es, (rank + 2) % 3, es)  # the root's; elsewhere it must stay untouched
                bufs = [inp, out]
            else:
                n = job["n"]
                out = Buf(hip_rt, n * es, (rank + 2) % 3, es)
                slab = Buf(hip_rt, P * n * es, (rank + 1) % 3, es) if ji % 2 else None
                ins = [Buf(hip_rt, n * es, (rank + q) % 3, es) for q in range(P)] if slab is None else []
                in_ptrs = [slab.ptr + q * n * es for q in range(P)] if slab else [b.ptr for b in ins]
                bufs = [out] + ([slab] if slab else ins)
            alias = bool(job.get("alias")) and rank == root0  # (never with rotate)
            off_root = sum(cnt[:root0]) * es
            in_ptr = out.ptr + off_root if gather and alias else inp.ptr if gather else None
            out_ptr = in_ptrs[rank] if alias and not gather else out.ptr
            a = None
            if not func:
                # `op` is not used: the pair the reductions refuse
                op = "bxor" if dtype != "u8" else 0
                if gather:
                    a = gloo_amd.Algorithm(ctx, "gather", op, dtype, [in_ptr, out_ptr], job.get("n", 0),
                                           recv_elems=[root0] + (cnt if counts is not None else []),
                                           workspace=job.get("ws", "device"), stream=stream)
                else:
                    ptrs = [out_ptr] + (in_ptrs if rank == root0 else [])
                    a = gloo_amd.Algorithm(ctx, "scatter", op, dtype, ptrs, job["n"], recv_elems=[root0],
                                           workspace=job.get("ws", "device"), stream=stream)
                if job.get("profile"):
                    a.set_profiling(job["profile"])
            modes, stats = [], None
            for run in range(job["runs"]):
                root = (root0 + run) % P if job.get("rotate") else root0
                pay = [payload(ji, job, run, q, cnt[q] * es) for q in range(P)]
                out.fill(SENTINEL)
                if gather:
                    inp.fill(pay[rank])
                    if alias:
                        hip_rt.h2d(in_ptr, pay[rank])
                    if func:
                        gloo_amd.gather(ctx, in_ptr, job.get("n", 0), dtype, root, output=out_ptr, counts=counts,
                                        tag=job.get("tag", 0), stream=stream)
                else:
                    if slab:
                        slab.fill(np.concatenate(pay) if rank == root else SENTINEL)
                    for q, b in enumerate(ins):
                        b.fill(pay[q] if rank == root else SENTINEL)
                    if func:
                        gloo_amd.scatter(ctx, out_ptr, job["n"], dtype, root, inputs=in_ptrs if rank == root else None,
                                         tag=job.get("tag", 0), stream=stream)
                if func:
                    modes.append(ctx.last_mode() if total else {})
                else:
                    a.run()
                    modes.append(a.mode())
                if stream:
                    hip_rt.stream_synchronize(stream)
                if a is not None and job.get("profile"):
                    stats = a.stats()
                what = f"run {run} (root {root})"
                if gather:
                    want = np.concatenate(pay + [np.zeros(0, np.uint8)]) if rank == root else SENTINEL
                    out.check(want, what + (" output" if rank == root else " the output a non-root passed"))
                    inp.check(pay[rank], what + " input")
                else:
                    out.check(SENTINEL if alias else pay[rank], what + " output")  # in place: input `root` is checked below
                    if slab:
                        slab.check(np.concatenate(pay) if rank == root else SENTINEL, what + " inputs")
                    for q, b in enumerate(ins):
                        b.check(pay[q] if rank == root else SENTINEL, what + f" input {q}")
            if a is not None:
                a.close()
            if stream:
                hip_rt.stream_destroy(stream)
            for b in bufs:
                b.free()
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
