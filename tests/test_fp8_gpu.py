"""GPU: the FP8 dtypes F8E4M3 (OCP e4m3fn) and F8E5M2 (OCP e5m2) on every
kernel path — the chunk kernels over every operand pair (3-operand, in place,
multi-source), the threads' schedules, ranks as processes (interpreter, fold +
forward, graph replay: the routes u8 SUM takes) and the host-staged form.

Every expected byte is the model's (tests/fp8_model.py: torch on the CPU, an
f32 NaN stored as 0x7F).  FP8 sums are not associative, so the collectives'
expected bytes come from the plans simulated on the CPU (tests/plan_sim.py with
the model in the oracle's place): a route that folds in another order than the
reference's fails, and each collective test asserts that its inputs make the
order visible (left-to-right and right-to-left folds differ in at least 5 % of
the elements) while every output stays finite."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import threading
import uuid

import numpy as np
import pytest

import fp8_model
from fp8_model import fp8_op

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = sorted(fp8_model.FORMATS)


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def tables():
    """(a, b, {(dtype, op): want}) over all 65,536 operand pairs, computed once."""
    a, b = fp8_model.table()
    return a, b, {(dt, op): fp8_op(op, dt, a, b) for dt in FORMATS for op in fp8_model.OPS}


def to_dev(torch, arr, byte_offset):
    """arr's bytes in fresh device memory, `byte_offset` past a 256-B aligned allocation."""
    raw = np.ascontiguousarray(arr, dtype=np.uint8)
    t = torch.zeros(raw.size + byte_offset + 64, dtype=torch.uint8, device="cuda")
    t[byte_offset:byte_offset + raw.size].copy_(torch.from_numpy(raw.copy()))
    return t, t.data_ptr() + byte_offset


def from_dev(torch, t, byte_offset, n):
    torch.cuda.synchronize()
    return t[byte_offset:byte_offset + n].cpu().numpy().copy()


def assert_bytes(got, want, a, b, what):
    bad = np.flatnonzero(got != want)
    first = [f"a={a[i]:#04x} b={b[i]:#04x} got={got[i]:#04x} want={want[i]:#04x}" for i in bad[:16]]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ; first: {first}"


# ---- the chunk kernels: every operand pair ---------------------------------

# byte offsets of (c, a, b): congruent, and each operand at its own residue
OFFSETS = [(0, 0, 0), (1, 3, 15), (3, 15, 0), (15, 1, 3), (0, 15, 1)]


@pytest.mark.parametrize("op", fp8_model.OPS)
@pytest.mark.parametrize("dtype", FORMATS)
def test_every_operand_pair(torch, tables, dtype, op):
    """The 256 x 256 table through gloo_hip_reduce3 and the in-place
    gloo_hip_reduce, byte for byte, with c, a and b each at byte offsets from
    {0, 1, 3, 15}: the vector body (packed converts, the redone packets), the
    head and the tail all see every kind of pair."""
    import gloo_amd
    a, b, wants = tables
    want = wants[(dtype, op)]
    n = a.size
    for oc, oa, ob in OFFSETS:
        ta, pa = to_dev(torch, a, oa)
        tb, pb = to_dev(torch, b, ob)
        tc, pc = to_dev(torch, np.zeros(n, np.uint8), oc)
        gloo_amd.reduce3_ptr(op, dtype, pc, pa, pb, n)
        assert_bytes(from_dev(torch, tc, oc, n), want, a, b, ("reduce3", oc, oa, ob))
        assert not tc[:oc].any() and not tc[oc + n:].any(), ("reduce3 wrote outside its chunk", oc, oa, ob)
        assert (from_dev(torch, ta, oa, n) == a).all() and (from_dev(torch, tb, ob, n) == b).all()
        gloo_amd.reduce_ptr(op, dtype, pa, pb, n)  # in place: dst is a
        assert_bytes(from_dev(torch, ta, oa, n), want, a, b, ("in place", oa, ob))
        assert not ta[:oa].any() and not ta[oa + n:].any(), ("in place wrote outside its chunk", oa, ob)


@pytest.mark.parametrize("op", fp8_model.OPS)
@pytest.mark.parametrize("dtype", FORMATS)
def test_edges(torch, tables, dtype, op):
    """Sizes around one 16-byte packet on a slice of the table that steps
    through all kinds of pairs: the element-wise head and tail alone (n < 16
    plus offset), and with a short body between them."""
    import gloo_amd
    a, b, wants = tables
    for n in (0, 1, 15, 16, 17, 4099):
        idx = (np.arange(n) * 4099 + 77) % 65536  # 4099 is prime: no pair repeats
        x, y, want = a[idx], b[idx], wants[(dtype, op)][idx]
        for oc, oa, ob in ((3, 1, 15), (0, 0, 0)):
            ta, pa = to_dev(torch, x, oa)
            tb, pb = to_dev(torch, y, ob)
            tc, pc = to_dev(torch, np.zeros(n, np.uint8), oc)
            gloo_amd.reduce3_ptr(op, dtype, pc, pa, pb, n)
            assert_bytes(from_dev(torch, tc, oc, n), want, x, y, ("reduce3", n, oc))
            assert not tc[:oc].any() and not tc[oc + n:].any(), ("reduce3 wrote outside its chunk", n, oc)
            gloo_amd.reduce_ptr(op, dtype, pa, pb, n)
            assert_bytes(from_dev(torch, ta, oa, n), want, x, y, ("in place", n, oa))
            assert not ta[:oa].any() and not ta[oa + n:].any(), ("in place wrote outside its chunk", n, oa)


@pytest.mark.parametrize("op", ["sum", "product", "min"])
@pytest.mark.parametrize("dtype", FORMATS)
def test_reduce3_c_aliases_b(torch, tables, dtype, op):
    import gloo_amd
    a, b, wants = tables
    ta, pa = to_dev(torch, a, 1)
    tb, pb = to_dev(torch, b, 3)
    gloo_amd.reduce3_ptr(op, dtype, pb, pa, pb, a.size)
    assert_bytes(from_dev(torch, tb, 3, a.size), wants[(dtype, op)], a, b, "c aliases b")
    assert (from_dev(torch, ta, 1, a.size) == a).all()


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("op", ["sum", "max"])
@pytest.mark.parametrize("dtype", FORMATS)
def test_reduce_multi(torch, dtype, op, k):
    """The one-pass multi-source fold rounds to the format after every op: it
    is k - 1 applications of the two-operand model, left to right.  dst aliases
    srcs[0]; each source sits at its own residue mod 16 B."""
    import gloo_amd
    n = 10_007
    x = fp8_model.draw_small(np.random.default_rng([23, k]), dtype, (k, n))
    want = fp8_model.fold_left(op, dtype, list(x))
    assert fp8_model.is_finite(dtype, want).all()
    if op == "sum" and k >= 3:
        assert (want != fp8_model.fold_right(op, dtype, list(x))).mean() >= 0.05
    devs = [to_dev(torch, x[j], (5 * j + 1) % 16) for j in range(k)]
    gloo_amd.reduce_multi_ptr(op, dtype, devs[0][1], [p for _, p in devs], n)
    got = from_dev(torch, devs[0][0], 1, n)
    assert_bytes(got, want, x[0], x[-1], ("reduce_multi", k))
    for j in range(1, k):
        assert (from_dev(torch, devs[j][0], (5 * j + 1) % 16, n) == x[j]).all(), j


# ---- schedules, ranks as threads -------------------------------------------

SCHEDULES = [("ring_chunked", 3), ("ring_chunked", 4), ("halving_doubling", 4), ("halving_doubling", 5), ("ring", 3),
             ("local", 1), ("bcube", 4), ("bcube", 9)]
THREAD_CASES = [("sum", "f8e4m3", algo, P) for algo, P in SCHEDULES] + \
               [(op, dtype, algo, P) for op, dtype in (("product", "f8e5m2"), ("min", "f8e4m3"))
                for algo, P in (("ring_chunked", 4), ("halving_doubling", 5))]
N_THREADS = 10_007


def order_is_visible(op, dtype, x):
    """Non-vacuity of an order-sensitive collective on inputs x [P][k][n]: the
    share of elements where the left-to-right and the right-to-left fold of
    all P * k inputs differ."""
    xs = list(x.reshape(-1, x.shape[-1]))
    return float((fp8_model.fold_left(op, dtype, xs) != fp8_model.fold_right(op, dtype, xs)).mean())


def simulated(monkeypatch, algo, op, dtype, x, recv=None, **kw):
    import plan_sim
    monkeypatch.setattr(plan_sim, "oracle", fp8_model.ModelOracle)
    return plan_sim.simulate(algo, op, dtype, x, recv=recv, **kw)


@pytest.mark.parametrize("op,dtype,algo,P", THREAD_CASES)
def test_threads(torch, monkeypatch, op, dtype, algo, P):
    from test_collectives_gpu import run_threads
    k = 3 if algo == "local" else 1
    x = fp8_model.draw_small(np.random.default_rng(31 + P), dtype, (P, k, N_THREADS))
    recv = ([3] if P == 9 else [2]) if algo == "bcube" else None  # AllreduceBcube's base
    want = simulated(monkeypatch, algo, op, dtype, x, recv=recv)
    assert fp8_model.is_finite(dtype, want).all()
    if op == "min":  # exact in any order; instead: every rank holds the minimum somewhere
        assert all((want[0, 0] == x[r, 0]).any() and (want[0, 0] != x[r, 0]).any() for r in range(P))
    else:
        assert order_is_visible(op, dtype, x) >= 0.05
    y = run_threads(torch, algo, op, dtype, x, recv=recv, runs=1)
    for r in range(P):
        for j in range(k):
            assert_bytes(y[r, j], want[r, j], x[r, j], x[(r + 1) % P, j], (algo, r, j))


@pytest.mark.parametrize("dtype", FORMATS)
def test_reduce_scatter_threads(torch, monkeypatch, dtype):
    from test_collectives_gpu import run_threads
    P, n = 5, N_THREADS
    recv = [n // P + (1 if r < n % P else 0) for r in range(P)]
    x = fp8_model.draw_small(np.random.default_rng(31 + P), dtype, (P, 1, n))
    want = simulated(monkeypatch, "reduce_scatter", "sum", dtype, x, recv=recv)
    assert order_is_visible("sum", dtype, x) >= 0.05
    y = run_threads(torch, "reduce_scatter", "sum", dtype, x, recv=recv)
    for r in range(P):
        assert fp8_model.is_finite(dtype, want[r, 0, :recv[r]]).all()
        assert_bytes(y[r, 0, :recv[r]], want[r, 0, :recv[r]], x[r, 0], x[(r + 1) % P, 0], r)


def specials(dtype):
    """NaN, the largest finite values, the infinities (e5m2), subnormals."""
    if dtype == "f8e4m3":
        return np.array([0x7F, 0xFF, 0x7E, 0xFE, 0x01, 0x81, 0x07, 0x87], np.uint8)
    return np.array([0x7F, 0xFD, 0x7B, 0xFB, 0x7C, 0xFC, 0x01, 0x81, 0x03, 0x83], np.uint8)


@pytest.mark.parametrize("dtype", FORMATS)
def test_threads_with_specials(torch, monkeypatch, dtype):
    """About 1 % of the positions hold a special value: the overflow, infinity
    and NaN rules through a schedule (halving-doubling, P = 4: fold + tree)."""
    from test_collectives_gpu import run_threads
    P, n = 4, N_THREADS
    rng = np.random.default_rng(53)
    x = fp8_model.draw_small(rng, dtype, (P, 1, n))
    hit = rng.random((P, 1, n)) < 0.01
    x[hit] = rng.choice(specials(dtype), size=int(hit.sum()))
    want = simulated(monkeypatch, "halving_doubling", "sum", dtype, x)
    share = float((~fp8_model.is_finite(dtype, want[0, 0])).mean())
    assert 0.005 <= share <= 0.20, share
    y = run_threads(torch, "halving_doubling", "sum", dtype, x, runs=1)
    for r in range(P):
        assert_bytes(y[r, 0], want[r, 0], x[r, 0], x[(r + 1) % P, 0], r)


# ---- ranks as processes: FP8 takes u8 SUM's routes --------------------------

PROC_P = 4
PROC_RUNS = 3
PROC_DTYPE = "f8e4m3"
PROC_ALGOS = [("ring_chunked", 1), ("halving_doubling", 1), ("halving_doubling_pipelined", 2)]
SIM_ALGO = {"ring_chunked": "ring_chunked", "halving_doubling": "halving_doubling",
            "halving_doubling_pipelined": "halving_doubling",  # the plain plan's bytes (test_hd_pipelined_gpu)
            "ring": "allreduce_new", "bcube": "allreduce_bcube", "reduce": "reduce"}
NEW_STYLE = ["ring", "bcube", "reduce"]


def proc_input(what, n, run, rank, j):
    """Differs per case, run, rank and pointer: a stale read of an earlier
    run's bytes changes the result."""
    return fp8_model.draw_small(np.random.default_rng([41, what, n, run, rank, j]), PROC_DTYPE, n)


WORKER = r'''
import hashlib, json, os, sys, numpy as np
sys.path.insert(0, os.environ["GLOO_AMD_ROOT"])
sys.path.insert(0, os.path.join(os.environ["GLOO_AMD_ROOT"], "tests"))
import torch, gloo_amd
from test_fp8_gpu import PROC_ALGOS, PROC_RUNS, PROC_DTYPE, NEW_STYLE, proc_input
rank, size, store, n = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
torch.cuda.set_device(0)
ctx = gloo_amd.Context(rank, size, store, device=0, timeout_ms=60000)
sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
res = {}
for w, (algo, k) in enumerate(PROC_ALGOS):
    bufs = [torch.empty(n, dtype=torch.uint8, device="cuda") for j in range(k)]
    for dtype in (PROC_DTYPE, "u8"):
        a = gloo_amd.Algorithm(ctx, algo, "sum", dtype, [b.data_ptr() for b in bufs], n)
        outs, modes = [], []
        for run in range(PROC_RUNS):
            for j in range(k):
                bufs[j].copy_(torch.from_numpy(proc_input(w, n, run, rank, j)))
            torch.cuda.synchronize()
            a.run()
            outs.append([sha(b) for b in bufs])
            modes.append(a.mode())
        a.close()
        res[algo + "/" + dtype] = {"outs": outs, "modes": modes}
src = torch.empty(n, dtype=torch.uint8, device="cuda")
out = torch.empty_like(src)
for w, kind in enumerate(NEW_STYLE):
    for dtype in (PROC_DTYPE, "u8"):
        outs, modes = [], []
        for run in range(PROC_RUNS):
            src.copy_(torch.from_numpy(proc_input(10 + w, n, run, rank, 0)))
            out.fill_(0)
            torch.cuda.synchronize()
            if kind == "reduce":
                gloo_amd.reduce_to_root(ctx, out.data_ptr(), n, dtype, 0, "sum", input=src.data_ptr())
            else:
                gloo_amd.allreduce(ctx, [out.data_ptr()], n, dtype, "sum", inputs=[src.data_ptr()], algorithm=kind)
            outs.append(sha(out))
            modes.append(ctx.last_mode())
        res[kind + "/" + dtype] = {"outs": outs, "modes": modes}
ctx.close()
print("RESULT" + json.dumps(res), flush=True)
'''


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [12_289, 1_048_579])
def test_processes_take_u8_sums_routes(torch, monkeypatch, n):
    """P = 4 processes on one GPU (device signalling, IPC arenas), e4m3 sum.
    n = 12,289: messages under the 64 KiB fuse limit, the interpreters' regime;
    n = 1,048,579: fold + forward and graph replay.  Three runs per algorithm,
    each on different inputs, each checked by SHA-256 against the simulated
    plan; and mode() after every run is, field by field, what the same
    algorithm and shape reports with u8 sum (no mode is hard-coded)."""
    P = PROC_P
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(WORKER)
        e = dict(os.environ, GLOO_AMD_ROOT=ROOT)
        procs = [subprocess.Popen([sys.executable, w, str(r), str(P), "file:" + os.path.join(d, "s"), str(n)], env=e,
                                  stdout=subprocess.PIPE, text=True) for r in range(P)]
        outs = [None] * P
        try:
            for r, p in enumerate(procs):  # every rank under its own limit
                outs[r] = p.communicate(timeout=240)[0]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
        assert [p.returncode for p in procs] == [0] * P
    res = [json.loads(o.split("RESULT", 1)[1]) for o in outs]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731

    def same_modes(got, ref, what):
        for mb, ms in zip(got["modes"], ref["modes"]):
            assert set(mb) == set(ms)
            for field in ms:
                assert mb[field] == ms[field], (what, field, mb, ms)

    for w, (algo, k) in enumerate(PROC_ALGOS):
        wants = []
        for run in range(PROC_RUNS):
            x = np.array([[proc_input(w, n, run, r, j) for j in range(k)] for r in range(P)])
            assert order_is_visible("sum", PROC_DTYPE, x) >= 0.05
            y = simulated(monkeypatch, SIM_ALGO[algo], "sum", PROC_DTYPE, x, seed=run)
            assert fp8_model.is_finite(PROC_DTYPE, y).all()
            wants.append([[sha(y[r, j]) for j in range(k)] for r in range(P)])
        assert len({h[0][0] for h in wants}) == PROC_RUNS  # the runs differ: a stale result cannot pass
        for r in range(P):
            got = res[r][algo + "/" + PROC_DTYPE]
            assert got["outs"] == [wants[run][r] for run in range(PROC_RUNS)], (algo, r)
            same_modes(got, res[r][algo + "/u8"], (algo, r))
    for w, kind in enumerate(NEW_STYLE):
        wants = []
        for run in range(PROC_RUNS):
            x = np.array([[proc_input(10 + w, n, run, r, 0)] for r in range(P)])
            recv = np.array([0], np.int32) if kind == "reduce" else None
            y = simulated(monkeypatch, SIM_ALGO[kind], "sum", PROC_DTYPE, np.zeros_like(x), recv=recv, ins=x, seed=run)
            wants.append([sha(y[r, 0]) for r in range(P)])
        assert len({h[0] for h in wants}) == PROC_RUNS
        for r in range(P):
            got = res[r][kind + "/" + PROC_DTYPE]
            if kind != "reduce" or r == 0:  # gloo::reduce: only the root's output holds the result
                assert got["outs"] == [wants[run][r] for run in range(PROC_RUNS)], (kind, r)
            same_modes(got, res[r][kind + "/u8"], (kind, r))


# ---- host-staged -----------------------------------------------------------

@pytest.mark.parametrize("piece", [0, 1])
def test_staged(torch, piece):
    """gloo_hip_reduce_staged: zero-copy over PCIe (piece 0) and through the
    device scratch (piece 1, raised to one 16 MiB piece: a single pass)."""
    import gloo_amd
    n = 100_003
    rng = np.random.default_rng(47)
    a, b = fp8_model.draw_small(rng, "f8e4m3", n, bound=448.0), fp8_model.draw_small(rng, "f8e4m3", n, bound=448.0)
    want = fp8_op("sum", "f8e4m3", a, b)
    assert 0 < fp8_model.is_nan("f8e4m3", want).sum() < n // 10  # some sums overflow
    hd, hs = torch.from_numpy(a.copy()).pin_memory(), torch.from_numpy(b.copy()).pin_memory()
    dd = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ds = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream()
    gloo_amd.reduce_staged("sum", "f8e4m3", hd.data_ptr(), hs.data_ptr(), n, dd.data_ptr(), ds.data_ptr(), piece,
                           s.cuda_stream)
    s.synchronize()
    assert_bytes(hd.numpy(), want, a, b, ("staged", piece))
    assert (hs.numpy() == b).all()


# ---- rejection ---------------------------------------------------------------

def test_bxor_is_rejected_before_any_exchange(torch):
    """bxor on f8e5m2: reduce, reduce_multi, Algorithm(...) and the
    function-style allreduce refuse it on the calling rank alone — rank 1 of
    the two never makes the call, so a refusal that first exchanged anything
    with the peer would wait for it and time out instead."""
    import gloo_amd
    a = fp8_model.draw_small(np.random.default_rng(1), "f8e5m2", 1000)
    ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(a[::-1].copy()).cuda()

    def refused(call):
        with pytest.raises(gloo_amd.GlooHipError) as e:
            call()
        assert e.value.code == -1
        assert "bxor" in str(e.value) and "f8e5m2" in str(e.value)

    refused(lambda: gloo_amd.reduce_ptr("bxor", "f8e5m2", ta.data_ptr(), tb.data_ptr(), a.size))
    refused(lambda: gloo_amd.reduce_multi_ptr("bxor", "f8e5m2", ta.data_ptr(), [ta.data_ptr(), tb.data_ptr()], a.size))
    assert not gloo_amd.op_supported("bxor", "f8e5m2")

    url = "mem:" + uuid.uuid4().hex
    errors, done = [], threading.Event()

    def body(r):
        try:
            ctx = gloo_amd.Context(r, 2, url, device=0, timeout_ms=20000)
            if r == 0:
                refused(lambda: gloo_amd.Algorithm(ctx, "ring_chunked", "bxor", "f8e5m2", [ta.data_ptr()], a.size))
                refused(lambda: gloo_amd.allreduce(ctx, [ta.data_ptr()], a.size, "f8e5m2", "bxor"))
                done.set()
            else:
                assert done.wait(30)
            ctx.close()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            done.set()

    ts = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    assert (ta.cpu().numpy() == a).all()
