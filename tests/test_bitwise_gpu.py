"""GPU: the built-in bitwise reductions BAND / BOR / BXOR on every kernel
path — the chunk kernels (3-operand, in place, multi-source), the threads'
schedules, ranks as processes (interpreter, sliced interpreter, fold + forward,
graph replay; the same routes SUM takes) and the host-staged form.

Every expected value is numpy's (np.bitwise_and / or / xor): the ops are exact,
associative and commutative, so each schedule and fold order must return the
same bits.  Inputs cover the full bit range; AND inputs are the OR of three
draws (bit density 7/8) and OR inputs the AND of three (1/8), so that a 9-rank
result is neither all zeros nor all ones, and every collective test asserts
that its expected result has a 0 and a 1 at every bit position."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPS = {"band": np.bitwise_and, "bor": np.bitwise_or, "bxor": np.bitwise_xor}
NPT = {"i8": np.int8, "u8": np.uint8, "i32": np.int32, "u32": np.uint32, "i64": np.int64, "u64": np.uint64}
UNSIGNED = {1: np.uint8, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def bits(rng, npt, shape):
    """Uniform over the dtype's full bit range."""
    n = int(np.prod(shape)) * np.dtype(npt).itemsize
    return rng.integers(0, 256, n, dtype=np.uint8).view(npt).reshape(shape)


def draw(rng, op, npt, shape):
    if op == "band":
        return bits(rng, npt, shape) | bits(rng, npt, shape) | bits(rng, npt, shape)
    if op == "bor":
        return bits(rng, npt, shape) & bits(rng, npt, shape) & bits(rng, npt, shape)
    return bits(rng, npt, shape)


def assert_not_vacuous(want):
    """Every bit position holds a 0 somewhere and a 1 somewhere in `want`."""
    u = np.ascontiguousarray(want).view(UNSIGNED[want.dtype.itemsize]).ravel()
    ones = UNSIGNED[want.dtype.itemsize](~UNSIGNED[want.dtype.itemsize](0))
    assert np.bitwise_or.reduce(u) == ones, "some bit position is 0 everywhere"
    assert np.bitwise_and.reduce(u) == 0, "some bit position is 1 everywhere"


def same_bytes(a, b):
    return a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()


def to_dev(torch, arr, byte_offset):
    """arr's bytes in fresh device memory, `byte_offset` past a 256-B aligned allocation."""
    raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8)
    t = torch.zeros(raw.size + byte_offset + 64, dtype=torch.uint8, device="cuda")
    t[byte_offset:byte_offset + raw.size].copy_(torch.from_numpy(raw.copy()))
    return t, t.data_ptr() + byte_offset


def from_dev(torch, t, byte_offset, like):
    torch.cuda.synchronize()
    return t[byte_offset:byte_offset + like.nbytes].cpu().numpy().view(like.dtype).copy()


# ---- the chunk kernels -----------------------------------------------------

@pytest.mark.parametrize("dtype", sorted(NPT))
@pytest.mark.parametrize("op", sorted(OPS))
def test_kernel_parity(torch, op, dtype):
    """reduce3 and the in-place form, byte-exact, at sizes below one packet,
    ragged, several tiles; dst, a and b each start at their own element offset
    (1, 2 and 3 elements: three different residues mod 16 B for the 1- and
    4-byte dtypes, the two that exist for the 8-byte ones)."""
    import gloo_amd
    npt = NPT[dtype]
    es = np.dtype(npt).itemsize
    rng = np.random.default_rng([3, sorted(OPS).index(op), sorted(NPT).index(dtype)])
    oc, oa, ob = es, 2 * es, 3 * es
    assert len({oc % 16, oa % 16, ob % 16}) == min(3, 16 // es)
    for n in (1, 5, 33, 1000, 4099, 100_003):
        a, b = draw(rng, op, npt, n), draw(rng, op, npt, n)
        want = OPS[op](a, b)
        ta, pa = to_dev(torch, a, oa)
        tb, pb = to_dev(torch, b, ob)
        tc, pc = to_dev(torch, np.zeros(n, npt), oc)
        gloo_amd.reduce3_ptr(op, dtype, pc, pa, pb, n)
        assert same_bytes(from_dev(torch, tc, oc, want), want), ("reduce3", n)
        assert not tc[:oc].any() and not tc[oc + want.nbytes:].any(), ("reduce3 wrote outside its chunk", n)
        assert same_bytes(from_dev(torch, ta, oa, a), a) and same_bytes(from_dev(torch, tb, ob, b), b)
        gloo_amd.reduce_ptr(op, dtype, pa, pb, n)  # in place: dst is a
        assert same_bytes(from_dev(torch, ta, oa, want), want), ("in place", n)
        assert not ta[:oa].any() and not ta[oa + want.nbytes:].any(), ("in place wrote outside its chunk", n)


@pytest.mark.parametrize("op", sorted(OPS))
def test_reduce3_c_aliases_b(torch, op):
    import gloo_amd
    rng = np.random.default_rng(17)
    n = 4099
    a, b = draw(rng, op, np.uint32, n), draw(rng, op, np.uint32, n)
    ta, pa = to_dev(torch, a, 4)
    tb, pb = to_dev(torch, b, 8)
    gloo_amd.reduce3_ptr(op, "u32", pb, pa, pb, n)
    assert same_bytes(from_dev(torch, tb, 8, b), OPS[op](a, b))
    assert same_bytes(from_dev(torch, ta, 4, a), a)


@pytest.mark.parametrize("dtype", ["u8", "i64"])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("op", sorted(OPS))
def test_reduce_multi(torch, op, k, dtype):
    """The one-pass multi-source fold, dst aliasing srcs[0], each source at
    its own residue mod 16 B."""
    import gloo_amd
    npt = NPT[dtype]
    es = np.dtype(npt).itemsize
    n = 4099
    rng = np.random.default_rng([23, k])
    x = draw(rng, op, npt, (k, n))
    want = OPS[op].reduce(x, axis=0)
    devs = [to_dev(torch, x[j], (j + 1) * es % 16) for j in range(k)]
    gloo_amd.reduce_multi_ptr(op, dtype, devs[0][1], [p for _, p in devs], n)
    assert same_bytes(from_dev(torch, devs[0][0], es % 16, want), want)
    for j in range(1, k):
        assert same_bytes(from_dev(torch, devs[j][0], (j + 1) * es % 16, x[j]), x[j]), j


def test_floating_dtype_is_rejected(torch):
    import gloo_amd
    a = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(a[::-1].copy()).cuda()
    with pytest.raises(gloo_amd.GlooHipError) as e:
        gloo_amd.reduce_ptr("bxor", "f32", ta.data_ptr(), tb.data_ptr(), a.size)
    assert e.value.code == -1
    assert "bxor" in str(e.value) and "f32" in str(e.value)
    torch.cuda.synchronize()
    assert same_bytes(ta.cpu().numpy(), a)


# ---- schedules, ranks as threads -------------------------------------------

SCHEDULES = [("ring_chunked", 3), ("ring_chunked", 4), ("halving_doubling", 4), ("halving_doubling", 5), ("ring", 3),
             ("local", 1), ("bcube", 4), ("bcube", 9)]
THREAD_CASES = [("bxor", "i32", algo, P) for algo, P in SCHEDULES] + \
               [(op, dtype, algo, P) for op in ("band", "bor") for dtype in ("u8", "i64")
                for algo, P in (("ring_chunked", 4), ("halving_doubling", 5))]


@pytest.mark.parametrize("op,dtype,algo,P", THREAD_CASES)
def test_threads(torch, op, dtype, algo, P):
    from test_collectives_gpu import run_threads
    k = 3 if algo == "local" else 1
    x = draw(np.random.default_rng([31, P]), op, NPT[dtype], (P, k, 10_007))
    want = OPS[op].reduce(x.reshape(P * k, -1), axis=0)
    assert_not_vacuous(want)
    recv = ([3] if P == 9 else [2]) if algo == "bcube" else None  # AllreduceBcube's base
    y = run_threads(torch, algo, op, dtype, x, recv=recv, runs=1)
    for r in range(P):
        for j in range(k):
            assert same_bytes(y[r, j], want), (r, j)


def test_reduce_scatter_threads(torch):
    from test_collectives_gpu import run_threads
    P, n = 5, 10_007
    recv = [n // P + (1 if r < n % P else 0) for r in range(P)]
    x = draw(np.random.default_rng(37), "bxor", np.int32, (P, 1, n))
    want = np.bitwise_xor.reduce(x[:, 0], axis=0)
    assert_not_vacuous(want)
    y = run_threads(torch, "reduce_scatter", "bxor", "i32", x, recv=recv)
    off = 0
    for r in range(P):
        assert same_bytes(y[r, 0, :recv[r]], want[off:off + recv[r]]), r
        off += recv[r]


# ---- ranks as processes: the op takes SUM's routes ---------------------------

PROC_P = 4
PROC_RUNS = 3
PROC_ALGOS = [("ring_chunked", 1), ("halving_doubling", 1), ("halving_doubling_pipelined", 2)]
NEW_STYLE = ["ring", "bcube", "reduce"]


def proc_seed(n, rank, j):
    return bits(np.random.default_rng([41, n, rank, j]), np.uint32, n)


def proc_const(what, run, rank, j):
    """Run `run`'s input is the seed input XOR this constant: it differs per
    run, rank and pointer, so it does not cancel in the XOR over the ranks and
    a stale read of an earlier run's bytes changes the result."""
    return np.uint32(np.random.default_rng([43, what, run, rank, j]).integers(0, 1 << 32))


WORKER = r'''
import hashlib, json, os, sys, numpy as np
sys.path.insert(0, os.environ["GLOO_AMD_ROOT"])
sys.path.insert(0, os.path.join(os.environ["GLOO_AMD_ROOT"], "tests"))
import torch, gloo_amd
from test_bitwise_gpu import PROC_ALGOS, PROC_RUNS, NEW_STYLE, proc_seed, proc_const
rank, size, store, n = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
torch.cuda.set_device(0)
ctx = gloo_amd.Context(rank, size, store, device=0, timeout_ms=60000)
sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
res = {}
for w, (algo, k) in enumerate(PROC_ALGOS):
    seeds = [torch.from_numpy(proc_seed(n, rank, j).view(np.int32)).cuda() for j in range(k)]
    bufs = [torch.empty_like(s) for s in seeds]
    for op in ("bxor", "sum"):
        a = gloo_amd.Algorithm(ctx, algo, op, "u32", [b.data_ptr() for b in bufs], n)
        outs, modes = [], []
        for run in range(PROC_RUNS):
            for j in range(k):
                c = int(proc_const(w, run, rank, j).view(np.int32))
                torch.bitwise_xor(seeds[j], c, out=bufs[j])
            torch.cuda.synchronize()
            a.run()
            outs.append([sha(b) for b in bufs])
            modes.append(a.mode())
        a.close()
        res[algo + "/" + op] = {"outs": outs, "modes": modes}
src = torch.empty(n, dtype=torch.int32, device="cuda")
out = torch.empty_like(src)
seed = torch.from_numpy(proc_seed(n, rank, 0).view(np.int32)).cuda()
for w, kind in enumerate(NEW_STYLE):
    for op in ("bxor", "sum"):
        outs, modes = [], []
        for run in range(PROC_RUNS):
            torch.bitwise_xor(seed, int(proc_const(10 + w, run, rank, 0).view(np.int32)), out=src)
            out.fill_(0)
            torch.cuda.synchronize()
            if kind == "reduce":
                gloo_amd.reduce_to_root(ctx, out.data_ptr(), n, "u32", 0, op, input=src.data_ptr())
            else:
                gloo_amd.allreduce(ctx, [out.data_ptr()], n, "u32", op, inputs=[src.data_ptr()], algorithm=kind)
            outs.append(sha(out))
            modes.append(ctx.last_mode())
        res[kind + "/" + op] = {"outs": outs, "modes": modes}
ctx.close()
print("RESULT" + json.dumps(res), flush=True)
'''


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [12_289, 1_048_579])
def test_processes_take_sums_routes(torch, n):
    """P = 4 processes on one GPU (device signalling, IPC arenas), u32.
    n = 12,289: messages under the 64 KiB fuse limit, the interpreters' regime;
    n = 1,048,579 (4 MiB per rank): fold + forward and graph replay.  Three
    runs per algorithm, each on different inputs, each checked by SHA-256
    against numpy; and mode() after every run is, field by field, what the
    same algorithm and shape reports with "sum" (no mode is hard-coded)."""
    P = PROC_P
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(WORKER)
        e = dict(os.environ, GLOO_AMD_ROOT=ROOT)
        procs = [subprocess.Popen([sys.executable, w, str(r), str(P), "file:" + os.path.join(d, "s"), str(n)], env=e,
                                  stdout=subprocess.PIPE, text=True) for r in range(P)]
        outs = [p.communicate(timeout=280)[0] for p in procs]
        assert [p.returncode for p in procs] == [0] * P
    res = [json.loads(o.split("RESULT", 1)[1]) for o in outs]

    def expected(what, k, run):
        xs = [proc_seed(n, r, j) ^ proc_const(what, run, r, j) for r in range(P) for j in range(k)]
        want = np.bitwise_xor.reduce(np.stack(xs), axis=0)
        assert_not_vacuous(want)
        return hashlib.sha256(want.tobytes()).hexdigest()

    for w, (algo, k) in enumerate(PROC_ALGOS):
        want = [expected(w, k, run) for run in range(PROC_RUNS)]
        assert len(set(want)) == PROC_RUNS  # the runs differ: a stale result cannot pass
        for r in range(P):
            got = res[r][algo + "/bxor"]
            assert got["outs"] == [[h] * k for h in want], (algo, r)
            for mb, ms in zip(got["modes"], res[r][algo + "/sum"]["modes"]):
                assert set(mb) == set(ms)
                for field in ms:
                    assert mb[field] == ms[field], (algo, r, field, mb, ms)
    for w, kind in enumerate(NEW_STYLE):
        want = [expected(10 + w, 1, run) for run in range(PROC_RUNS)]
        assert len(set(want)) == PROC_RUNS
        for r in range(P):
            got = res[r][kind + "/bxor"]
            if kind != "reduce" or r == 0:  # gloo::reduce: only the root's output holds the result
                assert got["outs"] == want, (kind, r)
            for mb, ms in zip(got["modes"], res[r][kind + "/sum"]["modes"]):
                assert set(mb) == set(ms)
                for field in ms:
                    assert mb[field] == ms[field], (kind, r, field, mb, ms)


# ---- host-staged -----------------------------------------------------------

@pytest.mark.parametrize("piece", [0, 1])
def test_staged(torch, piece):
    """gloo_hip_reduce_staged: zero-copy over PCIe (piece 0) and through the
    device scratch (piece 1, raised to one 16 MiB piece: a single pass)."""
    import gloo_amd
    n = 100_003
    rng = np.random.default_rng(47)
    a, b = draw(rng, "bor", np.int32, n), draw(rng, "bor", np.int32, n)
    want = a | b
    hd, hs = torch.from_numpy(a.copy()).pin_memory(), torch.from_numpy(b.copy()).pin_memory()
    dd = torch.empty(n, dtype=torch.int32, device="cuda:0")
    ds = torch.empty(n, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream()
    gloo_amd.reduce_staged("bor", "i32", hd.data_ptr(), hs.data_ptr(), n, dd.data_ptr(), ds.data_ptr(), piece,
                           s.cuda_stream)
    s.synchronize()
    assert same_bytes(hd.numpy(), want)
    assert same_bytes(hs.numpy(), b)
