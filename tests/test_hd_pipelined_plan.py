"""CPU: the pipelined halving-doubling plan
(GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED = 11, plan.cc planHalvingDoubling
with `pipelined`), the restatement of CudaAllreduceHalvingDoubling with
pipelineBroadcastAndReduce set (gloo/cuda_allreduce_halving_doubling.cc:246-455).

Its exchange is the plain plan's; only the local multi-pointer steps differ:
the whole-range LOCAL_REDUCE is cut into the first send's and the first
receive's range, the whole-range LOCAL_BCAST into one range per all-gather
step.  So every check here is against the plain `halving_doubling` plan or its
simulation (plan_sim, unchanged), and against the reference's own
multi-pointer golden.
"""
import ctypes

import numpy as np
import pytest

import oracle
import plan_sim
from plan_sim import KIND, SRC_ARENA, ProtocolError, cut_range, simulate, sliceable, sliced_interp_steps, user_cuts

HDP = 11  # GLOO_HIP_ALGO_HALVING_DOUBLING_PIPELINED
NAME = "halving_doubling_pipelined"
EINVAL_ARG = -4
MAX_SRCS, MAX_XDST = 8, 8


@pytest.fixture(autouse=True)
def _name_the_algorithm(monkeypatch):
    """plan_sim.ALGO has no name for the new code: give it one for this module."""
    monkeypatch.setitem(plan_sim.ALGO, NAME, HDP)


def plan_rc(algo, rank, size, count, nptrs):
    """gloo_hip_plan_ex by numeric algorithm code -> (status, steps)."""
    L = plan_sim.plan_lib()
    n, arena = ctypes.c_size_t(), ctypes.c_size_t()
    L.gloo_hip_plan_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    args = (algo, rank, size, count, 0, nptrs, 4, 0, None)
    rc = L.gloo_hip_plan_ex(*args, None, 0, ctypes.byref(n), ctypes.byref(arena))
    if rc:
        return rc, []
    steps = (plan_sim.Step * max(1, n.value))()
    rc = L.gloo_hip_plan_ex(*args, ctypes.cast(steps, ctypes.c_void_p), n.value, ctypes.byref(n),
                            ctypes.byref(arena))
    return rc, [steps[i] for i in range(n.value)]


def plan(algo, rank, size, count, nptrs):
    rc, steps = plan_rc(algo, rank, size, count, nptrs)
    assert rc == 0, f"gloo_hip_plan_ex({algo}) failed: {rc}"
    return steps


def tup(s):
    return (s.kind, s.peer, s.slot, s.flags, s.dst_off, s.src_off, s.length)


def union(ranges):
    """Sorted disjoint cover of [(off, len)]; overlapping ranges are an error."""
    out = []
    for off, ln in sorted(r for r in ranges if r[1]):
        assert not out or off >= out[-1][1], f"overlapping local ranges {ranges}"
        if out and off == out[-1][1]:
            out[-1] = (out[-1][0], off + ln)
        else:
            out.append((off, off + ln))
    return out


def block_of_one(rank, size):
    """The rank's binary block (gloo/allreduce_halving_doubling.h:39-64) has one rank."""
    off = size
    for b in (1 << i for i in range(size.bit_length())):
        if size & b:
            off -= b
            if off <= rank:
                return b == 1
    raise AssertionError


def local_ranges(steps, kind):
    return [(s.dst_off, s.length) for s in steps if s.kind == KIND[kind]]


def test_shape_p4_k3_rank0():
    P, k, n = 4, 3, 1000
    steps = [s for s in plan(HDP, 0, P, n, k) if s.kind != KIND["DECL_RECV"]]
    plain = [s for s in plan(1, 0, P, n, k) if s.kind != KIND["DECL_RECV"]]
    send = next(s for s in plain if s.kind == KIND["SEND"])
    recv = next(s for s in plain if s.kind == KIND["REDUCE"])
    assert [s.kind for s in steps[:4]] == [KIND["LOCAL_REDUCE"], KIND["SEND"], KIND["LOCAL_REDUCE"],
                                           KIND["WAIT_RECV"]]
    assert (steps[0].dst_off, steps[0].length) == (send.src_off, send.length)
    assert tup(steps[1]) == tup(send)
    assert (steps[2].dst_off, steps[2].length) == (recv.dst_off, recv.length)
    assert (0, n) not in local_ranges(steps, "LOCAL_BCAST")
    assert union(local_ranges(steps, "LOCAL_REDUCE")) == [(0, n)]
    assert union(local_ranges(steps, "LOCAL_BCAST")) == [(0, n)]
    # each broadcast sits between its step's COPY and NOTIFY (:376-383)
    for i, s in enumerate(steps):
        if s.kind == KIND["LOCAL_BCAST"]:
            assert steps[i - 1].kind == KIND["COPY"] and steps[i + 1].kind == KIND["NOTIFY"]
    # the exchange itself is the plain plan's
    talk = lambda v: [tup(s) for s in v if s.kind not in (KIND["LOCAL_REDUCE"], KIND["LOCAL_BCAST"])]
    assert talk(steps) == talk(plain)


@pytest.mark.parametrize("P", [2, 3, 5, 6, 7, 8, 12, 13])
def test_local_ranges_cover_the_buffer(P):
    """The reference's per-range reduces and broadcasts leave no gap and no
    overlap: both unions are exactly [0, n) on every rank that pipelines."""
    for n in (1, 3, 64, 1000, 4099):
        for k in (2, 3):
            for r in range(P):
                steps = plan(HDP, r, P, n, k)
                assert union(local_ranges(steps, "LOCAL_REDUCE")) == [(0, n)], (P, n, r)
                assert union(local_ranges(steps, "LOCAL_BCAST")) == [(0, n)], (P, n, r)
                differs = [tup(s) for s in steps] != [tup(s) for s in plan(1, r, P, n, k)]
                assert differs == (not block_of_one(r, P)), (P, n, r)


@pytest.mark.parametrize("P,n,k,rank", [(4, 1000, 1, 0), (4, 1000, 1, 3), (1, 1000, 3, 0), (4, 0, 3, 1), (3, 1000, 3, 2),
                                        (13, 4099, 4, 12)])
def test_degenerate_forms_equal_the_plain_plan(P, n, k, rank):
    assert [tup(s) for s in plan(HDP, rank, P, n, k)] == [tup(s) for s in plan(1, rank, P, n, k)]


def _inputs(dtype, op, P, k, n, seed):
    rng = np.random.default_rng(seed)
    npt = oracle.DTYPES[dtype][1]
    if dtype == "i32":
        hi = 3 if op == "product" else 1000
        return rng.integers(-hi, hi + 1, (P, k, n)).astype(npt)
    if dtype == "bf16":
        return rng.integers(0x3C00, 0x4200, (P, k, n)).astype(npt)  # finite, positive
    x = rng.standard_normal((P, k, n))
    if op == "product":
        x = 1.0 + x / 64
    return x.astype(npt)


def same(a, b):
    return a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()


@pytest.mark.parametrize("op", ["sum", "product", "max", "min"])
@pytest.mark.parametrize("P", [2, 3, 4, 5, 6, 7, 8, 9, 13, 16])
def test_parity_with_the_plain_plan(P, op):
    """Every pointer of every rank ends with the plain plan's bytes, whatever
    the interleaving: ops x dtypes x P x k x n, three seeds each."""
    for dtype in ("f32", "f64", "bf16", "i32"):
        for k in (2, 3, 8, 9):
            for n in (1, 5, 1000, 4099):
                x = _inputs(dtype, op, P, k, n, seed=P * 131 + k * 17 + n)
                want = simulate("halving_doubling", op, dtype, x, seed=0)
                for seed in (1, 2, 3):
                    assert same(simulate(NAME, op, dtype, x, seed=seed), want), (dtype, k, n, seed)


def test_reference_golden(golden_sched):
    """The reference's own multi-pointer halving-doubling output."""
    case = "halving_doubling/sum/f32/P3/k3/n500"
    x, want = golden_sched[case + "/in"], golden_sched[case + "/out"]
    for seed in range(3):
        y = simulate(NAME, "sum", "f32", x, seed=seed)
        for r in range(x.shape[0]):
            for j in range(x.shape[1]):
                assert same(y[r, j], want), (seed, r, j)


def test_repeated_runs_stay_exact():
    """Back-to-back runs with no barrier between them: the per-range
    broadcasts of run r and the per-range reduces of run r + 1 never meet a
    message of the other run (no ProtocolError under any interleaving), and
    the third run's bytes are the plain plan's."""
    P, k, n = 6, 3, 1000
    x = np.random.default_rng(5).integers(-8, 9, (P, k, n)).astype(np.float32)
    for run in range(3):
        xs = x * np.float32(2.0 ** run)
        want = simulate("halving_doubling", "sum", "f32", xs, seed=0, runs=3)
        for seed in range(20 if run == 0 else 3):
            try:
                got = simulate(NAME, "sum", "f32", xs, seed=seed, runs=3)
            except ProtocolError as e:  # a finding, not an error of the test
                pytest.fail(f"seed {seed}: {e}")
            assert same(got, want), (run, seed)
    # integers this small stay exact: run 3 of the sum is k * P^3 ... closed form
    total = x.sum(axis=(0, 1))
    y = simulate(NAME, "sum", "f32", x, seed=7, runs=1)
    assert (y == total).all()


def test_mesh_form_is_refused():
    import gloo_amd
    for P in (2, 4, 8):
        rc, _ = plan_rc(HDP | plan_sim.MESH, 0, P, 1000, 2)
        assert rc == EINVAL_ARG
        if plan_sim.plan_lib() is gloo_amd.lib:  # (a host-only planner build has no error text)
            assert b"mesh" in gloo_amd.lib.gloo_hip_last_error()
    assert plan_rc(1 | plan_sim.MESH, 0, 4, 1000, 2)[0] == 0  # HALVING_DOUBLING keeps its mesh form


def test_python_enum_names_it():
    import gloo_amd
    assert gloo_amd.ALGORITHMS[NAME] == HDP
    assert gloo_amd.ALGORITHMS["halving_doubling"] == 1


def emitted_interp_steps(steps, k, sliced):
    """What executor_run.cc buildInterp pushes for this plan (built-in op, all
    pointers local): the three fusions and the multi-destination broadcast."""
    cuts = user_cuts(steps) if sliced else []
    groups = lambda ndst: -(-ndst // (1 + MAX_XDST))
    total, i = 0, 0
    while i < len(steps):
        t = steps[i]
        K = t.kind
        nxt = steps[i + 1] if i + 1 < len(steps) else None
        nn = steps[i + 2] if i + 2 < len(steps) else None
        if (K == KIND["LOCAL_REDUCE"] and t.length and nn is not None and nxt.kind == KIND["WAIT_RECV"]
                and nn.kind == KIND["REDUCE"] and nn.flags == SRC_ARENA and (nn.dst_off, nn.length) == (t.dst_off, t.length)
                and 2 <= k and k + 1 <= MAX_SRCS and len(cut_range(cuts, t.dst_off, t.length)) == 1):
            total += 2  # wait, fold
            i += 3
            continue
        if (K == KIND["COPY"] and t.flags == SRC_ARENA and t.length and k >= 2 and nxt is not None
                and nxt.kind == KIND["LOCAL_BCAST"] and nxt.dst_off <= t.dst_off
                and t.dst_off + t.length <= nxt.dst_off + nxt.length):
            pcs = cut_range(sorted(set(cuts) | {t.dst_off, t.dst_off + t.length}), nxt.dst_off, nxt.length)
            if (t.dst_off, t.length) in pcs:
                total += sum(groups(k) if pc == (t.dst_off, t.length) else groups(k - 1) for pc in pcs)
                i += 2
                continue
        if K in (KIND["DECL_RECV"], KIND["WAIT_SEND"], KIND["FOLD_SRC"]):
            pass
        elif K == KIND["LOCAL_REDUCE"]:
            per = 1 if k <= MAX_SRCS else 1 + -(-(k - MAX_SRCS) // (MAX_SRCS - 1))
            total += len(cut_range(cuts, t.dst_off, t.length)) * per
        elif K == KIND["LOCAL_BCAST"]:
            total += len(cut_range(cuts, t.dst_off, t.length)) * groups(k - 1)
        else:
            total += 1
        i += 1
    return total


@pytest.mark.parametrize("P", [2, 3, 4, 6, 8, 13])
def test_sliced_step_bound_covers_the_emitted_list(P):
    """slicedInterpSteps (plan_sim.sliced_interp_steps is its statement) stays
    an upper bound of the device step list for plans with sub-range local
    steps, sliced or not, and fits the list's capacity at these sizes.

    Both sides here are Python statements: emitted_interp_steps restates
    buildInterp's lowering as designed, plan_sim.sliced_interp_steps restates
    the C++ bound (the hook tests/test_sliced.py uses).  So this checks the
    design's arithmetic, not the C++: a change of buildInterp alone cannot fail
    it.  The check of the C++ itself is buildInterp's own enforcement that a
    sliced list fits its proposed bound, which the sliced job of
    tests/test_hd_pipelined_gpu.py (P = 2, n = 65536) runs into."""
    for k in (2, 4, 8, 9, 12):
        for n in (1, 1000, 100_003):
            for r in range(P):
                steps = plan(HDP, r, P, n, k)
                bound = sliced_interp_steps(NAME, P, n, r, k=k)
                for sliced in (False, True):
                    assert emitted_interp_steps(steps, k, sliced) <= bound, (k, n, r, sliced)
                assert bound <= plan_sim.INTERP_MAX_STEPS


def test_sliceable_rule_handles_sub_range_local_steps():
    """sliceable / userCuts take local steps that are not cut from [0, n).  At
    two ranks every local range is exactly a message range, so the plan may
    run sliced, and sliced execution keeps the bytes; with more in-block steps
    the first receive's range is cut further by later steps and the rule
    refuses, as it does for the plain plan.  (An odd n is refused for both at
    any P: the two halves' messages share inbox bytes at different lengths.)"""
    k, n = 3, 4096
    assert all(sliceable(NAME, 2, n, r, k=k) for r in range(2))
    x = np.random.default_rng(11).standard_normal((2, k, n)).astype(np.float32)
    want = simulate("halving_doubling", "sum", "f32", x, seed=0)
    for slices, seed in ((2, 0), (3, 1), (7, 2)):
        assert same(simulate(NAME, "sum", "f32", x, seed=seed, slices=slices), want), slices
    for P in (4, 8):
        assert [sliceable(NAME, P, n, r, k=k) for r in range(P)] == \
            [sliceable("halving_doubling", P, n, r, k=k) for r in range(P)]


# ---- the batching rule with multi-destination copies -----------------------

class _Desc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("nsrc", ctypes.c_int32), ("dst", ctypes.c_uint64),
                ("src", ctypes.c_uint64 * MAX_SRCS), ("bytes", ctypes.c_uint64)]


class _DescEx(ctypes.Structure):
    _fields_ = [("step", _Desc), ("nxdst", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("xdst", ctypes.c_uint64 * MAX_XDST)]


def _batches_ex(steps):
    """steps: [(kind, dst, [srcs], bytes, [xdsts])] -> (status, defer flags)."""
    import gloo_amd
    arr = (_DescEx * len(steps))()
    for d, (kind, dst, srcs, nbytes, xd) in zip(arr, steps):
        d.step.kind, d.step.nsrc, d.step.dst, d.step.bytes = kind, len(srcs), dst, nbytes
        for j, a in enumerate(srcs):
            d.step.src[j] = a
        d.nxdst = len(xd)
        for j, a in enumerate(xd):
            d.xdst[j] = a
    out = (ctypes.c_int * len(steps))()
    gloo_amd.lib.gloo_hip_interp_batches_ex.argtypes = [ctypes.POINTER(_DescEx), ctypes.c_int,
                                                        ctypes.POINTER(ctypes.c_int)]
    rc = gloo_amd.lib.gloo_hip_interp_batches_ex(arr, len(steps), out)
    return rc, list(out)


def test_batching_counts_every_destination_as_written():
    """Two steps that meet only through an extra destination of the first must
    not share a drain (gloo_hip_interp_batches_ex, markInterpBatches)."""
    COPY, SEND, FOLD = 0, 1, 4
    A, B, C, D, E, F = (0x10000 * i for i in range(1, 7))
    n = 256
    # independent: the broadcast's destinations and the next copy are disjoint
    assert _batches_ex([(COPY, B, [A], n, [C, D]), (COPY, F, [E], n, [])]) == (0, [1, 0])
    # the next step READS an extra destination (a send of the range just broadcast)
    assert _batches_ex([(COPY, B, [A], n, [C, D]), (SEND, F, [D], n, [])]) == (0, [0, 0])
    assert _batches_ex([(COPY, B, [A], n, [C, D]), (FOLD, F, [E, C + n - 1], n, [])]) == (0, [0, 0])
    # the next step WRITES an extra destination, or an extra destination overwrites what the batch read
    assert _batches_ex([(COPY, B, [A], n, [C, D]), (COPY, D + 8, [E], n, [])]) == (0, [0, 0])
    assert _batches_ex([(COPY, F, [E], n, []), (COPY, B, [A], n, [C, E + n - 1])]) == (0, [0, 0])
    # ... also through a step in between that touches nothing (the open batch, not only the neighbour)
    assert _batches_ex([(COPY, B, [A], n, [C, D]), (COPY, F, [E], n, []), (SEND, 0x90000, [D], n, [])]) == \
        (0, [1, 0, 0])
    # adjacent but not overlapping: still one batch
    assert _batches_ex([(COPY, B, [A], n, [C]), (COPY, C + n, [E], n, [])]) == (0, [1, 0])
    # extra destinations belong to copies only, at most MAX_XDST of them
    assert _batches_ex([(SEND, B, [A], n, [C])])[0] == EINVAL_ARG
    assert _batches_ex([(FOLD, B, [A, E], n, [C])])[0] == EINVAL_ARG
