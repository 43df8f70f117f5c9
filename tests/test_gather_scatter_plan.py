"""CPU: the gather and scatter plans (GLOO_HIP_ALGO_GATHER = 15, gloo::gather /
gloo::gatherv; GLOO_HIP_ALGO_SCATTER = 16, gloo::scatter) against their
closed-form models, on the simulator of tests/rooted_sim.py: three consecutive
runs with a payload each and no barrier between them, under several
interleavings.  Also the plans' shape (the order of the phases, every SEND has
a DECL_RECV of equal length, the arena sizes, which input a step names), the
planner's refusals, and the negative control: without the credit / the
clear-to-send the simulator sees an inbox overwritten.
"""
import ctypes
import types

import numpy as np
import pytest

import plan_sim
import rooted_sim as sim
from plan_sim import KIND, FROM_INPUTS, SRC_ARENA, PREV_RUN, MESH

SIZES = (1, 2, 3, 5, 8, 9)
RUNS = 3
SLOT_DATA0, SLOT_NOTIFY = 0, 2


def roots(P):
    return list(range(P)) if P <= 3 else [0, P - 1]


CASES = [(P, root) for P in SIZES for root in roots(P)]


def ragged(P, root, seed):
    """Per-rank counts with empty blocks: rank 0's (the root's own block when
    root == 0) and, at P > 2, one more peer's; one odd-sized block."""
    rng = np.random.default_rng(seed)
    c = [int(v) for v in rng.integers(1, 40, P)]
    c[0] = 0
    if P > 2:
        c[(root + 1) % P] = 0
    if P > 1:
        c[P - 1] = 33
    return c


def gather_payloads(P, lens, seed):
    rng = np.random.default_rng(seed)
    out = []
    for run in range(RUNS):
        per = []
        for q in range(P):
            b = rng.integers(0, 256, lens[q], dtype=np.uint8)
            b[b == sim.SENTINEL] = run
            per.append(b)
        out.append(per)
    return out


@pytest.mark.parametrize("P, root", CASES)
@pytest.mark.parametrize("count", [1, 17])
def test_gather_even(P, root, count):
    for seed in range(4):
        sim.simulate("gather", P, root, gather_payloads(P, [count] * P, seed), count=count, seed=seed)


@pytest.mark.parametrize("P, root", CASES)
@pytest.mark.parametrize("which", [0, 1])
def test_gatherv_ragged(P, root, which):
    counts = ragged(P, root, 10 * P + which)
    for seed in range(4):
        sim.simulate("gather", P, root, gather_payloads(P, counts, seed), counts=counts, seed=seed)


@pytest.mark.parametrize("P, root", CASES)
def test_gatherv_with_equal_counts_is_the_even_form(P, root):
    for (a, aa), (b, ba) in zip(sim.gather_plans(P, root, count=5), sim.gather_plans(P, root, counts=[5] * P)):
        assert aa == ba and [bytes(s) for s in a] == [bytes(s) for s in b]


@pytest.mark.parametrize("P, root", CASES)
@pytest.mark.parametrize("count", [1, 17])
def test_scatter(P, root, count):
    for seed in range(4):
        sim.simulate("scatter", P, root, gather_payloads(P, [count] * P, seed), count=count, seed=seed)


def test_nothing_to_move():
    for steps, arena in sim.gather_plans(3, 1, counts=[0, 0, 0]) + sim.gather_plans(3, 1, count=0) + \
            sim.scatter_plans(3, 1, 0):
        assert steps == [] and arena == 0


def without_waits(plans):
    return [([s for s in steps if s.kind != KIND["WAIT_NOTIFY"]], arena) for steps, arena in plans]


def test_the_gather_credit_is_what_orders_the_runs():
    """With the previous-run credit removed from a copy of the step lists,
    some interleaving sends onto a block the root has not copied out."""
    P, root, count = 3, 1, 4
    stripped = without_waits(sim.gather_plans(P, root, count=count))
    assert sum(len(s) for s, _ in stripped) == sum(len(s) for s, _ in sim.gather_plans(P, root, count=count)) - (P - 1)
    with pytest.raises(plan_sim.ProtocolError, match="not copied out"):
        for seed in range(50):
            sim.simulate("gather", P, root, gather_payloads(P, [count] * P, seed), count=count, seed=seed,
                         drop_wait=True, plans=stripped)


def test_the_scatter_clear_to_send_is_what_orders_the_runs():
    P, root, count = 3, 0, 4
    stripped = without_waits(sim.scatter_plans(P, root, count))
    with pytest.raises(plan_sim.ProtocolError, match="not copied out"):
        for seed in range(50):
            sim.simulate("scatter", P, root, gather_payloads(P, [count] * P, seed), count=count, seed=seed,
                         drop_wait=True, plans=stripped)


def squeeze(kinds):
    return [k for i, k in enumerate(kinds) if i == 0 or kinds[i - 1] != k]


@pytest.mark.parametrize("P, root", CASES)
def test_gather_shape(P, root):
    counts = ragged(P, root, P)
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    pl = sim.gather_plans(P, root, counts=counts)
    for r, (steps, arena) in enumerate(pl):
        kinds = [s.kind for s in steps]
        if r != root:
            assert arena == 0
            if counts[r] == 0:
                assert steps == []
                continue
            assert kinds == [KIND["WAIT_NOTIFY"], KIND["SEND"], KIND["WAIT_SEND"]]
            w, s, ws = steps
            assert (w.peer, w.slot, w.flags) == (root, SLOT_NOTIFY, PREV_RUN)
            assert (s.peer, s.slot, s.flags, s.dst_off, s.src_off, s.length) == \
                (root, SLOT_DATA0, FROM_INPUTS, 0, 0, counts[r])
            assert (ws.peer, ws.slot) == (root, SLOT_DATA0)
            theirs = [d for d in pl[root][0] if d.kind == KIND["DECL_RECV"] and d.peer == r]
            assert len(theirs) == 1 and theirs[0].length == s.length and theirs[0].slot == s.slot
            continue
        peers = [q for q in range(P) if q != root and counts[q] > 0]
        assert arena == (off[P] if P > 1 else 0)
        decl = [s for s in steps if s.kind == KIND["DECL_RECV"]]
        assert [(d.peer, d.slot, d.dst_off, d.length) for d in decl] == [(q, SLOT_DATA0, off[q], counts[q]) for q in peers]
        own = [s for s in steps if s.kind == KIND["COPY"] and s.flags == FROM_INPUTS]
        assert [(s.dst_off, s.src_off, s.length) for s in own] == ([(off[root], 0, counts[root])] if counts[root] else [])
        assert [s.peer for s in steps if s.kind == KIND["WAIT_RECV"]] == peers
        outs = [s for s in steps if s.kind == KIND["COPY"] and s.flags == SRC_ARENA]
        assert [(s.dst_off, s.src_off, s.length) for s in outs] == [(off[q], off[q], counts[q]) for q in peers]
        notes = [s for s in steps if s.kind == KIND["NOTIFY"]]
        assert [(s.peer, s.slot) for s in notes] == [(q, SLOT_NOTIFY) for q in peers]
        assert len(steps) == len(decl) + len(own) + 3 * len(peers)
        # the order of the phases: DECL_RECVs, the own block, the waits, the copy-outs, the credits
        want = [KIND[k] for k in ("DECL_RECV", "COPY", "WAIT_RECV", "COPY", "NOTIFY")]
        it = iter(want)
        assert all(any(k == o for o in it) for k in squeeze(kinds)), kinds
        if own and peers:
            assert kinds.index(KIND["COPY"]) < kinds.index(KIND["WAIT_RECV"])


@pytest.mark.parametrize("P, root", CASES)
def test_scatter_shape(P, root):
    count = 6
    pl = sim.scatter_plans(P, root, count)
    for r, (steps, arena) in enumerate(pl):
        kinds = [s.kind for s in steps]
        if r != root:
            assert arena == count
            assert kinds == [KIND[k] for k in ("DECL_RECV", "NOTIFY", "WAIT_RECV", "COPY")]
            d, n, w, c = steps
            assert (d.peer, d.slot, d.dst_off, d.length) == (root, SLOT_DATA0, 0, count)
            assert (n.peer, n.slot) == (root, SLOT_NOTIFY) and (w.peer, w.slot) == (root, SLOT_DATA0)
            assert (c.flags, c.dst_off, c.src_off, c.length) == (SRC_ARENA, 0, 0, count)
            continue
        peers = [q for q in range(P) if q != root]
        assert arena == 0
        want = []
        for q in peers:
            want += [(KIND["WAIT_NOTIFY"], q, SLOT_NOTIFY, 0, 0),
                     (KIND["SEND"], q, SLOT_DATA0, FROM_INPUTS | q << sim.INPUT_SHIFT, count)]
        want += [(KIND["COPY"], -1, 0, FROM_INPUTS | root << sim.INPUT_SHIFT, count)]
        want += [(KIND["WAIT_SEND"], q, SLOT_DATA0, 0, 0) for q in peers]
        assert [(s.kind, s.peer, s.slot, s.flags, s.length) for s in steps] == want
        assert all(s.dst_off == 0 and s.src_off == 0 for s in steps)
        assert [sim.input_of(s.flags) for s in steps if s.kind == KIND["SEND"]] == peers


def test_plans_that_know_one_input_leave_the_input_bits_clear():
    """The extension of GLOO_HIP_FROM_INPUTS changes no step an existing plan emits."""
    for algo, kw in (("reduce", dict(recv=[1], nin=1)), ("allreduce_new", dict(nin=1))):
        for r in range(4):
            steps, _ = plan_sim.get_plan(algo, r, 4, 1000, 1, elem_size=4, **kw)
            assert steps and all(s.flags >> sim.INPUT_SHIFT == 0 for s in steps)
    for r in range(3):
        steps, _ = plan_sim.get_plan("gather", r, 3, 9, 1 if r == 0 else 0, recv=[0], nin=1, elem_size=1)
        assert all(s.flags >> sim.INPUT_SHIFT == 0 for s in steps)


def plan_ex(algo, rank, size, count, nin, nout, recv):
    L = plan_sim.plan_lib()
    L.gloo_hip_last_error.restype = ctypes.c_char_p
    n, arena = ctypes.c_size_t(99), ctypes.c_size_t(99)
    rp = None
    if recv is not None:
        rp = (ctypes.c_int * len(recv))(*recv)
    L.gloo_hip_plan_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                   ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                   ctypes.POINTER(ctypes.c_size_t)]
    rc = L.gloo_hip_plan_ex(algo, rank, size, count, nin, nout, 1, 0, rp, None, 0, ctypes.byref(n),
                            ctypes.byref(arena))
    return rc, n.value, arena.value, (L.gloo_hip_last_error() or b"").decode()


EINVAL_ARG = -4  # include/gloo_amd.h GLOO_HIP_EINVAL_ARG
PER_RANK = sim.COUNT_PER_RANK


def test_null_steps_fills_only_the_count():
    rc, n, arena, _ = plan_ex(sim.GATHER, 1, 4, 6, 1, 1, [1])
    assert (rc, n, arena) == (0, 3 + 1 + 3 + 3 + 3, 24)
    rc, n, arena, _ = plan_ex(sim.SCATTER, 1, 4, 6, 4, 1, [1])
    assert (rc, n, arena) == (0, 6 + 1 + 3, 0)
    rc, n, arena, _ = plan_ex(sim.SCATTER, 2, 4, 6, 0, 1, [1])
    assert (rc, n, arena) == (0, 4, 6)


@pytest.mark.parametrize("args, words", [
    ((sim.GATHER, 0, 2, 4, 1, 1, [2]), ("gather", "root rank 2")),                # a root outside [0, size)
    ((sim.GATHER, 0, 2, 4, 1, 0, [-1]), ("gather", "root rank -1")),
    ((sim.GATHER, 0, 2, PER_RANK, 1, 1, [0, 3, -5]), ("gather", "-5", "rank 1")),  # a negative count
    ((sim.GATHER, 0, 2, 4, 1, 1, None), ("gather", "NULL")),                      # no recv_elems at all
    ((sim.GATHER, 0, 2, 4, 0, 1, [0]), ("gather", "not 0")),                      # ninputs != 1
    ((sim.GATHER, 0, 2, 4, 2, 1, [0]), ("gather", "not 2")),
    ((sim.GATHER, 0, 2, 4, 1, 0, [0]), ("gather", "0 outputs", "root")),          # a root without an output
    ((sim.GATHER, 1, 2, 4, 1, 2, [0]), ("gather", "2 outputs")),
    ((sim.GATHER | MESH, 0, 2, 4, 1, 1, [0]), ("gather", str(sim.GATHER | MESH))),
    ((sim.SCATTER, 0, 2, 4, 2, 1, [2]), ("scatter", "root rank 2")),
    ((sim.SCATTER, 0, 2, 4, 2, 1, [-3]), ("scatter", "root rank -3")),
    ((sim.SCATTER, 0, 2, 4, 2, 1, None), ("scatter", "NULL")),
    ((sim.SCATTER, 0, 2, 4, 2, 0, [0]), ("scatter", "not 0")),                    # noutputs != 1
    ((sim.SCATTER, 0, 2, 4, 1, 1, [0]), ("scatter", "not 1")),                    # the root's inputs != size
    ((sim.SCATTER | MESH, 0, 2, 4, 2, 1, [0]), ("scatter", str(sim.SCATTER | MESH))),
])
def test_refusals(args, words):
    rc, n, arena, msg = plan_ex(*args)
    assert rc == EINVAL_ARG, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_a_rank_that_is_not_the_root_may_state_no_output_or_one():
    a = plan_ex(sim.GATHER, 1, 3, 4, 1, 0, [0])
    b = plan_ex(sim.GATHER, 1, 3, 4, 1, 1, [0])
    assert a[0] == 0 and a[:3] == b[:3] == (0, 3, 0)


def test_a_count_list_of_the_wrong_length_is_refused_where_the_length_is_known():
    """A C pointer carries no length: gloo_hip_plan_ex reads {root} or, with
    count == GLOO_HIP_COUNT_PER_RANK, {root, size counts}.  The front ends
    that know the length refuse a wrong one before any call into the library."""
    import gloo_amd
    ctx = types.SimpleNamespace(size=3, rank=0, _h=None)
    with pytest.raises(gloo_amd.GlooHipError, match="2 per-rank counts for 3 ranks"):
        gloo_amd.gather(ctx, 1, 0, "u8", 0, output=1, counts=[1, 2])
    with pytest.raises(gloo_amd.GlooHipError, match="negative count -2 for rank 1"):
        gloo_amd.gather(ctx, 1, 0, "u8", 0, output=1, counts=[1, -2, 3])
    with pytest.raises(gloo_amd.GlooHipError, match="recv_elems has 3 entries"):
        gloo_amd.Algorithm(ctx, "gather", "sum", "u8", [1, 2], 0, recv_elems=[0, 1, 2])
    with pytest.raises(gloo_amd.GlooHipError, match="recv_elems has 0 entries"):
        gloo_amd.Algorithm(ctx, "gather", "sum", "u8", [1, 2], 4)
    with pytest.raises(gloo_amd.GlooHipError, match="recv_elems has 2 entries"):
        gloo_amd.Algorithm(ctx, "scatter", "sum", "u8", [1], 4, recv_elems=[0, 4])
    with pytest.raises(gloo_amd.GlooHipError, match="2 inputs for 3 ranks"):
        gloo_amd.scatter(ctx, 1, 4, "u8", 0, inputs=[1, 2])


def test_short_form():
    L = plan_sim.plan_lib()
    L.gloo_hip_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    n, arena = ctypes.c_size_t(), ctypes.c_size_t()
    rp = (ctypes.c_int * 1)(2)
    # gather: {in} on a rank without an output, {in, out} on the root
    assert L.gloo_hip_plan(sim.GATHER, 0, 3, 5, 1, rp, None, 0, ctypes.byref(n), ctypes.byref(arena)) == 0
    assert (n.value, arena.value) == (3, 0)
    assert L.gloo_hip_plan(sim.GATHER, 2, 3, 5, 2, rp, None, 0, ctypes.byref(n), ctypes.byref(arena)) == 0
    assert (n.value, arena.value) == (2 + 1 + 6, 15)
    assert L.gloo_hip_plan(sim.GATHER, 2, 3, 5, 1, rp, None, 0, ctypes.byref(n), ctypes.byref(arena)) == EINVAL_ARG
    # scatter: {out} off the root, {out, in_0 ... in_{P-1}} on it
    assert L.gloo_hip_plan(sim.SCATTER, 0, 3, 5, 1, rp, None, 0, ctypes.byref(n), ctypes.byref(arena)) == 0
    assert (n.value, arena.value) == (4, 5)
    assert L.gloo_hip_plan(sim.SCATTER, 2, 3, 5, 4, rp, None, 0, ctypes.byref(n), ctypes.byref(arena)) == 0
    assert (n.value, arena.value) == (4 + 1 + 2, 0)
    assert L.gloo_hip_plan(sim.SCATTER, 2, 3, 5, 1, rp, None, 0, ctypes.byref(n), ctypes.byref(arena)) == EINVAL_ARG
