"""CPU: the alltoall plan (GLOO_HIP_ALGO_ALLTOALL = 14; gloo::alltoall and
gloo::alltoallv) against its closed-form model, on the simulator of
tests/alltoall_sim.py: three consecutive runs with a payload each and no
barrier between them, under several interleavings.  Also the plan's shape
(every SEND has a DECL_RECV of equal length, the arena is the output's size),
the planner's refusals and the steps == NULL form of gloo_hip_plan_ex.
"""
import ctypes

import numpy as np
import pytest

import alltoall_sim as sim
import plan_sim
from plan_sim import KIND, FROM_INPUTS, SRC_ARENA, PREV_RUN, MESH

SIZES = (1, 2, 3, 5, 8)
RUNS = 3


def ragged(P, seed):
    """A P x P matrix with zero-length blocks, a rank that sends nothing
    (row P - 1 at P > 1) and one that receives nothing from its peers."""
    rng = np.random.default_rng(seed)
    M = rng.integers(0, 40, (P, P))
    M[rng.random((P, P)) < 0.3] = 0
    if P > 1:
        M[P - 1, :] = 0
    if P > 2:
        M[:, 1] = 0
        M[1, 1] = 7  # ... but keeps its own block
    return [[int(v) for v in row] for row in M]


def payloads(M, seed):
    rng = np.random.default_rng(seed)
    out = []
    for run in range(RUNS):
        per = []
        for row in M:
            b = rng.integers(0, 256, sum(row), dtype=np.uint8)
            b[b == sim.SENTINEL] = run
            per.append(b)
        out.append(per)
    return out


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("count", [1, 17])
def test_even_form(P, count):
    M = sim.even(P, count)
    for seed in range(4):
        sim.simulate(M, payloads(M, seed), seed=seed, even_count=count)


@pytest.mark.parametrize("P", SIZES)
def test_even_form_equals_its_counts(P):
    """recv_elems NULL is `count` everywhere (alltoall.cc:29-30)."""
    M = sim.even(P, 5)
    for (a, aa), (b, ba) in zip(sim.plans(M, even_count=5), sim.plans(M)):
        assert aa == ba and [bytes(s) for s in a] == [bytes(s) for s in b]


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_ragged_forms(P, which):
    M = ragged(P, 10 * P + which)
    for seed in range(4):
        sim.simulate(M, payloads(M, seed), seed=seed)


def test_all_zero():
    M = [[0, 0], [0, 0]]
    for steps, arena in sim.plans(M):
        assert steps == [] and arena == 0


def test_the_credit_wait_is_what_orders_the_runs():
    """With the previous-run credit taken as met, some interleaving sends
    onto a block that has not been copied out: the simulator sees it."""
    M = sim.even(3, 4)
    with pytest.raises(plan_sim.ProtocolError, match="not copied out"):
        for seed in range(50):
            sim.simulate(M, payloads(M, seed), seed=seed, even_count=4, drop_credit_wait=True)


@pytest.mark.parametrize("P", SIZES)
def test_shape(P):
    M = ragged(P, P)
    pl = sim.plans(M)
    for r, (steps, arena) in enumerate(pl):
        outc = [M[q][r] for q in range(P)]
        in_off, out_off = sim.prefix(M[r]), sim.prefix(outc)
        assert arena == (sum(outc) if P > 1 else 0)
        kinds = [s.kind for s in steps]
        decl = {s.peer: s for s in steps if s.kind == KIND["DECL_RECV"]}
        assert set(decl) == {q for q in range(P) if q != r and outc[q] > 0}
        for q, d in decl.items():
            assert (d.dst_off, d.length) == (out_off[q], outc[q])
        own = [s for s in steps if s.kind == KIND["COPY"] and s.flags == FROM_INPUTS]
        assert len(own) == (1 if M[r][r] else 0)
        for s in own:
            assert (s.dst_off, s.src_off, s.length) == (out_off[r], in_off[r], M[r][r])
        sends = [s for s in steps if s.kind == KIND["SEND"]]
        assert [s.peer for s in sends] == [(r + d) % P for d in range(1, P) if M[r][(r + d) % P] > 0]
        for s in sends:
            assert s.flags == FROM_INPUTS and (s.src_off, s.length, s.dst_off) == (in_off[s.peer], M[r][s.peer], 0)
            theirs = [d for d in pl[s.peer][0] if d.kind == KIND["DECL_RECV"] and d.peer == r]
            assert len(theirs) == 1 and theirs[0].length == s.length
            i = steps.index(s)
            w = steps[i - 1]
            assert w.kind == KIND["WAIT_NOTIFY"] and w.flags & PREV_RUN and w.peer == s.peer
        waits = [s.peer for s in steps if s.kind == KIND["WAIT_RECV"]]
        assert waits == [(r - d) % P for d in range(1, P) if outc[(r - d) % P] > 0]
        outs = [s for s in steps if s.kind == KIND["COPY"] and s.flags == SRC_ARENA]
        assert [(s.dst_off, s.src_off, s.length) for s in outs] == [(out_off[q], out_off[q], outc[q]) for q in waits]
        assert [s.peer for s in steps if s.kind == KIND["NOTIFY"]] == waits
        # the order of the phases
        order = [KIND[k] for k in ("DECL_RECV", "COPY", "WAIT_NOTIFY", "WAIT_RECV", "COPY", "NOTIFY", "WAIT_SEND")]
        squeezed = [k for i, k in enumerate(kinds) if i == 0 or kinds[i - 1] != k]
        squeezed = [k for k in squeezed if k != KIND["SEND"]]
        squeezed = [k for i, k in enumerate(squeezed) if i == 0 or squeezed[i - 1] != k]
        it = iter(order)
        assert all(any(k == o for o in it) for k in squeezed), squeezed
    if P == 1:
        assert len(pl[0][0]) == (1 if M[0][0] else 0)


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


def test_null_steps_fills_only_the_count():
    rc, n, arena, _ = plan_ex(sim.ALLTOALL, 1, 4, 6, 1, 1, None)
    steps, a = plan_sim.get_plan("alltoall", 1, 4, 6, 1, nin=1, elem_size=1)
    assert rc == 0 and n == len(steps) == 3 + 1 + 6 + 3 + 3 + 3 + 3 and arena == a == 24


@pytest.mark.parametrize("args, word", [
    ((sim.ALLTOALL, 0, 2, 4, 0, 1, None), "not 0"),                   # ninputs != 1
    ((sim.ALLTOALL, 0, 2, 4, 2, 1, None), "not 2"),
    ((sim.ALLTOALL, 0, 2, 4, 1, 2, None), "not 2"),                   # noutputs != 1
    ((sim.ALLTOALL, 0, 2, 0, 1, 1, [3, -5, 3, 1]), "-5"),             # a negative in_count
    ((sim.ALLTOALL, 0, 2, 0, 1, 1, [3, 5, 3, -7]), "-7"),             # a negative out_count
    ((sim.ALLTOALL, 1, 2, 0, 1, 1, [3, 5, 3, 6]), "in_count 5 but out_count 6"),  # in[rank] != out[rank]
    ((sim.ALLTOALL | MESH, 0, 2, 4, 1, 1, None), str(sim.ALLTOALL | MESH)),
])
def test_refusals(args, word):
    rc, n, arena, msg = plan_ex(*args)
    assert rc == EINVAL_ARG, (rc, msg)
    assert "alltoall" in msg and word in msg, msg


def test_short_form_takes_the_even_form_only():
    L = plan_sim.plan_lib()
    L.gloo_hip_last_error.restype = ctypes.c_char_p
    L.gloo_hip_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    n, arena = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.gloo_hip_plan(sim.ALLTOALL, 0, 3, 5, 1, None, None, 0, ctypes.byref(n), ctypes.byref(arena)) == 0
    assert (n.value, arena.value) == (len(plan_sim.get_plan("alltoall", 0, 3, 5, 1, nin=1, elem_size=1)[0]), 15)
    rp = (ctypes.c_int * 6)(1, 1, 1, 1, 1, 1)
    assert L.gloo_hip_plan(sim.ALLTOALL, 0, 3, 5, 1, rp, None, 0, ctypes.byref(n), ctypes.byref(arena)) == EINVAL_ARG
    assert b"even form only" in L.gloo_hip_last_error()
