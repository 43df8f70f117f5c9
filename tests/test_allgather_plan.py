"""GLOO_HIP_ALGO_ALLGATHER (AllgatherRing, gloo::allgather / allgatherv) on the
CPU: the plans of gloo_hip_plan_ex simulated for all ranks
(tests/allgather_sim.py), their shape, and the refusals.

The model is closed form: after a run every rank's output holds block 0,
block 1, ... block P-1 back to back, block r being rank r's k inputs
concatenated.  Before the algorithm existed gloo_hip_plan_ex refused
algorithm 13, so every test here that plans one failed.
"""
import ctypes
import os

import numpy as np
import pytest

import allgather_sim
from allgather_sim import KIND
from plan_sim import PREV_RUN, SRC_ARENA, ProtocolError, Step, get_plan, plan_lib

EINVAL_ARG = -4
ALLGATHER = 13
MESH = 0x100
SIZES = (1, 2, 3, 5, 8, 13)
COUNTS = (0, 1, 17)
INPUTS = (1, 3, 0)  # k; 0 = in place
NOTIFY_SLOT, DATA0 = 2, 0
# per-rank counts with zeros, and one where a single rank contributes
RAGGED = {2: [[0, 5], [3, 0]], 3: [[2, 0, 9], [0, 0, 4]], 4: [[0, 17, 1, 5], [0, 0, 6, 0]],
          5: [[1, 0, 0, 17, 2]], 8: [[3, 0, 1, 0, 17, 0, 2, 5], [0, 0, 0, 0, 0, 9, 0, 0]],
          13: [[i % 4 for i in range(13)]]}


def make_payloads(rng, P, k, counts, runs=3):
    out = []
    for _ in range(runs):
        per_rank = []
        for r in range(P):
            arrs = [rng.integers(0, 256, counts[r], dtype=np.uint8) for _ in range(max(1, k))]
            for a in arrs:  # never the sentinel, so "still the sentinel" cannot pass
                a[a == allgather_sim.SENTINEL] = 0
            per_rank.append(arrs)
        out.append(per_rank)
    return out


def test_python_name_and_codes():
    import gloo_amd
    assert gloo_amd.ALGORITHMS["allgather"] == ALLGATHER
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gloo_amd.h")).read()
    assert "GLOO_HIP_ALGO_ALLGATHER = 13" in header and "GLOO_HIP_STEP_LOCAL_GATHER = 12" in header


@pytest.mark.parametrize("k", INPUTS)
@pytest.mark.parametrize("P", SIZES)
def test_three_runs_with_a_payload_each(P, k):
    """Every count: three runs back to back, a different payload per run, the
    whole output of every rank checked after each run, inputs unmodified, the
    ranks interleaved in several seeded random orders with no barrier."""
    rng = np.random.default_rng(P * 16 + k)
    for count in COUNTS:
        for seed in range(4):
            payloads = make_payloads(rng, P, k, [count] * P)
            allgather_sim.simulate(P, count, k, None, payloads, seed=seed + 10 * count)


@pytest.mark.parametrize("k", INPUTS)
@pytest.mark.parametrize("P", sorted(RAGGED))
def test_per_rank_counts_with_empty_blocks(P, k):
    rng = np.random.default_rng(P * 32 + k)
    for counts in RAGGED[P]:
        for seed in range(4):
            payloads = make_payloads(rng, P, k, counts)
            # `count` is ignored when counts are given
            allgather_sim.simulate(P, 999, k, counts, payloads, seed=seed)


def test_simulator_sees_a_send_onto_an_unread_inbox(monkeypatch):
    """The check the three-run tests rely on: without the credit wait a
    sender's next run overwrites the inbox of a receiver still in its
    previous run."""
    real = allgather_sim.plans

    def no_credit_wait(P, count, k, counts=None):
        return [([s for s in steps if s.kind != KIND["WAIT_NOTIFY"]], arena) for steps, arena in
                real(P, count, k, counts)]

    payloads = make_payloads(np.random.default_rng(1), 2, 1, [16, 16])
    for seed in range(40):  # the plan as planned never raises ...
        allgather_sim.simulate(2, 16, 1, None, payloads, seed=seed)
    monkeypatch.setattr(allgather_sim, "plans", no_credit_wait)
    seen = 0
    for seed in range(40):  # ... and without its credit wait some interleaving does
        try:
            allgather_sim.simulate(2, 16, 1, None, payloads, seed=seed)
        except ProtocolError as e:  # (an interleaving that misses the hazard ends with credits nobody awaited)
            seen += "not copied out" in str(e)
    assert seen > 0


def block_geometry(P, count, k, counts):
    c, off = allgather_sim.offsets(P, count, k, counts)
    return c, off, max(1, k)


@pytest.mark.parametrize("P", SIZES)
def test_step_shape_and_order(P):
    cases = [(count, None) for count in COUNTS] + [(0, c) for c in RAGGED.get(P, [])]
    for count, counts in cases:
        for k in INPUTS:
            c, off, kk = block_geometry(P, count, k, counts)
            for r in range(P):
                steps, arena = get_plan("allgather", r, P, count, 1, recv=counts, nin=k, elem_size=1)
                total = off[P]
                if total == 0 or (P == 1 and k == 0):
                    assert steps == [] and arena == 0
                    continue
                mine = kk * c[r]
                to = [(r + d) % P for d in range(1, P)] if mine else []
                frm = [q for q in ((r - d) % P for d in range(1, P)) if c[q]]
                want = [(KIND["DECL_RECV"], q) for q in frm]
                if k and mine:
                    want.append((KIND["LOCAL_GATHER"], -1))
                for q in to:
                    want += [(KIND["WAIT_NOTIFY"], q), (KIND["SEND"], q)]
                want += [(KIND["WAIT_RECV"], q) for q in frm] + [(KIND["COPY"], -1) for q in frm]
                want += [(KIND["NOTIFY"], q) for q in frm] + [(KIND["WAIT_SEND"], q) for q in to]
                assert [(s.kind, s.peer) for s in steps] == want, (P, r, k, count, counts)
                assert arena == (total if P > 1 else 0)
                sends = [s for s in steps if s.kind == KIND["SEND"]]
                assert len(sends) == (P - 1 if mine else 0)
                for s in sends:
                    assert (s.slot, s.flags, s.dst_off, s.src_off, s.length) == (DATA0, 0, 0, off[r], mine)
                for s in steps:
                    if s.kind == KIND["WAIT_NOTIFY"]:
                        assert s.slot == NOTIFY_SLOT and s.flags == PREV_RUN
                    elif s.kind == KIND["NOTIFY"]:
                        assert s.slot == NOTIFY_SLOT
                    elif s.kind == KIND["LOCAL_GATHER"]:
                        assert (s.dst_off, s.length) == (off[r], c[r])
                    elif s.kind == KIND["DECL_RECV"]:
                        assert (s.slot, s.dst_off, s.length) == (DATA0, off[s.peer], kk * c[s.peer])
                copies = [s for s in steps if s.kind == KIND["COPY"]]
                assert [(s.flags, s.dst_off, s.src_off, s.length) for s in copies] == \
                    [(SRC_ARENA, off[q], off[q], kk * c[q]) for q in frm]


def plan_rc(algo, rank, size, count, nin, nout, recv):
    L = plan_lib()
    n, arena = ctypes.c_size_t(), ctypes.c_size_t()
    rp = None
    if recv is not None:
        rp = (ctypes.c_int * len(recv))(*recv)
    L.gloo_hip_plan_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                   ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                   ctypes.POINTER(ctypes.c_size_t)]
    return L.gloo_hip_plan_ex(algo, rank, size, count, nin, nout, 1, 0, rp, None, 0, ctypes.byref(n),
                              ctypes.byref(arena))


def last_error():
    import gloo_amd
    return gloo_amd.lib.gloo_hip_last_error().decode()


def test_refusals():
    assert plan_rc(ALLGATHER, 0, 2, 4, 1, 1, None) == 0
    assert plan_rc(ALLGATHER | MESH, 0, 2, 4, 1, 1, None) == EINVAL_ARG
    assert str(ALLGATHER | MESH) in last_error() and "mesh" in last_error()
    assert plan_rc(ALLGATHER, 0, 3, 4, 1, 1, [4, -7, 2]) == EINVAL_ARG
    assert "-7" in last_error()
    assert plan_rc(ALLGATHER, 0, 2, 4, 1, 2, None) == EINVAL_ARG     # one output
    assert plan_rc(ALLGATHER, 0, 2, 4, -1, 1, None) == EINVAL_ARG    # a negative input count
    assert plan_rc(ALLGATHER, 2, 2, 4, 1, 1, None) == EINVAL_ARG     # rank outside the group


def test_algorithm_entry_points_refuse_the_mesh_flag_before_any_exchange():
    """Refused on the calling rank, before anything that needs a peer or a GPU."""
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:allgather_plan_refusals")
    try:
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.Algorithm(ctx, ALLGATHER | MESH, 0, "u8", [0x1000, 0x2000], 4)
        assert e.value.code == EINVAL_ARG and str(ALLGATHER | MESH) in str(e.value)
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.Algorithm(ctx, "allgather", 0, "u8", [0x1000, 0x2000], 4, recv_elems=[4])
        assert e.value.code == EINVAL_ARG and "recv_elems" in str(e.value)
    finally:
        ctx.close()
