"""GLOO_HIP_ALGO_BROADCAST (CudaBroadcastOneToAll's twin) on the CPU: the
plans of gloo_hip_plan simulated for all ranks (tests/broadcast_sim.py), their
shape, the refusals, and the interpreter's batching of a lowered broadcast.

The model is closed form: after a run every pointer of every rank holds the
bytes the root's root pointer held.  Before the algorithm existed,
gloo_hip_plan refused algorithm 12, so every test here that plans one failed.
"""
import ctypes

import numpy as np
import pytest

import broadcast_sim
from plan_sim import KIND, ProtocolError, Step, get_plan

EINVAL_ARG = -4
BROADCAST = 12
MESH = 0x100
SIZES = (1, 2, 3, 5, 8, 12)
COUNTS = (0, 1, 7, 1000)


def plan(rank, P, count, nptrs=1, root=0, root_pointer=0):
    return get_plan("broadcast", rank, P, count, nptrs, recv=[root, root_pointer], elem_size=1)


def kinds(steps):
    return [s.kind for s in steps]


def test_python_name_and_code():
    import gloo_amd
    assert gloo_amd.ALGORITHMS["broadcast"] == BROADCAST


@pytest.mark.parametrize("nptrs", (1, 3))
@pytest.mark.parametrize("P", SIZES)
def test_three_runs_with_a_payload_each(P, nptrs):
    """Every root, count and root pointer: three runs back to back, a
    different payload per run, every pointer of every rank checked after each
    run (a stale inbox or pointer of run r - 1 would show), the ranks
    interleaved at random with no barrier between runs."""
    rng = np.random.default_rng(P * 16 + nptrs)
    for root in range(P):
        for count in COUNTS:
            for rp in range(nptrs):
                payloads = [rng.integers(0, 256, count, dtype=np.uint8) for _ in range(3)]
                for p in payloads:  # never the sentinel, so "still the sentinel" cannot pass
                    p[p == broadcast_sim.SENTINEL] = 0
                broadcast_sim.simulate(P, count, nptrs, root, rp, payloads, seed=root * 7 + rp)


def test_simulator_sees_a_send_onto_an_unread_inbox(monkeypatch):
    """The check the three-run test relies on: a root that does not wait for
    the clear-to-send overwrites the inbox of a receiver still in its
    previous run."""
    real = broadcast_sim.plans

    def no_credit(P, count, nptrs, root, rp):
        out = []
        for steps, arena in real(P, count, nptrs, root, rp):
            out.append(([s for s in steps if s.kind not in (KIND["NOTIFY"], KIND["WAIT_NOTIFY"])], arena))
        return out

    monkeypatch.setattr(broadcast_sim, "plans", no_credit)
    payloads = [np.full(16, v, np.uint8) for v in (1, 2, 3)]
    seen = 0
    for seed in range(40):
        try:
            broadcast_sim.simulate(2, 16, 1, 0, 0, payloads, seed=seed)
        except (ProtocolError, AssertionError):
            seen += 1
    assert seen > 0


@pytest.mark.parametrize("P", SIZES)
def test_sends_and_receives_match_pairwise(P):
    """Per (sender, receiver, slot): as many SENDs as WAIT_RECVs, each SEND
    inside the region the receiver declared; as many NOTIFYs as WAIT_NOTIFYs."""
    for root in range(P):
        for count in (1, 1000):
            for nptrs in (1, 3):
                pl = [plan(r, P, count, nptrs, root, nptrs - 1)[0] for r in range(P)]
                sends, recvs, notes, waits, decl = {}, {}, {}, {}, {}
                for r, steps in enumerate(pl):
                    for s in steps:
                        if s.kind == KIND["SEND"]:
                            sends.setdefault((r, s.peer, s.slot), []).append(s)
                        elif s.kind == KIND["WAIT_RECV"]:
                            recvs[(s.peer, r, s.slot)] = recvs.get((s.peer, r, s.slot), 0) + 1
                        elif s.kind == KIND["NOTIFY"]:
                            notes[(r, s.peer, s.slot)] = notes.get((r, s.peer, s.slot), 0) + 1
                        elif s.kind == KIND["WAIT_NOTIFY"]:
                            waits[(s.peer, r, s.slot)] = waits.get((s.peer, r, s.slot), 0) + 1
                        elif s.kind == KIND["DECL_RECV"]:
                            decl[(s.peer, r, s.slot)] = s
                assert {k: len(v) for k, v in sends.items()} == recvs
                assert notes == waits
                assert set(sends) == set(decl) == {(root, r, 0) for r in range(P) if r != root}
                for key, ss in sends.items():
                    for s in ss:
                        assert s.src_off == 0 and s.length == count and s.flags == 0
                        assert s.dst_off + s.length <= decl[key].length


@pytest.mark.parametrize("P", (2, 3, 5, 8, 12))
def test_root_order_is_the_references(P):
    """cuda_broadcast_one_to_all.cc:98-128: per peer in ascending rank the
    clear-to-send then the send; the local broadcast; the send completions."""
    for root in range(P):
        for nptrs in (1, 3):
            steps, arena = plan(root, P, 7, nptrs, root, 0)
            peers = [r for r in range(P) if r != root]
            want = []
            for _ in peers:
                want += [KIND["WAIT_NOTIFY"], KIND["SEND"]]
            if nptrs > 1:
                want.append(KIND["LOCAL_BCAST"])
            want += [KIND["WAIT_SEND"]] * len(peers)
            assert kinds(steps) == want
            assert [s.peer for s in steps if s.kind == KIND["SEND"]] == peers
            assert [s.peer for s in steps if s.kind == KIND["WAIT_NOTIFY"]] == peers
            assert [s.peer for s in steps if s.kind == KIND["WAIT_SEND"]] == peers
            assert arena == 0


@pytest.mark.parametrize("P", (2, 3, 5, 8, 12))
def test_receiver_order_is_the_references(P):
    """.cc:130-148: clear-to-send to the root, the arrival, inbox -> pointer
    0, the local broadcast."""
    root = P - 1
    for r in range(P - 1):
        for nptrs in (1, 3):
            steps, arena = plan(r, P, 7, nptrs, root, 0)
            want = [KIND["DECL_RECV"], KIND["NOTIFY"], KIND["WAIT_RECV"], KIND["COPY"]]
            if nptrs > 1:
                want.append(KIND["LOCAL_BCAST"])
            assert kinds(steps) == want
            assert all(s.peer == root for s in steps[:3])
            assert arena == 7
            copy = steps[3]
            assert (copy.flags, copy.dst_off, copy.src_off, copy.length) == (1, 0, 0, 7)  # SRC_ARENA


def test_one_rank_and_no_elements():
    steps, arena = plan(0, 1, 1000, 3, 0, 2)
    assert kinds(steps) == [KIND["LOCAL_BCAST"]] and arena == 0
    assert (steps[0].dst_off, steps[0].length) == (0, 1000)
    assert plan(0, 1, 1000, 1) == ([], 0)  # one rank, one pointer: nothing to do
    for P in SIZES:
        for r in range(P):
            for nptrs in (1, 3):
                assert plan(r, P, 0, nptrs, P - 1, nptrs - 1) == ([], 0)  # no elements: no data steps


def test_plan_does_not_depend_on_the_root_pointer():
    """Pointer 0 of a plan IS the root pointer (the entry points reorder), so
    the steps are the same for every root pointer."""
    def flat(steps):
        return [tuple(getattr(s, f) for f, _ in Step._fields_) for s in steps]
    for r in range(3):
        base = flat(plan(r, 3, 100, 3, 1, 0)[0])
        assert flat(plan(r, 3, 100, 3, 1, 1)[0]) == base == flat(plan(r, 3, 100, 3, 1, 2)[0])


def raw_plan(algo, rank, size, count, nptrs, recv):
    import gloo_amd
    L = gloo_amd.lib
    L.gloo_hip_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    n, arena = ctypes.c_size_t(), ctypes.c_size_t()
    rp = (ctypes.c_int * 2)(*recv) if recv is not None else None
    rc = L.gloo_hip_plan(algo, rank, size, count, nptrs, rp, None, 0, ctypes.byref(n), ctypes.byref(arena))
    return rc, L.gloo_hip_last_error().decode(), n.value


@pytest.mark.parametrize("root", (-1, 4, 100))
def test_root_out_of_range_is_refused(root):
    rc, msg, _ = raw_plan(BROADCAST, 0, 4, 10, 1, [root, 0])
    assert rc == EINVAL_ARG
    assert f"root rank {root} " in msg and "[0, 4)" in msg


@pytest.mark.parametrize("rp", (-1, 3, 9))
def test_root_pointer_out_of_range_is_refused(rp):
    rc, msg, _ = raw_plan(BROADCAST, 0, 4, 10, 3, [1, rp])
    assert rc == EINVAL_ARG
    assert f"root pointer {rp} " in msg and "[0, 3)" in msg


def test_mesh_form_is_refused():
    rc, msg, _ = raw_plan(BROADCAST | MESH, 0, 4, 10, 1, [0, 0])
    assert rc == EINVAL_ARG
    assert str(BROADCAST | MESH) in msg and "mesh" in msg


def test_null_geometry_means_root_0_pointer_0():
    rc, _, n = raw_plan(BROADCAST, 0, 3, 10, 2, None)
    assert rc == 0 and n == 2 * 2 + 1 + 2  # the root's plan: rank 0 is the root


def test_plan_ex_takes_every_dtype_size():
    for es in (1, 2, 4, 8):
        steps, arena = get_plan("broadcast", 1, 2, 33, 1, recv=[0, 0], elem_size=es)
        assert arena == 33 and steps[-1].length == 33


def test_algorithm_entry_points_refuse_before_any_exchange():
    """gloo_hip_algorithm_create*: the geometry and the mesh flag are checked
    on the calling rank before any exchange with a peer, whatever `op` is; the bitwise-on-float refusal
    (GLOO_HIP_EINVAL_OP) does not fire for a broadcast.  A one-rank context
    over a mem: store needs no GPU to be created."""
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:bcast_refusals")
    try:
        bxor, f32 = 7, "f32"
        for kw, text in ((dict(root=1), "root rank 1 "), (dict(root=-2), "root rank -2 "),
                         (dict(root=0, root_pointer=2), "root pointer 2 "),
                         (dict(root=0, root_pointer=-1), "root pointer -1 ")):
            for streams in (None, []):
                with pytest.raises(gloo_amd.GlooHipError) as e:
                    gloo_amd.Algorithm(ctx, "broadcast", bxor, f32, [0x1000, 0x2000], 16, streams=streams, **kw)
                assert e.value.code == EINVAL_ARG and text in str(e.value)
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.Algorithm(ctx, BROADCAST | MESH, bxor, f32, [0x1000], 16, root=0)
        assert e.value.code == EINVAL_ARG and str(BROADCAST | MESH) in str(e.value)
        # the reductions do refuse that pair, with another code
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.Algorithm(ctx, "local", bxor, f32, [0x1000], 16)
        assert e.value.code == -1
    finally:
        ctx.close()


class Desc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("nsrc", ctypes.c_int32), ("dst", ctypes.c_uint64),
                ("src", ctypes.c_uint64 * 8), ("bytes", ctypes.c_uint64)]


class DescEx(ctypes.Structure):
    _fields_ = [("step", Desc), ("nxdst", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("xdst", ctypes.c_uint64 * 8)]


COPY, SEND, SIGNAL, WAIT, FOLD = range(5)


def batches(steps):
    import gloo_amd
    arr = (DescEx * len(steps))()
    for i, (kind, dst, src, n, xd) in enumerate(steps):
        arr[i].step.kind, arr[i].step.nsrc, arr[i].step.dst, arr[i].step.bytes = kind, 1, dst, n
        arr[i].step.src[0] = src
        arr[i].nxdst = len(xd)
        for j, x in enumerate(xd):
            arr[i].xdst[j] = x
    out = (ctypes.c_int * len(steps))()
    L = gloo_amd.lib
    L.gloo_hip_interp_batches_ex.argtypes = [ctypes.POINTER(DescEx), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    assert L.gloo_hip_interp_batches_ex(arr, len(steps), out) == 0
    return list(out)


def test_interp_batches_of_a_lowered_broadcast():
    """The interpreter's step lists of a broadcast as buildInterp lowers them.
    Root (2 peers, 3 pointers): wait, send, wait, send, then the local
    broadcast as ONE copy to pointer 1 with pointer 2 as a further
    destination.  The last send and the broadcast are independent (both read
    the source), so they share a drain; waits and sends alternate, so nothing
    else batches.  Receiver: signal, wait, then the receive + broadcast: ONE
    copy inbox -> pointer 0 with pointers 1 and 2 as further destinations.
    A step that reads a further destination must not join that copy's batch:
    every destination of the fan-out counts as written."""
    n = 4096
    S, P1, P2, X, Y, INBOX, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    root = [(WAIT, 0, 0, 0, []), (SEND, X, S, n, []), (WAIT, 0, 0, 0, []), (SEND, Y, S, n, []),
            (COPY, P1, S, n, [P2])]
    assert batches(root) == [0, 0, 0, 1, 0]
    recv = [(SIGNAL, 0, 0, 0, []), (WAIT, 0, 0, 0, []), (COPY, S, INBOX, n, [P1, P2])]
    assert batches(recv) == [0, 0, 0]
    # a reader of the LAST further destination right behind the fan-out
    for reads, want in ((P2, 0), (P1, 0), (S, 0), (E, 1)):
        tail = recv + [(COPY, E + 0x10000, reads, n, [])]
        assert batches(tail)[2] == want, hex(reads)
    # and a writer into one of them
    assert batches(recv + [(COPY, P2 + 16, E, n, [])])[2] == 0
