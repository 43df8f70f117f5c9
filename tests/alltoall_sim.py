"""CPU simulation of the alltoall plan — TEST INFRASTRUCTURE (beside plan_sim.py,
broadcast_sim.py and allgather_sim.py).

Runs every rank's GLOO_HIP_ALGO_ALLTOALL step list (gloo_hip_plan_ex) several
times back to back with a DIFFERENT payload per run and no barrier between
runs, the ranks interleaved in a seeded random order.  An alltoall has no
arithmetic, so the model is closed form (gloo/alltoallv.cc):

    out_r[outOff_r[q], +out_counts_r[q]) == in_q[inOff_q[r], +in_counts_q[r])

with the offsets the prefix sums of the counts.  `counts` is the P x P matrix
M, M[q][r] = elements rank q sends to rank r: rank r's in_counts are row r,
its out_counts column r.  At the start of each of its runs a rank's output is
refilled with a sentinel, so bytes left by run r - 1 would be seen.  Inbox
regions are exactly the DECL_RECVs: a SEND to an undeclared region, past its
region's end, or onto a block the receiver has not copied out yet is a
ProtocolError; the last is the ordering the previous-run credit has to give
(a sender's run r + 1 SEND after the receiver's run r COPY).  Inputs must
come back unmodified.
"""
import random

import numpy as np

import plan_sim
from plan_sim import SRC_ARENA, DST_ARENA, FROM_INPUTS, PREV_RUN, KIND, ProtocolError

ALLTOALL = 14  # include/gloo_amd.h GLOO_HIP_ALGO_ALLTOALL
plan_sim.ALGO.setdefault("alltoall", ALLTOALL)
SENTINEL = 0xEE


def even(P, count):
    return [[count] * P for _ in range(P)]


def recv_elems(M, r):
    """Rank r's recv_elems: in_counts (row r) then out_counts (column r)."""
    P = len(M)
    return list(M[r]) + [M[q][r] for q in range(P)]


def plans(M, even_count=None):
    """even_count: take the even form (recv_elems NULL) with that count."""
    P = len(M)
    if even_count is not None:
        return [plan_sim.get_plan("alltoall", r, P, even_count, 1, nin=1, elem_size=1) for r in range(P)]
    return [plan_sim.get_plan("alltoall", r, P, 0, 1, recv=recv_elems(M, r), nin=1, elem_size=1) for r in range(P)]


def prefix(v):
    off = [0]
    for c in v:
        off.append(off[-1] + c)
    return off


def expected(M, ins, r):
    """Rank r's output for the inputs ins[q] (uint8, sum of row q long)."""
    P = len(M)
    parts = []
    for q in range(P):
        o = prefix(M[q])[r]
        parts.append(ins[q][o:o + M[q][r]])
    return np.concatenate(parts + [np.zeros(0, np.uint8)])


def simulate(M, payloads, seed=0, even_count=None, drop_credit_wait=False):
    """payloads[run][r]: rank r's input of that run.  drop_credit_wait: run
    the plans with their WAIT_NOTIFY | PREV_RUN steps taken as met at once
    (the test of the test: the simulator must then see an overwritten inbox)."""
    P = len(M)
    pl = plans(M, even_count)
    out_total = [sum(M[q][r] for q in range(P)) for r in range(P)]
    runs = len(payloads)
    out = [np.full(out_total[r], SENTINEL, np.uint8) for r in range(P)]
    ins = [None] * P
    arena = [np.full(max(1, a), SENTINEL, np.uint8) for _, a in pl]
    region = {}
    for r, (steps, _) in enumerate(pl):
        for s in steps:
            if s.kind == KIND["DECL_RECV"]:
                assert (s.peer, r, s.slot) not in region
                region[(s.peer, r, s.slot)] = (s.dst_off, s.length)
    body = [[s for s in steps if s.kind != KIND["DECL_RECV"]] for steps, _ in pl]
    lag_per_run = {}
    for r in range(P):
        for s in body[r]:
            if s.kind == KIND["WAIT_NOTIFY"] and s.flags & PREV_RUN:
                lag_per_run[(s.peer, r, s.slot)] = lag_per_run.get((s.peer, r, s.slot), 0) + 1
    sent, consumed, lagged, unread = {}, {}, {}, {}
    run_of, pc = [0] * P, [0] * P
    rng = random.Random(seed)

    def begin_run(r):
        out[r][:] = SENTINEL
        ins[r] = payloads[run_of[r]][r].copy()

    def end_run(r):
        want = expected(M, payloads[run_of[r]], r)
        bad = np.flatnonzero(out[r] != want)
        assert bad.size == 0, f"run {run_of[r]}: rank {r} output byte {bad[0]} is {out[r][bad[0]]:#x}, " \
                              f"want {want[bad[0]]:#x}"
        assert (ins[r] == payloads[run_of[r]][r]).all(), f"run {run_of[r]}: rank {r}'s input was modified"

    def runnable(r):
        if run_of[r] >= runs:
            return False
        if pc[r] >= len(body[r]):
            return True
        s = body[r][pc[r]]
        key = (s.peer, r, s.slot)
        if s.kind == KIND["WAIT_NOTIFY"] and s.flags & PREV_RUN:
            return drop_credit_wait or sent.get(key, 0) >= lagged.get(key, 0) + 1 - lag_per_run[key]
        if s.kind in (KIND["WAIT_RECV"], KIND["WAIT_NOTIFY"]):
            return sent.get(key, 0) > consumed.get(key, 0)
        return True

    for r in range(P):
        begin_run(r)
    while True:
        ready = [r for r in range(P) if runnable(r)]
        if not ready:
            if all(run_of[r] >= runs for r in range(P)):
                break
            raise ProtocolError(f"deadlock: runs {run_of}, pcs {pc}")
        r = rng.choice(ready)
        if pc[r] >= len(body[r]):
            end_run(r)
            run_of[r] += 1
            pc[r] = 0
            for (snd, rcv, slot), (roff, cap) in region.items():
                if rcv == r and not unread.get((snd, rcv, slot)):
                    arena[r][roff:roff + cap] = SENTINEL
            if run_of[r] < runs:
                begin_run(r)
            continue
        s = body[r][pc[r]]
        pc[r] += 1
        K = s.kind
        if K == KIND["WAIT_SEND"]:
            continue
        if K == KIND["SEND"]:
            key = (r, s.peer, s.slot)
            if key not in region:
                raise ProtocolError(f"send to undeclared region {key}")
            if unread.get(key):
                raise ProtocolError(f"send {key} lands on a block the receiver has not copied out")
            roff, cap = region[key]
            if s.dst_off + s.length > cap:
                raise ProtocolError(f"send {key} of {s.length} exceeds its region of {cap}")
            assert s.flags == FROM_INPUTS, f"rank {r}: a SEND with flags {s.flags}"
            arena[s.peer][roff + s.dst_off:roff + s.dst_off + s.length] = ins[r][s.src_off:s.src_off + s.length]
            unread[key] = True
            sent[key] = sent.get(key, 0) + 1
        elif K == KIND["NOTIFY"]:
            key = (r, s.peer, s.slot)
            sent[key] = sent.get(key, 0) + 1
        elif K == KIND["WAIT_NOTIFY"] and s.flags & PREV_RUN:
            key = (s.peer, r, s.slot)
            lagged[key] = lagged.get(key, 0) + 1
        elif K in (KIND["WAIT_RECV"], KIND["WAIT_NOTIFY"]):
            key = (s.peer, r, s.slot)
            consumed[key] = consumed.get(key, 0) + 1
        elif K == KIND["COPY"]:
            assert not s.flags & DST_ARENA
            src = ins[r] if s.flags & FROM_INPUTS else arena[r] if s.flags & SRC_ARENA else out[r]
            assert s.src_off + s.length <= len(src) and s.dst_off + s.length <= len(out[r])
            out[r][s.dst_off:s.dst_off + s.length] = src[s.src_off:s.src_off + s.length].copy()
            if s.flags & SRC_ARENA:
                hit = [key for key, (roff, cap) in region.items()
                       if key[1] == r and roff == s.src_off and cap == s.length]
                if len(hit) != 1:
                    raise ProtocolError(f"rank {r}: a COPY out of [{s.src_off}, +{s.length}), no declared region")
                unread[hit[0]] = False
        else:
            raise ProtocolError(f"step kind {K} has no place in an alltoall plan")
    if not drop_credit_wait:
        for key, n in sent.items():
            if key in lag_per_run:
                if n != lagged.get(key, 0):
                    raise ProtocolError(f"{key}: {n} credits sent, {lagged.get(key, 0)} awaited")
            elif n != consumed.get(key, 0):
                raise ProtocolError(f"{key}: {n} sent, {consumed.get(key, 0)} consumed")
