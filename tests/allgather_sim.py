"""CPU simulation of the allgather plan — TEST INFRASTRUCTURE (beside plan_sim.py
and broadcast_sim.py).

Runs every rank's GLOO_HIP_ALGO_ALLGATHER step list (gloo_hip_plan_ex) several
times back to back with a DIFFERENT payload per run and no barrier between
runs, the ranks interleaved in a seeded random order.  An allgather has no
arithmetic, so the model is closed form: rank r contributes k inputs of
counts[r] elements; block r is those inputs concatenated; after a rank's run
its output holds block 0, block 1, ... block P-1 back to back.  At the start
of each of its runs a rank's output and arena are refilled with a sentinel
(in place: the output keeps only the rank's own block), so bytes left by run
r - 1 would be seen.  A SEND that lands in an inbox whose previous block has
not been copied out yet is a ProtocolError: that is the ordering the
previous-run credit has to give (a sender's run r + 1 SEND after the
receiver's run r COPY).  Inputs must come back unmodified.

plan_sim.py is an existing test file, so this module teaches its own copy of
the step table the new step kind, as broadcast_sim.py registers its algorithm.
"""
import random

import numpy as np

import plan_sim
from plan_sim import SRC_ARENA, DST_ARENA, PREV_RUN, ProtocolError

ALLGATHER = 13  # include/gloo_amd.h GLOO_HIP_ALGO_ALLGATHER
plan_sim.ALGO.setdefault("allgather", ALLGATHER)
KIND = dict(plan_sim.KIND, LOCAL_GATHER=12)  # include/gloo_amd.h GLOO_HIP_STEP_LOCAL_GATHER
SENTINEL = 0xEE


def plans(P, count, k, counts=None):
    """k: inputs per rank, 0 = in place.  counts: per-rank list or None."""
    return [plan_sim.get_plan("allgather", r, P, count, 1, recv=counts, nin=k, elem_size=1) for r in range(P)]


def offsets(P, count, k, counts):
    kk = max(1, k)
    c = [count] * P if counts is None else list(counts)
    off = [0]
    for q in range(P):
        off.append(off[-1] + kk * c[q])
    return c, off


def expected(P, count, k, counts, ins):
    """ins[r][i]: rank r's input i (in place: ins[r][0] is its block)."""
    return np.concatenate([np.concatenate(ins[r]) if len(ins[r]) else np.zeros(0, np.uint8) for r in range(P)]
                          + [np.zeros(0, np.uint8)])


def simulate(P, count, k, counts, payloads, seed=0):
    """payloads[run][r][i]: uint8 array of counts[r] bytes, input i of rank r
    in that run (k = 0: one array, the rank's own block).  Returns nothing;
    raises ProtocolError / AssertionError."""
    pl = plans(P, count, k, counts)
    kk = max(1, k)
    c, off = offsets(P, count, k, counts)
    total = off[P]
    runs = len(payloads)
    out = [np.full(total, SENTINEL, np.uint8) for _ in range(P)]
    ins = [[None] * kk for _ in range(P)]
    arena = [np.full(max(1, a), SENTINEL, np.uint8) for _, a in pl]
    for r, (_, a) in enumerate(pl):
        assert a == (total if P > 1 and total else 0), f"rank {r}: arena of {a}, output of {total}"
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
    sent, consumed, lagged = {}, {}, {}
    unread = {}  # (sender, receiver, slot) -> a block sits in the inbox, not yet copied out
    run_of = [0] * P
    pc = [0] * P
    rng = random.Random(seed)

    def begin_run(r):
        out[r][:] = SENTINEL
        # the arena is NOT refilled here: a peer ahead of this rank may already
        # have delivered this run's block (refilled at the end of the run, below)
        for i in range(kk):
            ins[r][i] = payloads[run_of[r]][r][i].copy()
        if k == 0:
            out[r][off[r]:off[r + 1]] = ins[r][0]

    def end_run(r):
        want = expected(P, count, k, counts, payloads[run_of[r]])
        bad = np.flatnonzero(out[r] != want)
        assert bad.size == 0, f"run {run_of[r]}: rank {r} output byte {bad[0]} is {out[r][bad[0]]:#x}, " \
                              f"want {want[bad[0]]:#x}"
        for i in range(kk):
            assert (ins[r][i] == payloads[run_of[r]][r][i]).all(), f"run {run_of[r]}: rank {r} input {i} modified"

    def runnable(r):
        if run_of[r] >= runs:
            return False
        if pc[r] >= len(body[r]):
            return True  # finishes its run
        s = body[r][pc[r]]
        key = (s.peer, r, s.slot)
        if s.kind == KIND["WAIT_NOTIFY"] and s.flags & PREV_RUN:
            # the i-th such wait is met by the previous run's credits
            return sent.get(key, 0) >= lagged.get(key, 0) + 1 - lag_per_run[key]
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
            # every inbox of this rank that holds no unread block goes back to the sentinel
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
        if K == KIND["LOCAL_GATHER"]:
            assert k > 0, "LOCAL_GATHER in an in-place plan"
            for i in range(k):
                out[r][s.dst_off + i * s.length:s.dst_off + (i + 1) * s.length] = ins[r][i][:s.length]
        elif K == KIND["SEND"]:
            key = (r, s.peer, s.slot)
            if key not in region:
                raise ProtocolError(f"send to undeclared region {key}")
            if unread.get(key):
                raise ProtocolError(f"send {key} lands on a block the receiver has not copied out")
            roff, cap = region[key]
            if s.dst_off + s.length > cap:
                raise ProtocolError(f"send {key} of {s.length} exceeds its region of {cap}")
            src = arena[r] if s.flags & SRC_ARENA else out[r]
            arena[s.peer][roff + s.dst_off:roff + s.dst_off + s.length] = src[s.src_off:s.src_off + s.length]
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
            src = arena[r] if s.flags & SRC_ARENA else out[r]
            dst = arena[r] if s.flags & DST_ARENA else out[r]
            dst[s.dst_off:s.dst_off + s.length] = src[s.src_off:s.src_off + s.length].copy()
            if s.flags & SRC_ARENA:  # the inbox that holds [src_off, +length) is free again
                for key, (roff, cap) in region.items():
                    if key[1] == r and roff <= s.src_off < roff + max(1, cap):
                        unread[key] = False
        else:
            raise ProtocolError(f"step kind {K} has no place in an allgather plan")
    for key, n in sent.items():
        if key in lag_per_run:
            if n != lagged.get(key, 0):
                raise ProtocolError(f"{key}: {n} credits sent, {lagged.get(key, 0)} awaited")
        elif n != consumed.get(key, 0):
            raise ProtocolError(f"{key}: {n} sent, {consumed.get(key, 0)} consumed")
