"""CPU simulation of the gather and scatter plans — TEST INFRASTRUCTURE (beside
plan_sim.py, broadcast_sim.py, allgather_sim.py and alltoall_sim.py).

Runs every rank's GLOO_HIP_ALGO_GATHER or GLOO_HIP_ALGO_SCATTER step list
(gloo_hip_plan_ex) several times back to back with a DIFFERENT payload per run
and no barrier between runs, the ranks interleaved in a seeded random order.
Neither collective has arithmetic, so the model is closed form:

    gather   (gloo/gather.cc, gloo/gatherv.cc): the root's output is rank 0's
             input, rank 1's input, ... back to back (counts[q] elements of
             rank q); no other rank has an output
    scatter  (gloo/scatter.cc): rank q's output is the root's input q

At the start of each of its runs a rank's output is refilled with a sentinel,
so bytes left by run r - 1 would be seen; a gather rank that is not the root
keeps a sentinel-filled "output" that must stay untouched.  Inbox regions are
exactly the DECL_RECVs: a SEND to an undeclared region, past its region's end,
or onto a block the receiver has not copied out yet is a ProtocolError; the
last is the ordering the gather's previous-run credit and the scatter's
clear-to-send have to give.  Inputs must come back unmodified.
"""
import random

import numpy as np

import plan_sim
from plan_sim import SRC_ARENA, DST_ARENA, FROM_INPUTS, PREV_RUN, KIND, ProtocolError

GATHER, SCATTER = 15, 16  # include/gloo_amd.h GLOO_HIP_ALGO_GATHER / GLOO_HIP_ALGO_SCATTER
plan_sim.ALGO.setdefault("gather", GATHER)
plan_sim.ALGO.setdefault("scatter", SCATTER)
COUNT_PER_RANK = (1 << 64) - 1  # GLOO_HIP_COUNT_PER_RANK
INPUT_SHIFT = 8                 # GLOO_HIP_INPUT_SHIFT
SENTINEL = 0xEE


def input_of(flags):
    return flags >> INPUT_SHIFT


def gather_plans(P, root, counts=None, count=0):
    """counts: the gatherv form (recv_elems = [root] + counts); else `count` per rank."""
    out = []
    for r in range(P):
        nout = 1 if r == root else 0
        if counts is None:
            out.append(plan_sim.get_plan("gather", r, P, count, nout, recv=[root], nin=1, elem_size=1))
        else:
            out.append(plan_sim.get_plan("gather", r, P, COUNT_PER_RANK, nout, recv=[root] + list(counts), nin=1,
                                         elem_size=1))
    return out


def scatter_plans(P, root, count):
    return [plan_sim.get_plan("scatter", r, P, count, 1, recv=[root], nin=P if r == root else 0, elem_size=1)
            for r in range(P)]


def simulate(kind, P, root, payloads, counts=None, count=0, seed=0, drop_wait=False, plans=None):
    """kind: "gather" or "scatter".  gather: payloads[run][r] is rank r's
    input; scatter: payloads[run][q] is the root's input for rank q.
    drop_wait: every WAIT_NOTIFY (the gather's previous-run credit, the
    scatter's clear-to-send) is taken as met at once (the test of the test:
    the simulator must then see an overwritten inbox)."""
    gather = kind == "gather"
    if plans is None:
        plans = gather_plans(P, root, counts, count) if gather else scatter_plans(P, root, count)
    cnt = list(counts) if counts is not None else [count] * P
    off = [0]
    for c in cnt:
        off.append(off[-1] + c)
    runs = len(payloads)
    out_len = [(off[P] if r == root else 0) if gather else count for r in range(P)]
    out = [np.full(out_len[r], SENTINEL, np.uint8) for r in range(P)]
    untouched = [np.full(16, SENTINEL, np.uint8) for _ in range(P)]  # a gather non-root's "output"
    ins = [None] * P  # gather: one array; scatter root: a list of P arrays
    arena = [np.full(max(1, a), SENTINEL, np.uint8) for _, a in plans]
    region = {}
    for r, (steps, _) in enumerate(plans):
        for s in steps:
            if s.kind == KIND["DECL_RECV"]:
                assert (s.peer, r, s.slot) not in region
                if s.dst_off + s.length > plans[r][1]:
                    raise ProtocolError(f"rank {r}: a region outside its arena of {plans[r][1]}")
                region[(s.peer, r, s.slot)] = (s.dst_off, s.length)
    body = [[s for s in steps if s.kind != KIND["DECL_RECV"]] for steps, _ in plans]
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
        pay = payloads[run_of[r]]
        if gather:
            ins[r] = [pay[r].copy()]
        else:
            ins[r] = [p.copy() for p in pay] if r == root else []

    def end_run(r):
        pay = payloads[run_of[r]]
        if gather:
            want = np.concatenate([pay[q][:cnt[q]] for q in range(P)] + [np.zeros(0, np.uint8)]) if r == root \
                else np.zeros(0, np.uint8)
        else:
            want = pay[r]
        bad = np.flatnonzero(out[r] != want)
        assert bad.size == 0, f"run {run_of[r]}: rank {r} output byte {bad[0]} is {out[r][bad[0]]:#x}, " \
                              f"want {want[bad[0]]:#x}"
        assert (untouched[r] == SENTINEL).all(), f"run {run_of[r]}: rank {r} wrote a buffer it does not own"
        orig = [pay[r]] if gather else (list(pay) if r == root else [])
        for a, b in zip(ins[r], orig):
            assert (a == b).all(), f"run {run_of[r]}: rank {r}'s input was modified"

    def runnable(r):
        if run_of[r] >= runs:
            return False
        if pc[r] >= len(body[r]):
            return True
        s = body[r][pc[r]]
        key = (s.peer, r, s.slot)
        if s.kind == KIND["WAIT_NOTIFY"] and drop_wait:
            return True
        if s.kind == KIND["WAIT_NOTIFY"] and s.flags & PREV_RUN:
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
            for (snd, rcv, slot), (roff, cap) in region.items():
                if rcv == r and not unread.get((snd, rcv, slot)):
                    arena[r][roff:roff + cap] = SENTINEL
            if run_of[r] < runs:
                begin_run(r)
            continue
        s = body[r][pc[r]]
        pc[r] += 1
        K = s.kind
        # output 0 of a gather rank without an output is a buffer it must not touch
        user = out[r] if (not gather or r == root) else untouched[r]
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
            assert s.flags & FROM_INPUTS and not s.flags & (SRC_ARENA | DST_ARENA), \
                f"rank {r}: a SEND with flags {s.flags}"
            src = ins[r][input_of(s.flags)]
            assert s.src_off + s.length <= len(src)
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
            assert not s.flags & DST_ARENA
            src = ins[r][input_of(s.flags)] if s.flags & FROM_INPUTS else arena[r] if s.flags & SRC_ARENA else user
            assert s.src_off + s.length <= len(src) and s.dst_off + s.length <= len(user)
            user[s.dst_off:s.dst_off + s.length] = src[s.src_off:s.src_off + s.length].copy()
            if s.flags & SRC_ARENA:
                hit = [key for key, (roff, cap) in region.items()
                       if key[1] == r and roff == s.src_off and cap == s.length]
                if len(hit) != 1:
                    raise ProtocolError(f"rank {r}: a COPY out of [{s.src_off}, +{s.length}), no declared region")
                unread[hit[0]] = False
        else:
            raise ProtocolError(f"step kind {K} has no place in a {kind} plan")
    if not drop_wait:
        for key, n in sent.items():
            if key in lag_per_run:
                if n != lagged.get(key, 0):
                    raise ProtocolError(f"{key}: {n} credits sent, {lagged.get(key, 0)} awaited")
            elif n != consumed.get(key, 0):
                raise ProtocolError(f"{key}: {n} sent, {consumed.get(key, 0)} consumed")
