"""CPU simulation of the broadcast plan — TEST INFRASTRUCTURE (beside plan_sim.py).

Runs every rank's GLOO_HIP_ALGO_BROADCAST step list (gloo_hip_plan) several
times back to back with a DIFFERENT payload per run and no barrier between
runs, the ranks interleaved in a seeded random order.  A broadcast has no
arithmetic, so the model is closed form: after a rank's run r every one of
its pointers equals run r's payload.  Each rank's buffers are refilled at
the start of each of its runs (the root's root pointer with the payload,
everything else with a sentinel), so bytes left in an inbox or a pointer by
run r - 1 would be seen.  A SEND that lands in an inbox whose previous message
has not been copied out yet is a protocol error: that is the ordering the
clear-to-send has to give (the root's run r + 1 send after the receiver's
run r copy).
"""
import random

import numpy as np

import plan_sim
from plan_sim import KIND, SRC_ARENA, DST_ARENA, ProtocolError

BROADCAST = 12  # include/gloo_amd.h GLOO_HIP_ALGO_BROADCAST
plan_sim.ALGO.setdefault("broadcast", BROADCAST)
SENTINEL = 0xEE


def plans(P, count, nptrs, root, root_pointer):
    return [plan_sim.get_plan("broadcast", r, P, count, nptrs, recv=[root, root_pointer], elem_size=1)
            for r in range(P)]


def pointer_order(nptrs, root_pointer):
    """The executor's pointer i is the caller's pointer order[i] (the C-ABI
    layer hands the list over with the root pointer first)."""
    return [root_pointer] + [i for i in range(nptrs) if i != root_pointer]


def simulate(P, count, nptrs, root, root_pointer, payloads, seed=0):
    """payloads: one uint8 array of `count` bytes per run.  Returns nothing;
    raises ProtocolError / AssertionError."""
    pl = plans(P, count, nptrs, root, root_pointer)
    order = pointer_order(nptrs, root_pointer)
    runs = len(payloads)
    # the caller's pointers, and the executor's view of them
    user = [[np.full(count, SENTINEL, np.uint8) for _ in range(nptrs)] for _ in range(P)]
    arena = [np.full(max(1, a), SENTINEL, np.uint8) for _, a in pl]
    region = {}
    for r, (steps, _) in enumerate(pl):
        for s in steps:
            if s.kind == KIND["DECL_RECV"]:
                assert (s.peer, r, s.slot) not in region
                region[(s.peer, r, s.slot)] = (s.dst_off, s.length)
    body = [[s for s in steps if s.kind != KIND["DECL_RECV"]] for steps, _ in pl]
    sent, consumed = {}, {}
    unread = {}  # (sender, receiver, slot) -> a message sits in the inbox, not yet copied out
    run_of = [0] * P
    pc = [0] * P
    rng = random.Random(seed)

    def begin_run(r):
        for j in range(nptrs):
            user[r][j][:] = SENTINEL
        if r == root:
            user[r][root_pointer][:] = payloads[run_of[r]]

    def end_run(r):
        for j in range(nptrs):
            assert (user[r][j] == payloads[run_of[r]]).all(), \
                f"run {run_of[r]}: rank {r} pointer {j} differs from the root's payload"

    def runnable(r):
        if run_of[r] >= runs:
            return False
        if pc[r] >= len(body[r]):
            return True  # finishes its run
        s = body[r][pc[r]]
        if s.kind in (KIND["WAIT_RECV"], KIND["WAIT_NOTIFY"]):
            key = (s.peer, r, s.slot)
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
            if run_of[r] < runs:
                begin_run(r)
            continue
        s = body[r][pc[r]]
        pc[r] += 1
        K = s.kind
        ptr = [user[r][order[i]] for i in range(nptrs)]  # executor pointer i
        if K == KIND["WAIT_SEND"]:
            continue
        if K == KIND["SEND"]:
            key = (r, s.peer, s.slot)
            if key not in region:
                raise ProtocolError(f"send to undeclared region {key}")
            if unread.get(key):
                raise ProtocolError(f"send {key} lands on a message the receiver has not copied out")
            roff, cap = region[key]
            if s.length > cap:
                raise ProtocolError(f"send {key} of {s.length} exceeds its region of {cap}")
            src = arena[r] if s.flags & SRC_ARENA else ptr[0]
            arena[s.peer][roff + s.dst_off:roff + s.dst_off + s.length] = src[s.src_off:s.src_off + s.length]
            unread[key] = True
            sent[key] = sent.get(key, 0) + 1
        elif K == KIND["NOTIFY"]:
            key = (r, s.peer, s.slot)
            sent[key] = sent.get(key, 0) + 1
        elif K in (KIND["WAIT_RECV"], KIND["WAIT_NOTIFY"]):
            key = (s.peer, r, s.slot)
            consumed[key] = consumed.get(key, 0) + 1
        elif K == KIND["COPY"]:
            src = arena[r] if s.flags & SRC_ARENA else ptr[0]
            dst = arena[r] if s.flags & DST_ARENA else ptr[0]
            dst[s.dst_off:s.dst_off + s.length] = src[s.src_off:s.src_off + s.length].copy()
            if s.flags & SRC_ARENA:  # the inbox that holds [src_off, +length) is free again
                for key, (roff, cap) in region.items():
                    if key[1] == r and roff <= s.src_off < roff + max(1, cap):
                        unread[key] = False
        elif K == KIND["LOCAL_BCAST"]:
            for i in range(1, nptrs):
                ptr[i][s.dst_off:s.dst_off + s.length] = ptr[0][s.dst_off:s.dst_off + s.length]
        else:
            raise ProtocolError(f"step kind {K} has no place in a broadcast plan")
    for key, n in sent.items():
        if n != consumed.get(key, 0):
            raise ProtocolError(f"{key}: {n} sent, {consumed.get(key, 0)} consumed")
