"""CPU: the interpreter model (tests/interp_model.py) and the shapes and inputs
tests/test_interp_kernel_gpu.py runs it at, on the model alone.

  * the slice bounds cover [0, n) exactly once, in order, and every slice
    starts on a 16-byte boundary of the step, for every (n, G) of the GPU tests;
  * the inputs of the GPU fold cases tell modes 0 / 1 / 2 apart on the float
    dtypes (a kernel folding in another order cannot pass);
  * the loopback chain's outcome (bytes, flags, err) changes when any one of
    its steps is skipped.  The WAIT moves no byte: that it is live shows in
    the unmet wait a skipped SEND leaves behind.
"""
import numpy as np
import pytest

import fold_model as fm
import interp_model as im


def test_slice_bounds_cover_every_gpu_shape_once_on_packet_boundaries():
    shapes = im.gpu_shapes()
    assert {G for _, G, _ in shapes} == set(im.SLICE_COUNTS) | {im.MANY_SLICES}
    for n, G, es in shapes:
        b = im.slice_bounds(n, G, es)
        assert len(b) == G and b[0][0] == 0 and b[-1][1] == n, (n, G, es)
        for g in range(G):
            lo, hi = b[g]
            # (a slice past the end is the empty [n, n): it moves nothing)
            assert 0 <= lo <= hi <= n and ((lo * es) % 16 == 0 or lo == hi == n), (n, G, es, g, lo, hi)
            assert g == 0 or lo == b[g - 1][1], (n, G, es, g)
        # every slice but the last non-empty one is whole packets
        sizes = [hi - lo for lo, hi in b if hi > lo]
        assert all((s * es) % 16 == 0 for s in sizes[:-1]) and sum(sizes) == n, (n, G, es)


def test_sliced_sizes_are_what_they_claim():
    for es in (1, 2, 4, 8):
        kV = 16 // es
        for G in im.SLICE_COUNTS + (im.MANY_SLICES,):
            ragged, short, exact = im.sliced_sizes(G, es)
            b = im.slice_bounds(ragged, G, es)
            assert sum(hi > lo for lo, hi in b) >= min(G, 2) and b[0][1] > kV, "several slices of several packets"
            b = im.slice_bounds(short, G, es)
            assert [hi - lo for lo, hi in b] == ([kV + 1] if G == 1 else [kV, 1] + [0] * (G - 2))
            b = im.slice_bounds(exact, G, es)
            assert len({hi - lo for lo, hi in b}) == 1 and b[0][1] % kV == 0


def ndiff(a, b):
    return int((fm.bits(a) != fm.bits(b)).sum())


@pytest.mark.parametrize("dtype", fm.FLOATS)
def test_gpu_fold_inputs_tell_the_modes_apart(dtype):
    """At the shape of test_every_dtype_and_op (k = 4, one pass and a bit):
    max and min separate all three orders, sum separates left from tree."""
    es = fm.itemsize(dtype)
    n = im.fp_bytes(es) // es + 16 // es + 3
    for op in ("max", "min"):
        srcs = im.fold_case(op, dtype, 4, n)
        f = [fm.fold(op, dtype, srcs, m) for m in range(3)]
        assert ndiff(f[0], f[1]) >= 1 and ndiff(f[1], f[2]) >= 1 and ndiff(f[0], f[2]) >= 1, (dtype, op)
    srcs = im.fold_case("sum", dtype, 4, n)
    assert ndiff(fm.fold("sum", dtype, srcs, 0), fm.fold("sum", dtype, srcs, 2)) >= 1


def test_shape_case_inputs_tell_left_from_reverse_in_head_body_and_tail():
    """f32 max of the shape cases: modes 0 and 1 differ inside the first packet,
    so a swapped operand shows at every size from one packet up."""
    n = im.fold_sizes(4)[-1]
    for k in (2, 3, 5, 8):
        srcs = im.fold_case("max", "f32", k, n)
        d = fm.bits(fm.fold("max", "f32", srcs, 0)) != fm.bits(fm.fold("max", "f32", srcs, 1))
        assert d.sum() >= n // 64, (k, int(d.sum()))


def run_chain(op, dtype, n, skip=None, sub=None, run=1, flag_init=0):
    es = fm.itemsize(dtype)
    steps = [s for i, s in enumerate(im.chain(n, sub)) if i != skip]
    bufs = im.chain_buffers(im.chain_inputs(op, dtype, n), n, es)
    flags = {"f0": [flag_init] * 4, "f1": [flag_init] * 4}
    res = im.run_steps(op, dtype, steps, bufs, flags, run)
    return bufs, flags, res


@pytest.mark.parametrize("dtype", ("f32", "bf16", "u8"))
def test_chain_outcome_changes_when_a_step_is_skipped(dtype):
    n = 1027
    full_b, full_f, full = run_chain("sum", dtype, n)
    assert full.err == 0 and full.done == 1 and full.ticket == 0
    assert full_f == {"f0": [8, 0, 0, 0], "f1": [107, 0, 0, 0]}
    for name in im.CHAIN_BUFFERS:
        assert name in im.CHAIN_SOURCES or full.written[name].all(), name
    kinds = [s.kind for s in im.chain(n)]
    assert sorted(set(kinds)) == [im.COPY, im.SEND, im.SIGNAL, im.WAIT, im.FOLD]
    for skip, kind in enumerate(kinds):
        b, f, res = run_chain("sum", dtype, n, skip=skip)
        same = f == full_f and res.err == full.err and all((b[k] == full_b[k]).all() for k in b)
        if kind == im.WAIT:
            assert same  # it orders, it moves nothing ...
        else:
            assert not same, (dtype, "skipping step", skip)
    # ... and is live: without the SEND it is not met, and nothing after it runs
    b, f, res = run_chain("sum", dtype, n, skip=kinds.index(im.SEND))
    assert res.err == 1 and res.done is None and res.stopped == kinds.index(im.WAIT) - 1
    assert not res.written["out"].any() and not res.written["out2"].any()


def test_chain_sub_range_send_keeps_the_rest_of_the_inbox():
    n, sub = 1027, (16, 515)
    b, f, res = run_chain("sum", "f32", n, sub=sub)
    w = res.written["inbox"].reshape(-1, 4).all(axis=1)
    assert w[16:16 + 515].all() and not w[:16].any() and not w[16 + 515:].any()
    whole, _, _ = run_chain("sum", "f32", n)
    assert not (b["out"] == whole["out"]).all()


def test_sequence_values_and_signed_waits():
    M = im.M64
    s = im.Step(im.SIGNAL, flag="f0", base=M - 4, per_run=3)
    assert [im.value(s, r) for r in (1, 2, 1 << 32)] == [M - 1, 1, (M - 4 + 3 * (1 << 32)) & M]
    assert im.met(5, 5) and im.met(6, 5) and not im.met(4, 5)
    assert im.met(1, M - 1)            # the counter wrapped past the target
    assert not im.met(M - 1, 1)        # the target wrapped, the counter not yet
    assert im.met(1000, 11)            # a target below the counter passes at once
    # runs 1, 2, 3 on the same flags: each run's wait needs that run's send
    flags = {"f0": [0], "f1": [0]}
    for run in (1, 2, 3):
        def fresh():
            return im.chain_buffers(im.chain_inputs("sum", "u8", 64), 64, 1)
        no_send = [t for t in im.chain(64) if t.kind != im.SEND]
        assert im.run_steps("sum", "u8", no_send, fresh(), {k: list(v) for k, v in flags.items()}, run).err == 1
        assert im.run_steps("sum", "u8", im.chain(64), fresh(), flags, run).err == 0
        assert flags == {"f0": [5 + 3 * run], "f1": [100 + 7 * run]}
