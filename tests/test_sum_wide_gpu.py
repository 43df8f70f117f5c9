"""GPU: GLOO_HIP_SUM_WIDE (include/gloo_amd.h "Wide sum"): a pass over k >= 3
sources of f16 / bf16 / f8e4m3 / f8e5m2 carries the sum in f32 and rounds once.
The model is numpy float32 adds in list order, narrowed once by torch on the
CPU, with the contract's canonical NaN where the f32 sum is a NaN.  Every case
asserts that this differs from the step-rounded SUM model, so a build that
routes the op to SUM cannot pass."""
import threading
import uuid

import numpy as np
import pytest

import fold_model as fm
import fp8_model

pytestmark = pytest.mark.gpu

from test_fp8_gpu import from_dev, to_dev, torch  # noqa: E402,F401  (the module's torch fixture)

# torch's name; the bits of the canonical NaN, the largest finite value, +inf (e4m3fn has none), 1.0, half an ulp of 1.0
BITS = {"f16": ("float16", 0x7E00, 0x7BFF, 0x7C00, 0x3C00, 0x1000), "bf16": ("bfloat16", 0x7FC0, 0x7F7F, 0x7F80, 0x3F80, 0x3B80),
        "f8e4m3": ("float8_e4m3fn", 0x7F, 0x7E, None, 0x38, 0x18), "f8e5m2": ("float8_e5m2", 0x7F, 0x7B, 0x7C, 0x3C, 0x30)}
DTYPES = tuple(BITS)
big_n = lambda dtype: {2: 8192 + 40 + 3, 1: 16384 + 80 + 5}[fm.itemsize(dtype)]  # noqa: E731  one tile + 5 packets + a tail
TORCH, NAN, MAX, INF, ONE, HALF_ULP = ({d: v[i] for d, v in BITS.items()} for i in range(6))


def widen(torch, dtype, bits):
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.uint8).copy()).view(getattr(torch, TORCH[dtype]))
    return t.float().numpy()


def narrow(torch, dtype, f):
    """f (float32 or float64) converted once by torch; a NaN is the contract's canonical one."""
    st = fm.STORAGE[dtype]
    bits = torch.from_numpy(np.ascontiguousarray(f)).to(getattr(torch, TORCH[dtype])).view(torch.uint8).numpy().view(st)
    return np.where(np.isnan(f), st(NAN[dtype]), bits)


def model(torch, dtype, srcs):
    a = widen(torch, dtype, srcs[0])
    for s in srcs[1:]:
        with np.errstate(invalid="ignore", over="ignore"):  # inf - inf is planted; bf16's 2 * max overflows f32
            a = (a + widen(torch, dtype, s)).astype(np.float32)
    return narrow(torch, dtype, a)


def sources(dtype, k, n):
    """Random finite values; (max, max, -max), a NaN source, +inf -inf, all -0 and (1, ulp/2, ulp/2)
    planted in the head, the body and the tail (the last only where five elements fit)."""
    rng = np.random.default_rng([7, k, n])
    srcs = [fm.mixed(dtype, n, rng) for _ in range(k)]
    sign = 0x80 << 8 * (fm.itemsize(dtype) - 1)
    for base in ([0] if n < 100 else [0, 1000, n - 4]):
        for s in srcs:
            s[base:base + 5] = [0, s[base + 1], s[base + 2], sign, 0][:n - base]
        srcs[0][base], srcs[1][base], srcs[2][base] = MAX[dtype], MAX[dtype], MAX[dtype] | sign
        srcs[1][base + 1] = NAN[dtype]
        if INF[dtype]:
            srcs[0][base + 2], srcs[2][base + 2] = INF[dtype], INF[dtype] | sign
        if base + 4 < n:
            srcs[0][base + 4], srcs[1][base + 4], srcs[2][base + 4] = ONE[dtype], HALF_ULP[dtype], HALF_ULP[dtype]
    return srcs


def run_pass(torch, dtype, srcs, op, mode, forward=False):
    """dst one element past a 16-B boundary (a forward: one before it), source j at its own residue;
    mode None: reduce_multi_ptr.  Returns [dst, forward]; sources and the bytes around dst must stay."""
    import gloo_amd
    es, n = fm.itemsize(dtype), srcs[0].size
    soff = [(5 * j + 1) % 16 // es * es for j in range(len(srcs))]
    dev = [to_dev(torch, s.view(np.uint8), o) for s, o in zip(srcs, soff)]
    ooff = [es, 16 - es][:2 if forward else 1]
    outs = [to_dev(torch, np.zeros(n * es, np.uint8), o) for o in ooff]
    ptrs = [p for _, p in dev]
    if mode is None:
        gloo_amd.reduce_multi_ptr(op, dtype, outs[0][1], ptrs, n)
    else:
        gloo_amd.fold_kernel(op, dtype, outs[0][1], ptrs, n, mode=mode, fwd=[p for _, p in outs[1:]])
    for (t, _), s, o in zip(dev, srcs, soff):
        assert (from_dev(torch, t, o, n * es) == s.view(np.uint8)).all(), "a source was modified"
    for (t, _), o in zip(outs, ooff):
        assert not t[:o].any() and not t[o + n * es:].any(), "wrote outside the chunk"
    return [from_dev(torch, t, o, n * es).view(srcs[0].dtype) for (t, _), o in zip(outs, ooff)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pass_is_the_f32_model(torch, dtype, k, mode):
    for n in (5, big_n(dtype)):
        srcs = sources(dtype, k, n)
        want = model(torch, dtype, srcs)
        assert (want != fm.fold("sum", dtype, srcs, 0)).any()  # not the step-rounded SUM
        # max + max - max comes back finite where SUM overflows, except for bf16, whose range is f32's:
        # there the contract's own f32 add overflows, and the pass must store that infinity
        assert want[0] == (INF[dtype] if dtype == "bf16" else MAX[dtype])
        assert want[1] == NAN[dtype] and want[3] == srcs[0][3] and want[4] == ONE[dtype] + 1
        got = run_pass(torch, dtype, srcs, "sum_wide", mode) + run_pass(torch, dtype, srcs, "sum_wide", mode, True)
        if mode == 0:
            got += run_pass(torch, dtype, srcs, "sum_wide", None)
        for i, g in enumerate(got):
            bad = np.flatnonzero(g != want)
            assert bad.size == 0, (n, i, bad[:8], g[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_sources_are_sum(torch, dtype, k):
    srcs = fm.inputs("sum", dtype, k, big_n(dtype), np.random.default_rng([3, k]))
    for mode, forward in ((0, False), (0, True), (None, False)):
        wide, plain = (run_pass(torch, dtype, srcs, op, mode, forward) for op in ("sum_wide", "sum"))
        assert all((w == p).all() for w, p in zip(wide, plain))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_e4m3_is_order_free(torch, mode):
    """Every f32 partial sum of 8 e4m3 values is exact: the pass stores the
    correctly rounded true sum (overflow: the NaN with its sign)."""
    n = big_n("f8e4m3")
    srcs = list(fp8_model.draw_small(np.random.default_rng(11), "f8e4m3", (8, n), bound=448.0))
    want = narrow(torch, "f8e4m3", sum(widen(torch, "f8e4m3", s).astype(np.float64) for s in srcs))
    assert 0 < fp8_model.is_nan("f8e4m3", want).sum() < n // 2
    assert (want != fp8_model.fold_left("sum", "f8e4m3", srcs)).any()
    assert (run_pass(torch, "f8e4m3", srcs, "sum_wide", mode)[0] == want).all()


@pytest.mark.parametrize("dtype", ["f8e4m3", "bf16"])
@pytest.mark.parametrize("algo", ["ring_chunked", "halving_doubling"])
def test_mesh_plans_round_once(torch, monkeypatch, algo, dtype):
    """P = 4 rank threads, one pointer: every element is folded once, at its
    owner.  Three runs on one algorithm object (each reduces the previous
    outputs); all f32 partial sums are exact for these inputs, so every run is
    the float64 sum of its inputs converted once, on every rank."""
    import plan_sim
    from test_collectives_gpu import run_threads
    P, n, runs = 4, 12_289, 3
    rng = np.random.default_rng(5)
    if dtype == "bf16":  # integers in [-256, 256]
        x = (rng.integers(-256, 257, (P, 1, n)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    else:
        x = fp8_model.draw_small(rng, dtype, (P, 1, n), bound=2.0)
        monkeypatch.setattr(plan_sim, "oracle", fp8_model.ModelOracle)
    want = x[:, 0]
    for _ in range(runs):
        want = [narrow(torch, dtype, sum(widen(torch, dtype, w).astype(np.float64) for w in want))] * P
    assert np.isfinite(widen(torch, dtype, want[0])).all()
    assert (want[0] != plan_sim.simulate(algo, "sum", dtype, x, runs=runs)[0, 0]).any()
    y = run_threads(torch, algo, "sum_wide", dtype, x, runs=runs)
    for r in range(P):
        assert (y[r, 0] == want[r]).all(), (r, np.flatnonzero(y[r, 0] != want[r])[:8])


def test_i32_is_refused_before_any_exchange(torch):
    """Rank 1 of the two never makes the call: a refusal that first exchanged
    anything with the peer would wait for it and time out instead."""
    import gloo_amd
    t = torch.zeros(1000, dtype=torch.int32, device="cuda")
    url, errors, done = "mem:" + uuid.uuid4().hex, [], threading.Event()

    def body(r):
        try:
            ctx = gloo_amd.Context(r, 2, url, device=0, timeout_ms=20000)
            calls = [lambda: gloo_amd.Algorithm(ctx, "ring_chunked", "sum_wide", "i32", [t.data_ptr()], t.numel()),
                     lambda: gloo_amd.allreduce(ctx, [t.data_ptr()], t.numel(), "i32", "sum_wide")]
            for call in calls if r == 0 else []:
                with pytest.raises(gloo_amd.GlooHipError, match="sum_wide.*i32") as e:
                    call()
                assert e.value.code == -1
            assert done.set() is None if r == 0 else done.wait(30)
            ctx.close()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            done.set()

    ts = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    [th.start() for th in ts]
    [th.join() for th in ts]
    assert not errors, errors
