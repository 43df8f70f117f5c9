"""GPU: the MX block-scaled sum (gloo_amd.reduce_mx, include/gloo_amd.h "MX
block-scaled sum") against the numpy model of tests/mx_model.py, byte for
byte, elements and scales alike."""
import threading
import uuid

import numpy as np
import pytest

import mx_model as mm
from test_fp8_gpu import torch  # noqa: F401  (the module's torch fixture)

pytestmark = pytest.mark.gpu
LENGTHS = {"1": lambda T: 1, "2": lambda T: 2, "3": lambda T: 3, "T-1": lambda T: T - 1, "T": lambda T: T,
           "T+1": lambda T: T + 1, "2T+5": lambda T: 2 * T + 5}
GUARD = 0xA5


def draw(fmt, k, nblocks, seed):
    """Uniform element bytes without the element-NaN codes; per source and block a scale in [100, 150]."""
    rng = np.random.default_rng([seed, mm.FORMATS.index(fmt), k, nblocks])
    ok = np.flatnonzero(~np.isnan(mm.TABLE[fmt])).astype(np.uint8)
    elems = [mm.pack(fmt, rng.choice(ok, nblocks * 32).reshape(-1, 32)) for _ in range(k)]
    return [(e, rng.integers(100, 151, nblocks).astype(np.uint8)) for e in elems]


def run(torch, fmt, srcs, inplace=False):
    """reduce_mx with scale arrays one byte past an allocation; the sources and the bytes around dst must stay."""
    import gloo_amd
    ne, ns = srcs[0][0].size, srcs[0][1].size
    dev = []
    for e, s in srcs:
        se = torch.from_numpy(np.concatenate([[0], s]).astype(np.uint8)).cuda()
        dev.append((torch.from_numpy(e).cuda(), se[1:]))
    de, ds = (torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda") for n in (ne, ns + 1))
    dst = dev[0] if inplace else (de[:ne], ds[1:1 + ns])
    gloo_amd.reduce_mx(fmt, dst, dev)
    torch.cuda.synchronize()
    for (te, ts), (e, s) in list(zip(dev, srcs))[1 if inplace else 0:]:
        assert (te.cpu().numpy() == e).all() and (ts.cpu().numpy() == s).all(), "a source was modified"
    assert (de[ne:] == GUARD).all() and (ds[1 + ns:] == GUARD).all() and ds[0] == GUARD, "wrote outside dst"
    return dst[0].cpu().numpy(), dst[1].cpu().numpy()


def check(fmt, got, want):
    for name, g, w in zip(("elements", "scales"), got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (fmt, name, bad[:8], g[bad[:8]], w[bad[:8]])


@pytest.mark.parametrize("length", list(LENGTHS))
@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_fold_is_the_model(torch, fmt, k, length):
    import gloo_amd
    nblocks = LENGTHS[length](gloo_amd.MX_TILE_BLOCKS[gloo_amd.MX_FORMAT_NAMES[fmt]])
    srcs = draw(fmt, k, nblocks, 1)
    want = mm.fold(fmt, srcs)
    assert nblocks < 100 or (want[1] != 255).sum() > nblocks // 20  # e5m2's infinities leave enough finite blocks
    check(fmt, run(torch, fmt, srcs), want)


@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_in_place(torch, fmt):
    import gloo_amd
    srcs = draw(fmt, 3, gloo_amd.MX_TILE_BLOCKS[gloo_amd.MX_FORMAT_NAMES[fmt]] + 3, 2)
    check(fmt, run(torch, fmt, srcs, inplace=True), mm.fold(fmt, srcs))


@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_specials(torch, fmt):
    """k = 2, one block per case, in one launch."""
    fp4 = fmt == "mxfp4_e2m1"
    finite = np.flatnonzero(np.isfinite(mm.TABLE[fmt]))
    code = lambda v: int(finite[np.flatnonzero(mm.TABLE[fmt][finite] == v)[0]])  # noqa: E731  (+0 for 0)
    top = float(np.nanmax(mm.TABLE[fmt][finite]))                                  # max normal
    step, tiny, neg0 = {448.0: 32.0, 57344.0: 4096.0, 6.0: 1.0}[top], code(-mm.TABLE[fmt][1]), 8 if fp4 else 0x80
    rng = np.random.default_rng(3)
    small = lambda: rng.choice(finite[np.abs(mm.TABLE[fmt][finite]) <= 1], 32)  # noqa: E731
    z, cases = np.zeros(32, np.int64), []
    cases += [("all zero", z, 127, z, 3, 0), ("-0 elements", z + neg0, 127, z + neg0, 120, 0)]
    a, b = small(), z.copy()
    a[7], b[7] = code(top), code(step)
    cases.append(("amax mantissa forces the clamp", a, 130, b, 130, None))   # max + step < 2 * 2^emax
    a, b = z.copy(), z.copy()
    a[0], b[1] = code(top), tiny
    cases.append(("rounds to -0", a, 127, b, 90, None))
    if not fp4:
        cases.append(("a NaN element", np.where(np.arange(32) == 5, 0x7F, small()), 127, small(), 127, 255))
    cases.append(("a source with scale 255", small(), 127, small(), 255, 255))
    cases.append(("scales 0 and 1", rng.choice(finite, 32), 0, rng.choice(finite, 32), 1, None))
    cases.append(("the f32 sum overflows", a, 254, a, 254, 255))  # a: max normal and zeros, from "rounds to -0"
    srcs = [(mm.pack(fmt, np.stack([c[i] for c in cases])), np.array([c[i + 1] for c in cases], np.uint8)) for i in (1, 3)]
    want = mm.fold(fmt, srcs)
    for (name, *_, scale), w in zip(cases, want[1]):  # the model itself, where the contract names the scale
        assert scale is None or w == scale, (name, w)
    we = mm.codes(fmt, want[0])
    assert (we[1] == neg0).all() and we[2, 7] == code(top) and we[3, 1] == neg0 and (we[-1] == mm.NAN_BYTE[fmt]).all()
    check(fmt, run(torch, fmt, srcs), want)


def test_allreduce_mx_threads(torch):
    """P = 3 rank threads, 5 blocks of MXFP8 e4m3: every rank ends with the model of the inputs in rank order."""
    import gloo_amd
    fmt, P, nblocks = "mxfp8_e4m3", 3, 5
    srcs = draw(fmt, P, nblocks, 4)
    want = mm.fold(fmt, srcs)
    url, got, errors = "mem:" + uuid.uuid4().hex, [None] * P, []

    def body(r):
        try:
            ctx = gloo_amd.Context(r, P, url, device=0, timeout_ms=20000)
            e, s = (torch.from_numpy(x).cuda() for x in srcs[r])
            ge, gs = (torch.zeros(P * x.numel(), dtype=torch.uint8, device="cuda") for x in (e, s))
            gloo_amd.allreduce_mx(ctx, fmt, e, s, ge, gs)
            torch.cuda.synchronize()
            got[r] = (e.cpu().numpy(), s.cpu().numpy())
            ctx.close()
        except BaseException as ex:  # noqa: BLE001
            errors.append((r, repr(ex)))

    ts = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    for r in range(P):
        check(fmt, got[r], want)
