"""GPU: quantise_mx, reduce_mx_wide, dequantise_mx and allreduce_via_mx (include/gloo_amd.h "MX quantise and
wide-output fold") against the numpy model of tests/mx_quant_model.py, byte for byte."""
import uuid
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mx_model as mm
import mx_quant_model as qm
from test_fp8_gpu import torch  # noqa: F401  (the module's torch fixture)
from test_mx_gpu import draw as mx_draw

pytestmark = pytest.mark.gpu
GUARD = 0xA5
LENGTHS = {"1": lambda T: 1, "3": lambda T: 3, "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1,
           "2T+5": lambda T: 2 * T + 5}
# quantise: per block a power of two around standard normal values; f16 stays finite (6 sigma * 2^11 < 65504)
Q_EXPONENTS = {"f32": (-100, 100), "bf16": (-100, 100), "f16": (-11, 11)}
# wide fold: f32 and bf16 hold every product of test_mx_gpu.draw's scale range, f16 reaches from 2^-24 to 2^16
W_SCALES = {"f32": (100, 151), "bf16": (100, 151), "f16": (118, 131)}
MBITS = {"mxfp8_e4m3": 3, "mxfp8_e5m2": 2, "mxfp4_e2m1": 1}
INF_BITS = {"f32": 0x7F800000, "f16": 0x7C00, "bf16": 0x7F80}


def as_dtype(dtype, x):
    """f32 values in the model's form of `dtype` (bf16: truncated to uint16 bits)."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore"):
        return x if dtype == "f32" else x.astype(np.float16) if dtype == "f16" else (x.view(np.uint32) >> 16).astype(np.uint16)


def wide_view(torch, dtype, raw):
    return raw.view({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype])


def guarded(torch, nbytes, front):
    """nbytes of device memory between guard bytes, `front` bytes past an allocation: -> (inner, the guards are intact)."""
    whole = torch.full((front + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    return whole[front:front + nbytes], lambda: bool((whole[:front] == GUARD).all() and (whole[front + nbytes:] == GUARD).all())


def run_quantise(torch, fmt, dtype, x):
    """quantise_mx of the model-form array x; the scale array starts one byte past an allocation."""
    import gloo_amd
    raw = torch.from_numpy(x.reshape(-1).view(np.uint8)).cuda()
    (de, e_ok), (ds, s_ok) = guarded(torch, x.size // 32 * mm.BLOCK_BYTES[fmt], 16), guarded(torch, x.size // 32, 1)
    gloo_amd.quantise_mx(fmt, (de, ds), wide_view(torch, dtype, raw))
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == x.reshape(-1).view(np.uint8)).all(), "the source was modified"
    assert e_ok() and s_ok(), "wrote outside dst"
    return de.cpu().numpy(), ds.cpu().numpy()


def run_fold(torch, fmt, dtype, srcs):
    """reduce_mx_wide of the sources (scales one byte past an allocation) into guarded memory: -> the result's bits."""
    import gloo_amd
    dev = [(torch.from_numpy(e).cuda(), torch.from_numpy(np.concatenate([[0], s]).astype(np.uint8)).cuda()[1:]) for e, s in srcs]
    raw, ok = guarded(torch, srcs[0][1].size * 32 * (4 if dtype == "f32" else 2), 16)
    gloo_amd.reduce_mx_wide(fmt, wide_view(torch, dtype, raw), dev)
    torch.cuda.synchronize()
    for (te, ts), (e, s) in zip(dev, srcs):
        assert (te.cpu().numpy() == e).all() and (ts.cpu().numpy() == s).all(), "a source was modified"
    assert ok(), "wrote outside dst"
    return raw.cpu().numpy().view(np.uint32 if dtype == "f32" else np.uint16)


def check(what, got, want):
    for g, w in zip(got, want) if isinstance(want, tuple) else [(got, want)]:
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, bad.size, bad[:8], g[bad[:8]], w[bad[:8]])


def draw(fmt, k, nblocks, seed, scales):
    """test_mx_gpu.draw, its scale bytes of [100, 151) folded into [scales[0], scales[1])."""
    return [(e, (scales[0] + (s - 100) % (scales[1] - scales[0])).astype(np.uint8)) for e, s in mx_draw(fmt, k, nblocks, seed)]


@pytest.mark.parametrize("length", list(LENGTHS))
@pytest.mark.parametrize("dtype", qm.DTYPES)
@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_quantise_is_the_model(torch, fmt, dtype, length):
    import gloo_amd
    nblocks = LENGTHS[length](gloo_amd.mx_quantise_tile_blocks(fmt, dtype))
    rng = np.random.default_rng([5, mm.FORMATS.index(fmt), qm.DTYPES.index(dtype), nblocks])
    x = as_dtype(dtype, rng.standard_normal((nblocks, 32)) * 2.0 ** rng.integers(*Q_EXPONENTS[dtype], (nblocks, 1)))
    want = qm.quantise(fmt, x)
    assert (want[1] != 255).all()
    check((fmt, dtype), run_quantise(torch, fmt, dtype, x), want)


@pytest.mark.parametrize("dtype", qm.DTYPES)
@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_quantise_specials(torch, fmt, dtype):
    """One block per case, in one launch; the model is held to the scale the contract names first."""
    emax, fp4, half = mm.EMAX[fmt], fmt == "mxfp4_e2m1", 2.0 ** -(MBITS[fmt] + 1)
    top = float(np.nanmax(mm.TABLE[fmt][np.isfinite(mm.TABLE[fmt])]))
    top_code, neg0 = int(np.flatnonzero(mm.TABLE[fmt] == top)[0]), 8 if fp4 else 0x80
    big = 65504.0 if dtype == "f16" else np.finfo(np.float32).max  # bf16: truncated to its largest finite value
    rng = np.random.default_rng(6)
    block = lambda base, **at: np.array([at.get(f"i{i}", rng.standard_normal() if base is None else base)  # noqa: E731
                                         for i in range(32)])
    cases = [("all zero", block(0.0), 0), ("all -0", block(-0.0), 0),
             ("amax mantissa forces the clamp", block(None, i7=1.984375 * 2.0 ** emax), 127),
             ("rounds to -0", block(0.0, i0=top, i1=-2.0 ** -20), 127),
             ("ties to even", block(0.0, i0=2.0 ** emax, i1=1 + half, i2=1 + 3 * half, i3=-1 - half, i4=-1 - 3 * half), 127),
             ("an input NaN", block(None, i5=np.nan), 255), ("an input +inf", block(None, i9=np.inf), 255),
             ("the largest finite value", block(None, i3=big), (142 if dtype == "f16" else 254) - emax)]
    if dtype == "f32":
        cases.append(("denormals only", rng.integers(-2 ** 22, 2 ** 22, 32) * 2.0 ** -149, 0))
    x = as_dtype(dtype, np.stack([c[1] for c in cases]))
    want = qm.quantise(fmt, x)
    for (name, _, scale), w in zip(cases, want[1]):
        assert w == scale, (name, w)
    we = mm.codes(fmt, want[0])
    assert (we[1] == neg0).all() and we[2, 7] == top_code and we[3, 1] == neg0 and we[7, 3] == top_code
    assert we[4, 1] % 2 == 0 and we[4, 2] == we[4, 1] + 2 and we[4, 3] == we[4, 1] | neg0  # both ties went to the even code
    check((fmt, dtype), run_quantise(torch, fmt, dtype, x), want)


@pytest.mark.parametrize("length", ["1", "T-1", "T+1", "2T+5"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("dtype", qm.DTYPES)
@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_wide_fold_is_the_model(torch, fmt, dtype, k, length):
    import gloo_amd
    srcs = draw(fmt, k, LENGTHS[length](gloo_amd.mx_wide_tile_blocks(fmt, dtype)), 7, W_SCALES[dtype])
    want = qm.fold_wide(fmt, dtype, srcs)
    inf = INF_BITS[dtype]
    assert ((want & inf != inf) & (want << 1 != 0)).sum() * 4 >= want.size  # a quarter is finite and non-zero
    check((fmt, dtype, k), run_fold(torch, fmt, dtype, srcs), want)


@pytest.mark.parametrize("dtype", qm.DTYPES)
@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_wide_fold_specials(torch, fmt, dtype):
    """k = 2, one block per case, in one launch."""
    fp4 = fmt == "mxfp4_e2m1"
    finite = np.flatnonzero(np.isfinite(mm.TABLE[fmt]))
    top_code, neg0 = int(finite[np.argmax(mm.TABLE[fmt][finite])]), 8 if fp4 else 0x80
    rng = np.random.default_rng(8)
    some = lambda: rng.choice(finite, 32)  # noqa: E731
    z = np.zeros(32, np.int64)
    cases = [("a source with scale 255", np.where(np.arange(32) % 2, some(), 0), 127, some(), 255),
             ("the f32 sum overflows", z + top_code, 254, z + top_code, 254),
             ("above the f16 range", z + top_code, 143, z, 127),
             ("scales 0 and 1", some(), 0, some(), 1),
             ("-0 + -0", z + neg0, 127, z + neg0, 120)]
    if not fp4:
        cases.append(("a NaN element", np.where(np.arange(32) == 5, 0x7F, some()), 127, some(), 127))
    if fmt == "mxfp8_e5m2":
        cases.append(("inf - inf", z + 0x7C, 127, z + 0xFC, 127))
    srcs = [(mm.pack(fmt, np.stack([c[i] for c in cases])), np.array([c[i + 1] for c in cases], np.uint8)) for i in (1, 3)]
    want = qm.fold_wide(fmt, dtype, srcs).reshape(-1, 32)
    nan, inf, sign = qm.CANONICAL_NAN[dtype], INF_BITS[dtype], 0x80000000 if dtype == "f32" else 0x8000
    assert (want[0] == nan).all() and (want[1] == inf).all() and (want[4] == sign).all()
    assert (want[2] == inf).all() == (dtype == "f16") and (fp4 or want[5, 5] == nan)
    assert fmt != "mxfp8_e5m2" or (want[6] == nan).all()
    assert dtype != "f32" or ((want[3] & inf == 0) & (want[3] << 1 != 0)).any()  # denormal sums are kept
    check((fmt, dtype), run_fold(torch, fmt, dtype, srcs), want.reshape(-1))


@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_round_trip_is_reduce_mx(torch, fmt):
    """f32: quantise_mx(dequantise_mx(src)) is reduce_mx([src]), elements and scales; no model involved."""
    import gloo_amd
    nblocks = gloo_amd.MX_TILE_BLOCKS[gloo_amd.MX_FORMAT_NAMES[fmt]] + 3
    src = tuple(torch.from_numpy(a).cuda() for a in draw(fmt, 1, nblocks, 9, (0, 255))[0])
    wide = torch.empty(nblocks * 32, dtype=torch.float32, device="cuda")
    via, direct = [(torch.empty_like(src[0]), torch.empty_like(src[1])) for _ in range(2)]
    gloo_amd.quantise_mx(fmt, via, gloo_amd.dequantise_mx(fmt, wide, src))
    gloo_amd.reduce_mx(fmt, direct, [src])
    torch.cuda.synchronize()
    check(fmt, tuple(t.cpu().numpy() for t in via), tuple(t.cpu().numpy() for t in direct))


def test_allreduce_via_mx_threads(torch):
    """P = 3 rank threads, 5 blocks of bf16 through MXFP8 e4m3: every rank ends with the wide fold of the quantised inputs."""
    import gloo_amd
    fmt, dtype, P, nblocks = "mxfp8_e4m3", "bf16", 3, 5
    rng = np.random.default_rng(10)
    xs = [as_dtype(dtype, rng.standard_normal((nblocks, 32)) * 2.0 ** rng.integers(-8, 8, (nblocks, 1))) for _ in range(P)]
    want = qm.fold_wide(fmt, dtype, [qm.quantise(fmt, x) for x in xs])
    url = "mem:" + uuid.uuid4().hex

    def body(r):
        ctx = gloo_amd.Context(r, P, url, device=0, timeout_ms=20000)
        raw = torch.from_numpy(xs[r].reshape(-1).view(np.uint8)).cuda()
        e, s = (torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (nblocks * 32, nblocks))
        ge, gs = (torch.zeros(P * x.numel(), dtype=torch.uint8, device="cuda") for x in (e, s))
        gloo_amd.allreduce_via_mx(ctx, fmt, wide_view(torch, dtype, raw), e, s, ge, gs)
        torch.cuda.synchronize()
        ctx.close()
        return raw.cpu().numpy().view(np.uint16)

    with ThreadPoolExecutor(P) as pool:
        for r, got in enumerate(pool.map(body, range(P))):
            check((fmt, dtype, r), got, want)
