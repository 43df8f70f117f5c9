"""GPU: stochastic rounding of quantise_mx and reduce_mx (include/gloo_amd.h "MX stochastic rounding") against the
numpy model of tests/mx_sr_model.py, byte for byte, and its share of upward roundings against the binomial bound."""
import uuid
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mx_model as mm
import mx_quant_model as qm
import mx_sr_model as sm
from test_fp8_gpu import torch  # noqa: F401  (the module's torch fixture)
from test_mx_gpu import draw
from test_mx_quant_gpu import as_dtype, check, guarded, wide_view

pytestmark = pytest.mark.gpu
SEEDS = (1, 0x1234_5678_9ABC_DEF0)
GRID = {f: t[np.isfinite(t)] for f, t in mm.TABLE.items()}
MIN_NORMAL = {"mxfp8_e4m3": 2.0 ** -6, "mxfp8_e5m2": 2.0 ** -14, "mxfp4_e2m1": 1.0}


def run_quantise(torch, fmt, dtype, x, seed):
    """quantise_mx of the model-form array x into guarded memory, the scale array one byte past an allocation."""
    import gloo_amd
    raw = torch.from_numpy(x.reshape(-1).view(np.uint8)).cuda()
    (de, e_ok), (ds, s_ok) = guarded(torch, x.size // 32 * mm.BLOCK_BYTES[fmt], 16), guarded(torch, x.size // 32, 1)
    gloo_amd.quantise_mx(fmt, (de, ds), wide_view(torch, dtype, raw), seed=seed)
    torch.cuda.synchronize()
    assert e_ok() and s_ok(), "wrote outside dst"
    return de.cpu().numpy(), ds.cpu().numpy()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("length", ["1", "T+3"])
@pytest.mark.parametrize("dtype", qm.DTYPES)
@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_quantise_is_the_model(torch, fmt, dtype, length, seed):
    import gloo_amd
    nblocks = 1 if length == "1" else gloo_amd.mx_quantise_tile_blocks(fmt, dtype) + 3
    rng = np.random.default_rng([11, mm.FORMATS.index(fmt), nblocks])
    x = rng.standard_normal((nblocks, 32)) * 2.0 ** rng.integers(-11, 11, (nblocks, 1))
    if nblocks > 7:  # one block per special
        x[0] = rng.standard_normal(32) * 2.0 ** -130                    # scale 0 (f16: all +-0)
        x[1] = rng.uniform(-1, 1, 32) * MIN_NORMAL[fmt]                 # the element's subnormal range ...
        x[2] = rng.choice(GRID[fmt], 32)                                # ... and its grid, ...
        x[3] = np.where(np.arange(32) % 2, -0.0, 0.0)                   # ... +-0, ...
        x[4] = np.where(np.arange(32) % 3, 1.0, -1.0) * 1.99 * 2.0 ** mm.EMAX[fmt]  # ... the clamp: scale 127 each
        x[1:4, 0] = GRID[fmt].max()
        x[5, 9], x[6, 30] = np.nan, -np.inf                             # scale 255
    x = as_dtype(dtype, x)
    want = sm.quantise(fmt, x, seed)
    assert nblocks == 1 or ((want[1][:7] == [0, 127, 127, 127, 127, 255, 255]).all() and (want[0] != qm.quantise(fmt, x)[0]).any())
    check((fmt, dtype, seed), run_quantise(torch, fmt, dtype, x, seed), want)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_fold_is_the_model(torch, fmt, inplace):
    """reduce_mx(seed=) over k = 3 sources, scale arrays one byte past an allocation; in place dst is source 0."""
    import gloo_amd
    srcs = draw(fmt, 3, gloo_amd.MX_TILE_BLOCKS[gloo_amd.MX_FORMAT_NAMES[fmt]] + 3, 12)
    want = sm.fold(fmt, srcs, SEEDS[1])
    assert (want[0] != mm.fold(fmt, srcs)[0]).any()
    dev = [(torch.from_numpy(e).cuda(), torch.from_numpy(np.concatenate([[0], s]).astype(np.uint8)).cuda()[1:]) for e, s in srcs]
    (de, e_ok), (ds, s_ok) = guarded(torch, srcs[0][0].size, 16), guarded(torch, srcs[0][1].size, 1)
    dst = gloo_amd.reduce_mx(fmt, dev[0] if inplace else (de, ds), dev, seed=SEEDS[1])
    torch.cuda.synchronize()
    for (te, ts), (e, s) in list(zip(dev, srcs))[1 if inplace else 0:]:
        assert (te.cpu().numpy() == e).all() and (ts.cpu().numpy() == s).all(), "a source was modified"
    assert e_ok() and s_ok(), "wrote outside dst"
    check((fmt, inplace), tuple(t.cpu().numpy() for t in dst), want)


@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_on_grid_input_ignores_the_seed(torch, fmt):
    """Table values (max normal first, so the scaled values are the table's) times a power of two per block."""
    rng = np.random.default_rng(13)
    x = rng.choice(GRID[fmt], (67, 32))
    x[:, 0] = GRID[fmt].max()
    x = as_dtype("f32", x * 2.0 ** rng.integers(-60, 60, (67, 1)))
    nearest = run_quantise(torch, fmt, "f32", x, None)
    for seed in SEEDS:
        check((fmt, seed), run_quantise(torch, fmt, "f32", x, seed), nearest)


@pytest.mark.parametrize("seed", [1, 2])
def test_unbiased(torch, seed):
    """e2m1: 1.3 lies 0.6 of the way from 1.0 to 1.5.  The share of 63488 elements stored as 1.5 is within six standard
    deviations of a binomial share, 6 * sqrt(0.6 * 0.4 / 63488) = 0.0117, of 0.6 (frac16 moves the target by less than
    2^-16).  The model's shares are 0.60003 (seed 1) and 0.59912 (seed 2)."""
    x = np.full((2048, 32), 1.3, np.float32)
    x[:, 0] = 4.0
    elems, scales = run_quantise(torch, "mxfp4_e2m1", "f32", x, seed)
    stored = mm.TABLE["mxfp4_e2m1"][mm.codes("mxfp4_e2m1", elems)][:, 1:]
    assert (scales == 127).all() and np.isin(stored, (1.0, 1.5)).all()
    print("share stored as 1.5:", (stored == 1.5).mean())
    assert abs((stored == 1.5).mean() - 0.6) <= 0.012


@pytest.mark.parametrize("fmt", mm.FORMATS)
def test_allreduce_via_mx_threads(torch, fmt):
    """P = 3 rank threads, 5 blocks of bf16, seed 7: rank r quantises with seed 7 + r, every rank ends with the wide fold."""
    import gloo_amd
    dtype, P, nblocks = "bf16", 3, 5
    rng = np.random.default_rng(14)
    xs = [as_dtype(dtype, rng.standard_normal((nblocks, 32)) * 2.0 ** rng.integers(-8, 8, (nblocks, 1))) for _ in range(P)]
    want = qm.fold_wide(fmt, dtype, [sm.quantise(fmt, x, 7 + r) for r, x in enumerate(xs)])
    assert (want != qm.fold_wide(fmt, dtype, [qm.quantise(fmt, x) for x in xs])).any()
    url = "mem:" + uuid.uuid4().hex

    def body(r):
        ctx = gloo_amd.Context(r, P, url, device=0, timeout_ms=20000)
        raw = torch.from_numpy(xs[r].reshape(-1).view(np.uint8)).cuda()
        e, s = (torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (nblocks * mm.BLOCK_BYTES[fmt], nblocks))
        ge, gs = (torch.zeros(P * x.numel(), dtype=torch.uint8, device="cuda") for x in (e, s))
        gloo_amd.allreduce_via_mx(ctx, fmt, wide_view(torch, dtype, raw), e, s, ge, gs, seed=7)
        torch.cuda.synchronize()
        ctx.close()
        return raw.cpu().numpy().view(np.uint16)

    with ThreadPoolExecutor(P) as pool:
        for r, got in enumerate(pool.map(body, range(P))):  # one model for all: the results are identical across ranks
            check((fmt, dtype, r), got, want)
