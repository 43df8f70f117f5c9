"""GPU, one process: gloo_hip_copy_kernel and gloo_hip_copy_kernel_multi
(reduce.hip copy_signal_kernel without a flag, the SEND steps' copy engine)
against numpy.

Sizes: 0, 1, 15, 16, 17 (the head / tail byte path of the 16-byte packets),
16383, 16384, 16385 (one 16 KiB tile +- 1) and 3 * 16384 + 5 (several tiles).
Source and destination start 0, 1, 3 or 15 bytes past a 256-byte boundary,
independently (all 16 pairs).  blocks = 2 forces the grid stride over tiles at
sizes where the default grid has one workgroup per tile.  The multi form takes
1, 3 or 8 entries of different sizes in one launch, zero-byte entries among
them (skipped by the entry point) and all entries empty (no launch).  Guard
bytes in front of and behind every destination must stay intact, and the
sources unmodified.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 15, 16, 17, 16383, 16384, 16385, 3 * 16384 + 5)
OFFS = (0, 1, 3, 15)
GUARD, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gloo_amd
    import hip_rt
    hip_rt.set_device(0)
    cap = GUARD + 16 + SIZES[-1] + GUARD
    bufs = dict(src=[hip_rt.malloc(cap) for _ in range(8)], dst=[hip_rt.malloc(cap) for _ in range(8)])
    yield gloo_amd, hip_rt, bufs
    for v in bufs.values():
        for p in v:
            hip_rt.free(p)


def payload(rng, nbytes):
    b = rng.integers(0, 256, nbytes, dtype=np.uint8)
    b[b == FILL] = 0  # never the guard fill, so an unwritten byte cannot pass
    return b


def place(hip_rt, raw, off, body):
    """FILL, then `body` at raw + GUARD + off; returns the pointer to it."""
    img = np.full(GUARD + off + body.size + GUARD, FILL, np.uint8)
    img[GUARD + off:GUARD + off + body.size] = body
    hip_rt.h2d(raw, img)
    return raw + GUARD + off


def check(hip_rt, raw, off, want, what):
    got = hip_rt.d2h(raw, np.empty(GUARD + off + want.size + GUARD, np.uint8))
    img = np.full(got.size, FILL, np.uint8)
    img[GUARD + off:GUARD + off + want.size] = want
    bad = np.flatnonzero(got != img)
    assert bad.size == 0, (what, "first bad byte", int(bad[0]) - GUARD - off, int(got[bad[0]]), int(img[bad[0]]),
                           bad.size)


@pytest.mark.parametrize("blocks", (0, 2))
def test_copy_kernel_against_numpy(dev, blocks):
    gloo_amd, hip_rt, bufs = dev
    rng = np.random.default_rng(40 + blocks)
    for nbytes in SIZES:
        for soff in OFFS:
            for doff in OFFS:
                src = payload(rng, nbytes)
                sp = place(hip_rt, bufs["src"][0], soff, src)
                dp = place(hip_rt, bufs["dst"][0], doff, np.full(nbytes, FILL, np.uint8))
                gloo_amd.copy_kernel(dp, sp, nbytes, blocks=blocks)
                hip_rt.synchronize()
                what = (blocks, nbytes, soff, doff)
                check(hip_rt, bufs["dst"][0], doff, src, what + ("destination",))
                check(hip_rt, bufs["src"][0], soff, src, what + ("source",))


@pytest.mark.parametrize("blocks", (0, 2))
@pytest.mark.parametrize("n", (1, 3, 8))
def test_copy_kernel_multi_against_numpy(dev, n, blocks):
    """Entry j copies SIZES[(2 * j + c) % 9] bytes, so one launch mixes empty,
    sub-packet, one-tile and several-tile entries; offsets rotate per entry."""
    gloo_amd, hip_rt, bufs = dev
    rng = np.random.default_rng(10 * n + blocks)
    for c in range(len(SIZES)):
        for o in range(len(OFFS)):
            sizes = [SIZES[(2 * j + c) % len(SIZES)] for j in range(n)]
            soff = [OFFS[(j + o) % 4] for j in range(n)]
            doff = [OFFS[(j + 2 * o + 1) % 4] for j in range(n)]
            srcs = [payload(rng, sizes[j]) for j in range(n)]
            sp = [place(hip_rt, bufs["src"][j], soff[j], srcs[j]) for j in range(n)]
            dp = [place(hip_rt, bufs["dst"][j], doff[j], np.full(sizes[j], FILL, np.uint8)) for j in range(n)]
            gloo_amd.copy_kernel_multi(dp, sp, sizes, blocks=blocks)
            hip_rt.synchronize()
            what = (n, blocks, sizes, soff, doff)
            for j in range(n):
                check(hip_rt, bufs["dst"][j], doff[j], srcs[j], what + ("destination", j))
                check(hip_rt, bufs["src"][j], soff[j], srcs[j], what + ("source", j))


@pytest.mark.parametrize("n", (1, 3, 8))
def test_copy_kernel_multi_one_size_and_all_empty(dev, n):
    """nbytes as one number: every entry that size; all entries empty: no
    launch, nothing written, null pointers allowed."""
    gloo_amd, hip_rt, bufs = dev
    rng = np.random.default_rng(70 + n)
    for nbytes in (17, 16385):
        srcs = [payload(rng, nbytes) for _ in range(n)]
        sp = [place(hip_rt, bufs["src"][j], OFFS[j % 4], srcs[j]) for j in range(n)]
        dp = [place(hip_rt, bufs["dst"][j], OFFS[(j + 1) % 4], np.full(nbytes, FILL, np.uint8)) for j in range(n)]
        gloo_amd.copy_kernel_multi(dp, sp, nbytes)
        hip_rt.synchronize()
        for j in range(n):
            check(hip_rt, bufs["dst"][j], OFFS[(j + 1) % 4], srcs[j], (n, nbytes, "destination", j))
    blank = np.full(64, FILL, np.uint8)
    dp = [place(hip_rt, bufs["dst"][j], 0, blank) for j in range(n)]
    gloo_amd.copy_kernel_multi(dp, [bufs["src"][j] for j in range(n)], [0] * n)
    gloo_amd.copy_kernel_multi([0] * n, [0] * n, 0)
    gloo_amd.copy_kernel(0, 0, 0)
    hip_rt.synchronize()
    for j in range(n):
        check(hip_rt, bufs["dst"][j], 0, blank, (n, "all empty", j))


def test_refusals(dev):
    gloo_amd, hip_rt, bufs = dev
    d, s = bufs["dst"][0], bufs["src"][0]
    with pytest.raises(gloo_amd.GlooHipError) as e:
        gloo_amd.copy_kernel_multi([], [], [])
    assert e.value.code == -4
    with pytest.raises(gloo_amd.GlooHipError) as e:
        gloo_amd.copy_kernel_multi([d] * 9, [s] * 9, 16)
    assert e.value.code == -4
    for dsts, srcs in (([d, 0], [s, s]), ([d, d], [s, 0])):
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.copy_kernel_multi(dsts, srcs, [0, 16])
        assert e.value.code == -3
    for dp, sp in ((0, s), (d, 0)):
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.copy_kernel(dp, sp, 16)
        assert e.value.code == -3
