"""GPU, one process: gloo_hip_gather_fanout_kernel (reduce.hip
gather_fanout_kernel, the allgather sender's pass without its flags) against
numpy.

S sources of `bytes` bytes each go to n destinations, source i at dst + i *
bytes.  Sizes: 0, 1, 15, 16, 17 (the head / tail byte path of the 16-byte
packets), 16383, 16384, 16385 (one 16 KiB tile +- 1) and 3 * 16384 + 5 (several
tiles per source).  Sources and destinations start 0, 1, 3 or 15 bytes past a
256-byte boundary, rotated per case so that every (source, destination) pair
meets different misalignments, and i * bytes adds its own.  blocks = 2 forces
several grid-stride passes over the (source, tile) space, and the split of a
workgroup's walk across sources, at sizes where the default grid has one
workgroup per tile.  Guard bytes in front of and behind every destination must
stay intact, and the sources unmodified.  With S = 1 the destinations must be
byte-identical to gloo_hip_fanout_kernel's.
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
    cap = GUARD + 16 + 8 * SIZES[-1] + GUARD
    bufs = dict(src=[hip_rt.malloc(cap) for _ in range(8)], dst=[hip_rt.malloc(cap) for _ in range(8)],
                ref=[hip_rt.malloc(cap) for _ in range(8)])
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


def image(hip_rt, raw, off, nbytes):
    return hip_rt.d2h(raw, np.empty(GUARD + off + nbytes + GUARD, np.uint8))


@pytest.mark.parametrize("blocks", (0, 2))
@pytest.mark.parametrize("n", (1, 3, 8))
@pytest.mark.parametrize("S", (1, 2, 3, 8))
def test_against_numpy(dev, S, n, blocks):
    gloo_amd, hip_rt, bufs = dev
    rng = np.random.default_rng(100 * S + 10 * n + blocks)
    for nbytes in SIZES:
        for c in range(len(OFFS)):
            soff = [OFFS[(i + c) % 4] for i in range(S)]
            doff = [OFFS[(j + 2 * c + 1) % 4] for j in range(n)]
            srcs = [payload(rng, nbytes) for _ in range(S)]
            sp = [place(hip_rt, bufs["src"][i], soff[i], srcs[i]) for i in range(S)]
            blank = np.full(S * nbytes, FILL, np.uint8)
            dp = [place(hip_rt, bufs["dst"][j], doff[j], blank) for j in range(n)]
            gloo_amd.gather_fanout_kernel(dp, sp, nbytes, blocks=blocks)
            hip_rt.synchronize()
            want_body = np.concatenate(srcs) if nbytes else blank
            what = (S, n, blocks, nbytes, soff, doff)
            for j in range(n):
                got = image(hip_rt, bufs["dst"][j], doff[j], S * nbytes)
                want = np.full(got.size, FILL, np.uint8)
                want[GUARD + doff[j]:GUARD + doff[j] + S * nbytes] = want_body
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (what, "destination", j, "first bad byte", int(bad[0]) - GUARD - doff[j],
                                       int(got[bad[0]]), int(want[bad[0]]), bad.size)
            for i in range(S):
                got = image(hip_rt, bufs["src"][i], soff[i], nbytes)
                assert (got[GUARD + soff[i]:GUARD + soff[i] + nbytes] == srcs[i]).all(), (what, "source", i)
                assert (got[:GUARD + soff[i]] == FILL).all() and (got[GUARD + soff[i] + nbytes:] == FILL).all()


@pytest.mark.parametrize("blocks", (0, 2))
@pytest.mark.parametrize("n", (1, 3, 8))
def test_one_source_is_the_fanout_kernel(dev, n, blocks):
    gloo_amd, hip_rt, bufs = dev
    rng = np.random.default_rng(7 * n + blocks)
    for nbytes in SIZES:
        for c in range(len(OFFS)):
            soff = OFFS[c]
            doff = [OFFS[(j + 2 * c + 1) % 4] for j in range(n)]
            src = payload(rng, nbytes)
            sp = place(hip_rt, bufs["src"][0], soff, src)
            blank = np.full(nbytes, FILL, np.uint8)
            dp = [place(hip_rt, bufs["dst"][j], doff[j], blank) for j in range(n)]
            rp = [place(hip_rt, bufs["ref"][j], doff[j], blank) for j in range(n)]
            gloo_amd.gather_fanout_kernel(dp, [sp], nbytes, blocks=blocks)
            gloo_amd.fanout_kernel(rp, sp, nbytes, blocks=blocks)
            hip_rt.synchronize()
            for j in range(n):
                a = image(hip_rt, bufs["dst"][j], doff[j], nbytes)
                b = image(hip_rt, bufs["ref"][j], doff[j], nbytes)
                assert (a == b).all(), (n, blocks, nbytes, soff, doff, "destination", j)
                assert (a[GUARD + doff[j]:GUARD + doff[j] + nbytes] == src).all()


def test_refusals(dev):
    gloo_amd, hip_rt, bufs = dev
    with pytest.raises(gloo_amd.GlooHipError):
        gloo_amd.gather_fanout_kernel([bufs["dst"][0]] * 9, [bufs["src"][0]], 16)
    with pytest.raises(gloo_amd.GlooHipError):
        gloo_amd.gather_fanout_kernel([bufs["dst"][0]], [bufs["src"][0]] * 9, 16)
    with pytest.raises(gloo_amd.GlooHipError):
        gloo_amd.gather_fanout_kernel([bufs["dst"][0]], [0], 16)
