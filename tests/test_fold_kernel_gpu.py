"""GPU, one process: gloo_hip_fold_kernel (reduce.hip reduce_multi_vec_kernel
with plain stores, and fold_send_kernel) against tests/fold_model.py, bit for
bit.  Nothing here waits on a flag: every launch runs to completion alone.

A tile is 512 lanes x 2 x 16 B = 16 KiB; with es the element size, T = 16384 /
es elements fill one and kV = 16 / es one packet.  Sizes: 1, kV - 1, kV, kV + 1
(head / tail elements only, one packet), T - 1, T, T + 1 (grid 1 -> 2) and
3 * T + kV + 3 (several workgroups, head and tail both present under a
misaligned dst).  dst, every source and every forward start 0, es, 16 - es or
8 bytes past a 256-byte boundary (8-byte types: 0 or 8), rotated per case so
that each run has a source and a forward at another residue than dst, besides
the all-aligned case.  GUARD bytes of 0xA5 in front of and behind every
destination must stay intact and the sources unmodified.  A destination's body
is pre-filled with the complement of the expected bytes, so an element the
kernel never wrote cannot pass.
"""
import numpy as np
import pytest

import fold_model as fm

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
TILE = 16384
MAXB = 3 * TILE + 16 + 3 * 8  # bytes of the largest case


def sizes(es):
    T, kV = TILE // es, 16 // es
    return [n for n in (1, kV - 1, kV, kV + 1, T - 1, T, T + 1, 3 * T + kV + 3) if n > 0]


def offsets(es):
    out = []
    for o in (0, es, 16 - es, 8):
        if o % es == 0 and o not in out:
            out.append(o)
    return out


def offset_cases(es, k, nfwd):
    """(dst, sources, forwards) byte offsets: all aligned, then dst at each
    offset in turn with source 0 and forward 0 at the next one (another
    residue than dst) and the others rotated on."""
    O = offsets(es)
    L = len(O)
    yield 0, [0] * k, [0] * nfwd
    for c in range(L):
        yield O[c], [O[(c + 1 + i) % L] for i in range(k)], [O[(c + 1 + 3 * r) % L] for r in range(nfwd)]


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gloo_amd
    import hip_rt
    hip_rt.set_device(0)
    cap = GUARD + 16 + MAXB + GUARD
    bufs = dict(src=[hip_rt.malloc(cap) for _ in range(8)], dst=[hip_rt.malloc(cap)],
                fwd=[hip_rt.malloc(cap) for _ in range(8)], ref=[hip_rt.malloc(cap)], words=[hip_rt.malloc(512)])
    yield gloo_amd, hip_rt, bufs
    for v in bufs.values():
        for p in v:
            hip_rt.free(p)


_cases = {}


def case(op, dtype, k, n, seed=0):
    """Sources and the model's fold in every valid mode, computed once."""
    key = (op, dtype, k, n, seed)
    if key not in _cases:
        rng = np.random.default_rng([seed, k, n, fm.DTYPES.index(dtype), fm.ops_of(dtype).index(op)])
        srcs = fm.inputs(op, dtype, k, n, rng)
        modes = (0, 1, 2) if k & (k - 1) == 0 else (0, 1)
        _cases[key] = srcs, {m: fm.fold(op, dtype, srcs, m).view(np.uint8) for m in modes}
    return _cases[key]


def place(hip_rt, raw, off, body):
    """FILL, then `body` (bytes) at raw + GUARD + off; returns the pointer to it."""
    img = np.full(GUARD + off + body.size + GUARD, FILL, np.uint8)
    img[GUARD + off:GUARD + off + body.size] = body
    hip_rt.h2d(raw, img)
    return raw + GUARD + off


def check(hip_rt, raw, off, want, what, es):
    """The whole image: guards intact, body == want; first bad element in the message."""
    got = hip_rt.d2h(raw, np.empty(GUARD + off + want.size + GUARD, np.uint8))
    img = np.full(got.size, FILL, np.uint8)
    img[GUARD + off:GUARD + off + want.size] = want
    bad = np.flatnonzero(got != img)
    if bad.size:
        b = int(bad[0]) - GUARD - off
        where = f"element {b // es}" if 0 <= b < want.size else f"guard byte {b}"
        raise AssertionError(f"{what}: first bad byte {b} ({where}) got {int(got[bad[0]]):#04x} "
                             f"want {int(img[bad[0]]):#04x}, {bad.size} bad bytes")


def launch_and_check(dev, op, dtype, sp, n, mode, want, doff, foffs, what, dst_body=None, flags=None, values=None,
                     ticket=0, credit=False):
    """One launch into a fresh destination and fresh forwards; dst_body: what
    dst holds before (in place: a source), default the complement of want."""
    gloo_amd, hip_rt, bufs = dev
    es = fm.itemsize(dtype)
    blank = ~want
    dp = place(hip_rt, bufs["dst"][0], doff, blank if dst_body is None else dst_body)
    fp = [place(hip_rt, bufs["fwd"][r], foffs[r], blank) for r in range(len(foffs))]
    srcs = [dp if p is None else p for p in sp]  # None: the in-place source
    gloo_amd.fold_kernel(op, dtype, dp, srcs, n, mode=mode, fwd=fp + ([0] if credit else []), fwd_flags=flags,
                         fwd_values=values, ticket=ticket)
    hip_rt.synchronize()
    check(hip_rt, bufs["dst"][0], doff, want, what + ("dst",), es)
    for r in range(len(foffs)):
        check(hip_rt, bufs["fwd"][r], foffs[r], want, what + ("forward", r), es)


def place_sources(dev, srcs, soffs, skip=()):
    gloo_amd, hip_rt, bufs = dev
    return [None if i in skip else place(hip_rt, bufs["src"][i], soffs[i], srcs[i].view(np.uint8))
            for i in range(len(srcs))]


def check_sources(dev, srcs, soffs, what, dtype, skip=()):
    gloo_amd, hip_rt, bufs = dev
    for i in range(len(srcs)):
        if i not in skip:
            check(hip_rt, bufs["src"][i], soffs[i], srcs[i].view(np.uint8), what + ("source", i), fm.itemsize(dtype))


@pytest.mark.parametrize("dtype,op", [(d, o) for d in fm.DTYPES for o in fm.ops_of(d)])
def test_every_dtype_and_op(dev, dtype, op):
    """Modes 0, 1, 2 at k = 4, one tile and a bit, dst misaligned by one
    element, alone and with two forwards.  A signed dtype's bitwise op runs the
    unsigned twin's kernel: the raw bytes are compared."""
    es = fm.itemsize(dtype)
    k, n = 4, TILE // es + 16 // es + 3
    srcs, want = case(op, dtype, k, n)
    O = offsets(es)
    doff = es
    soffs = [O[(2 + i) % len(O)] for i in range(k)]
    foffs = [O[(2 + 3 * r) % len(O)] for r in range(2)] if len(O) > 2 else [0, 8]
    assert any(s % 16 != doff % 16 for s in soffs) and any(f % 16 != doff % 16 for f in foffs)
    sp = place_sources(dev, srcs, soffs)
    for mode in (0, 1, 2):
        for nfwd in (0, 2):
            launch_and_check(dev, op, dtype, sp, n, mode, want[mode], doff, foffs[:nfwd],
                             (dtype, op, "mode", mode, "nfwd", nfwd))
    check_sources(dev, srcs, soffs, (dtype, op), dtype)


SHAPE_CASES = [("u8", "sum"), ("bf16", "sum"), ("f32", "sum"), ("f64", "sum"), ("f32", "max")]


@pytest.mark.parametrize("k", (1, 2, 3, 5, 8))
@pytest.mark.parametrize("dtype,op", SHAPE_CASES)
def test_shapes_and_misalignment(dev, dtype, op, k):
    es = fm.itemsize(dtype)
    for n in sizes(es):
        srcs, want = case(op, dtype, k, n)
        for doff, soffs, foffs in offset_cases(es, k, 8):
            sp = place_sources(dev, srcs, soffs)
            for mode in want:
                for nfwd in (0, 1, 3, 8):
                    launch_and_check(dev, op, dtype, sp, n, mode, want[mode], doff, foffs[:nfwd],
                                     (dtype, op, "k", k, "n", n, "mode", mode, "nfwd", nfwd, "offsets", doff, soffs,
                                      foffs[:nfwd]))
            check_sources(dev, srcs, soffs, (dtype, op, "k", k, "n", n, "offsets", doff, soffs), dtype)


@pytest.mark.parametrize("alias", ("first", "last"))
@pytest.mark.parametrize("dtype,op", [("u8", "sum"), ("f16", "sum"), ("f32", "sum"), ("f32", "max"), ("f64", "min"),
                                      ("f8e4m3", "max"), ("u32", "bxor")])
def test_in_place(dev, dtype, op, alias):
    """dst is srcs[0] (the executor folds into output 0) or srcs[k-1]; the
    other sources sit at another residue.  Only the aliased source may change."""
    es = fm.itemsize(dtype)
    k = 4
    a = 0 if alias == "first" else k - 1
    O = offsets(es)
    for n in (16 // es + 1, TILE // es + 1, 3 * (TILE // es) + 16 // es + 3):
        srcs, want = case(op, dtype, k, n, seed=1)
        for c, doff in enumerate(O):
            soffs = [O[(c + 1 + i) % len(O)] for i in range(k)]
            soffs[a] = doff
            foffs = [O[(c + 1) % len(O)], doff]
            sp = place_sources(dev, srcs, soffs, skip=(a,))
            for mode in (0, 1, 2):
                for nfwd in (0, 2):
                    launch_and_check(dev, op, dtype, sp, n, mode, want[mode], doff, foffs[:nfwd],
                                     (dtype, op, alias, "n", n, "mode", mode, "nfwd", nfwd, "offsets", doff, soffs),
                                     dst_body=srcs[a].view(np.uint8))
            check_sources(dev, srcs, soffs, (dtype, op, alias, "n", n), dtype, skip=(a,))


def grid_of(n, es, doff):
    kV = 16 // es
    head = min(((16 - doff % 16) % 16) // es, n)
    return max(1, -(-((n - head) // kV) // 1024))


@pytest.mark.parametrize("doff", (0, 4))
def test_forward_flags_and_ticket(dev, doff):
    """Two forwards with flags and one credit: after the launch every flag
    holds its value and the ticket word is 0 again, so a second launch on the
    same ticket publishes its own values; an entry without a flag leaves its
    word alone.  No polling: launch, synchronize, read back."""
    gloo_amd, hip_rt, bufs = dev
    dtype, op, k, es = "f32", "sum", 3, 4
    T = TILE // es
    ns = (T, T + 4 + 3, 3 * T + 4 + 3)
    assert [grid_of(n, es, doff) for n in ns] == [1, 2, 4]
    words = bufs["words"][0]
    flag = [words + 64 + 8 * r for r in range(3)]
    ticket = words + 256

    def read_words():
        img = hip_rt.d2h(words, np.empty(512, np.uint8))
        f = img[64:88].view(np.uint64)
        t = int(img[256:260].view(np.uint32)[0])
        rest = np.concatenate([img[:64], img[88:256], img[260:]])
        assert (rest == FILL).all(), "bytes around the flag and ticket words changed"
        return [int(x) for x in f], t

    for n in ns:
        img = np.full(512, FILL, np.uint8)
        img[64:88] = 0
        img[256:260] = 0
        hip_rt.h2d(words, img)
        srcs, want = case(op, dtype, k, n, seed=2)
        soffs, foffs = [8, 0, 12], [12, doff]
        sp = place_sources(dev, srcs, soffs)
        what = ("n", n, "dst offset", doff)
        first, second, third = [11, 1 << 40, 13], [21, 22, (1 << 64) - 1], [31, 32, 33]
        launch_and_check(dev, op, dtype, sp, n, 0, want[0], doff, foffs, what + ("first",), flags=flag, values=first,
                         ticket=ticket, credit=True)
        assert read_words() == (first, 0), what
        launch_and_check(dev, op, dtype, sp, n, 1, want[1], doff, foffs, what + ("second",), flags=flag,
                         values=second, ticket=ticket, credit=True)
        assert read_words() == (second, 0), what
        # forward 1 without a flag: its word keeps the second launch's value
        launch_and_check(dev, op, dtype, sp, n, 0, want[0], doff, foffs, what + ("third",),
                         flags=[flag[0], 0, flag[2]], values=third, ticket=ticket, credit=True)
        assert read_words() == ([third[0], second[1], third[2]], 0), what
        check_sources(dev, srcs, soffs, what, dtype)


@pytest.mark.parametrize("dtype,op", [("u8", "sum"), ("bf16", "product"), ("f32", "sum"), ("f64", "max"),
                                      ("f8e5m2", "sum"), ("i64", "band")])
def test_matches_reduce_multi(dev, dtype, op):
    """Mode 0 alone makes gloo_hip_reduce_multi's bytes (plain against `nt` stores)."""
    gloo_amd, hip_rt, bufs = dev
    es = fm.itemsize(dtype)
    k = 5
    for n in (TILE // es + 16 // es + 3, 3 * (TILE // es) + 16 // es + 3):
        srcs, want = case(op, dtype, k, n, seed=3)
        O = offsets(es)
        doff, soffs = O[1], [O[i % len(O)] for i in range(k)]
        sp = place_sources(dev, srcs, soffs)
        launch_and_check(dev, op, dtype, sp, n, 0, want[0], doff, [], (dtype, op, "n", n))
        rp = place(hip_rt, bufs["ref"][0], doff, ~want[0])
        gloo_amd.reduce_multi_ptr(op, dtype, rp, sp, n)
        hip_rt.synchronize()
        a = hip_rt.d2h(bufs["dst"][0], np.empty(GUARD + doff + n * es + GUARD, np.uint8))
        b = hip_rt.d2h(bufs["ref"][0], np.empty(GUARD + doff + n * es + GUARD, np.uint8))
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (dtype, op, n, "first bad byte", int(bad[0]) - GUARD - doff)
