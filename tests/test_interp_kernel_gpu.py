"""GPU, one process: gloo_hip_interp_kernel (reduce.hip plan_interp_kernel with
interp_copy and interp_fold) against tests/interp_model.py, bit for bit.

Every wait here is one that an earlier step of the same list, or the host
before the launch, has already satisfied (timeout 10^7 ticks, 0.1 s), but for
the one bounded case at the end (2 * 10^5 ticks, 2 ms), whose wait nobody meets.

Sizes (tests/interp_model.py copy_sizes / fold_sizes / sliced_sizes): with kV =
16 / es, CP = 65536 bytes a copy pass and FP = 8192 (es = 1) or 32768 bytes a
fold pass -- the defaults of GLOO_AMD_INTERP_BLOCK, _COPY_UNROLL and
_FOLD_UNROLL; another build needs other sizes -- copies of 1, 15, 16, 17, CP -
1, CP, CP + 1 and 2 CP + 16 + 3 bytes and folds of 1, kV - 1, kV, kV + 1, FP /
es - 1, FP / es, FP / es + 1 and 2 FP / es + kV + 3 elements.  dst, every source
and every extra destination start 0, es, 16 - es or 8 bytes past a 256-byte
boundary, rotated per case so that each run has a source and an extra
destination at another residue than dst, besides the all-aligned case.

The harness is tests/guard_rig.py: 256 guard bytes of 0xA5 around every buffer
and around the flag, done, ticket and err words; a destination no step's source
is pre-filled with the complement of the expected bytes; sources are checked
unmodified; whole images are compared.
"""
import ctypes

import numpy as np
import pytest

import fold_model as fm
import guard_rig
import interp_model as im
from interp_model import COPY, FOLD, SEND, SIGNAL, WAIT, Step

pytestmark = pytest.mark.gpu

MAXB = 2 * im.CP + 16 * 8 + 3 * 8  # bytes of the largest case
TIMEOUT = 10 ** 7


def offsets(es):
    out = []
    for o in (0, es, 16 - es, 8):
        if o % es == 0 and o not in out:
            out.append(o)
    return out


def offset_cases(es, k, nx):
    """(dst, sources, extra destinations) byte offsets: all aligned, then dst
    at each offset in turn with source 0 and extra destination 0 at the next one
    (another residue than dst) and the others rotated on."""
    O = offsets(es)
    L = len(O)
    yield 0, [0] * k, [0] * nx
    for c in range(L):
        yield O[c], [O[(c + 1 + i) % L] for i in range(k)], [O[(c + 1 + 3 * r) % L] for r in range(nx)]


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gloo_amd
    import hip_rt
    hip_rt.set_device(0)
    rig = guard_rig.Rig(hip_rt, guard_rig.GUARD + 16 + MAXB + guard_rig.GUARD)
    yield gloo_amd, rig
    rig.close()


def run_case(dev, op, dtype, steps, init, offs, what, G=1, run=1, defer=None, flag_init=None, done=False,
             timeout=TIMEOUT, words=None):
    """Model, then kernel, then every buffer and every control word compared.
    steps: model steps over named buffers; init: name -> bytes before the
    launch (the sources; a name that is only written is absent, must be written
    whole, and starts as the complement of what the model expects); offs: name
    -> byte offset past the 256-byte boundary.  words: the control words as an
    earlier launch of the same test left them (flags, done), else fresh ones.
    Returns the model's buffers and the words afterwards."""
    gloo_amd, rig = dev
    es = fm.itemsize(dtype)
    size = dict((k, v.size) for k, v in init.items())
    for s in steps:
        for name, off in ([s.dst] if s.dst else []) + list(s.xdst):
            assert name in init or off == 0
            size[name] = max(size.get(name, 0), (off + s.n) * es)
    bufs = {k: init[k].copy() if k in init else np.zeros(size[k], np.uint8) for k in size}
    flags, done_before = words if words else ({k: [0] * guard_rig.NW for k in guard_rig.FLAG_AT}, guard_rig.DONE_INIT)
    for k, v in (flag_init or {}).items():
        flags[k] = [v] * guard_rig.NW
    before = {k: list(v) for k, v in flags.items()}
    res = im.run_steps(op, dtype, steps, bufs, flags, run, G)
    ptr = {}
    for k in size:
        if k not in init:
            assert res.err or res.written[k].all(), (what, k, "is neither a source nor written whole")
        ptr[k] = rig.place(k, offs.get(k, 0), init[k] if k in init else ~bufs[k])
    rig.set_words(before, done=done_before)
    at = lambda ref: ptr[ref[0]] + ref[1] * es
    cs = [gloo_amd.interp_step(s.kind, dst=at(s.dst) if s.dst else 0, src=[at(r) for r in s.src], n=s.n, mode=s.mode,
                               flag=rig.flag_ptr(s.flag) if s.flag else 0, base=s.base, per_run=s.per_run,
                               xdst=[at(r) for r in s.xdst], defer=defer[i] if defer else 0)
          for i, s in enumerate(steps)]
    gloo_amd.interp_kernel(op, dtype, cs, rig.words + guard_rig.ERR, run=run, slices=G, timeout_ticks=timeout,
                           done=rig.words + guard_rig.DONE if done else 0,
                           done_ticket=rig.words + guard_rig.TICKET if done else 0)
    for k in size:
        rig.check(k, offs.get(k, 0), bufs[k] if k in init or not res.err else ~bufs[k], what, es)
    done_after = res.done if done and not res.err else done_before
    rig.check_words(flags, done_after, 0, res.err, what)
    return bufs, (flags, done_after)


def src_bytes(n, seed):
    return np.random.default_rng([7, n, seed]).integers(0, 256, n, dtype=np.uint8)


def names(prefix, k):
    return [f"{prefix}{i}" for i in range(k)]


# ---- COPY and SEND ---------------------------------------------------------

@pytest.mark.parametrize("kind", (COPY, SEND))
def test_copy_and_send_bytes(dev, kind):
    """One step, u8: every size at every offset case; a SEND's flag holds its value."""
    for n in im.copy_sizes(1):
        init = {"s0": src_bytes(n, 0)}
        for doff, soffs, _ in offset_cases(1, 1, 0):
            step = Step(kind, ("d", 0), (("s0", 0),), n, flag="f0" if kind == SEND else None, base=40, per_run=2)
            run_case(dev, "sum", "u8", [step], init, {"d": doff, "s0": soffs[0]}, ("kind", kind, "n", n, doff, soffs))


@pytest.mark.parametrize("kind", (COPY, SEND))
@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_copy_and_send_pass_boundary_in_elements(dev, dtype, kind):
    es = fm.itemsize(dtype)
    for n in im.copy_sizes(es):
        init = {"s0": src_bytes(n * es, 1)}
        for doff, soffs, _ in offset_cases(es, 1, 0):
            step = Step(kind, ("d", 0), (("s0", 0),), n, flag="f1" if kind == SEND else None, base=1 << 40, per_run=1)
            run_case(dev, "sum", dtype, [step], init, {"d": doff, "s0": soffs[0]}, (dtype, "kind", kind, "n", n, doff))


@pytest.mark.parametrize("nx", (1, 3, 8))
def test_copy_to_extra_destinations(dev, nx):
    """Every destination at its own offset."""
    for dtype in ("u8", "f32"):
        es = fm.itemsize(dtype)
        for n in im.copy_sizes(1) if es == 1 else im.copy_sizes(es)[-2:] + [1, 16 // es + 1]:
            init = {"s0": src_bytes(n * es, 2)}
            for doff, soffs, xoffs in offset_cases(es, 1, nx):
                offs = {"d": doff, "s0": soffs[0], **dict(zip(names("x", nx), xoffs))}
                assert doff == 0 and not any(xoffs) or any(x % 16 != doff % 16 for x in xoffs)
                step = Step(COPY, ("d", 0), (("s0", 0),), n, xdst=tuple((x, 0) for x in names("x", nx)))
                run_case(dev, "sum", dtype, [step], init, offs, (dtype, "nx", nx, "n", n, doff, xoffs))


# ---- FOLD ------------------------------------------------------------------

def fold_init(op, dtype, k, n, seed=0):
    return {f"s{i}": np.ascontiguousarray(s).view(np.uint8) for i, s in enumerate(im.fold_case(op, dtype, k, n, seed))}


def fold_step(k, n, mode, dst=("d", 0)):
    return Step(FOLD, dst, tuple((f"s{i}", 0) for i in range(k)), n, mode=mode)


@pytest.mark.parametrize("dtype,op", [(d, o) for d in fm.DTYPES for o in fm.ops_of(d)])
def test_fold_every_dtype_and_op(dev, dtype, op):
    """Modes 0, 1, 2 at k = 4, one pass and a bit, dst misaligned by one
    element.  A signed dtype's bitwise op runs the unsigned twin's kernel: the
    raw bytes are compared."""
    es = fm.itemsize(dtype)
    k, n = 4, im.fp_bytes(es) // es + 16 // es + 3
    O = offsets(es)
    offs = {"d": es, **{f"s{i}": O[(2 + i) % len(O)] for i in range(k)}}
    assert any(offs[f"s{i}"] % 16 != es % 16 for i in range(k))
    init = fold_init(op, dtype, k, n)
    for mode in (0, 1, 2):
        run_case(dev, op, dtype, [fold_step(k, n, mode)], init, offs, (dtype, op, "mode", mode))


SHAPE_CASES = [("u8", "sum"), ("bf16", "sum"), ("f32", "sum"), ("f64", "sum"), ("f32", "max")]


@pytest.mark.parametrize("k", (1, 2, 3, 5, 8))
@pytest.mark.parametrize("dtype,op", SHAPE_CASES)
def test_fold_shapes_and_misalignment(dev, dtype, op, k):
    es = fm.itemsize(dtype)
    for n in im.fold_sizes(es):
        init = fold_init(op, dtype, k, n)
        for doff, soffs, _ in offset_cases(es, k, 0):
            offs = {"d": doff, **{f"s{i}": soffs[i] for i in range(k)}}
            for mode in im.modes_of(k):
                run_case(dev, op, dtype, [fold_step(k, n, mode)], init, offs,
                         (dtype, op, "k", k, "n", n, "mode", mode, "offsets", doff, soffs))


@pytest.mark.parametrize("alias", ("first", "last"))
@pytest.mark.parametrize("dtype,op", [("u8", "sum"), ("f16", "sum"), ("f32", "max"), ("f64", "min"), ("u32", "bxor")])
def test_fold_in_place(dev, dtype, op, alias):
    """dst is src[0] (the executor folds into output 0) or src[k - 1]; the
    other sources sit at another residue.  Only the aliased source changes."""
    es = fm.itemsize(dtype)
    k = 4
    a = 0 if alias == "first" else k - 1
    O = offsets(es)
    for n in (16 // es + 1, im.fp_bytes(es) // es + 1, im.fold_sizes(es)[-1]):
        init = fold_init(op, dtype, k, n, seed=1)
        for c, doff in enumerate(O):
            offs = {f"s{i}": O[(c + 1 + i) % len(O)] for i in range(k)}
            offs[f"s{a}"] = doff
            for mode in (0, 1, 2):
                run_case(dev, op, dtype, [fold_step(k, n, mode, dst=(f"s{a}", 0))], init, offs,
                         (dtype, op, alias, "n", n, "mode", mode, "offsets", offs))


# ---- sliced ----------------------------------------------------------------

def sliced_steps(kind, n):
    if kind == COPY:
        return [Step(COPY, ("d", 0), (("s0", 0),), n, xdst=(("x0", 0), ("x1", 0)))]
    if kind == SEND:
        return [Step(SEND, ("d", 0), (("s0", 0),), n, flag="f0", base=1000, per_run=10)]
    return [fold_step(3, n, 1), Step(SIGNAL, flag="f1", base=7, per_run=1 << 33)]


@pytest.mark.parametrize("G", im.SLICE_COUNTS + (im.MANY_SLICES,))
@pytest.mark.parametrize("kind", (COPY, SEND, FOLD))
def test_sliced(dev, kind, G):
    """dst one element off 16 bytes: every slice that moves bytes has a head
    and, when it is whole packets long, a tail.  Slices without bytes publish
    their flag word all the same; the word after the G-th stays."""
    for dtype, op in (("f32", "max"),) if G == im.MANY_SLICES else (("u8", "sum"), ("bf16", "sum"), ("f32", "max"),
                                                                   ("f64", "sum")):
        es = fm.itemsize(dtype)
        O = offsets(es)
        for n in im.sliced_sizes(G, es):
            init = fold_init(op, dtype, 3, n, seed=2)
            if kind != FOLD:
                init = {"s0": init["s0"]}
            offs = {"d": es, "s0": O[2 % len(O)], "s1": 0, "s2": O[-1], "x0": O[-1], "x1": 0}
            _, (flags, _) = run_case(dev, op, dtype, sliced_steps(kind, n), init, offs, (dtype, "kind", kind, "G", G,
                                                                                         "n", n), G=G, run=3)
            if kind != COPY:
                f, v = ("f0", 1030) if kind == SEND else ("f1", 7 + 3 * (1 << 33))
                assert flags[f][:G] == [v] * G and flags[f][G] == 0  # (what check_words compared the device with)


# ---- sequence values, done -------------------------------------------------

@pytest.mark.parametrize("run", (1, 2, 1 << 32))
def test_sequence_values(dev, run):
    """base + run * per_run mod 2^64, a base near 2^64 that wraps, a wait met
    exactly, one whose counter is far above it and one whose counter has
    wrapped past it."""
    M = im.M64
    n = 100
    init = {"s0": src_bytes(n, 3)}
    steps = [Step(SIGNAL, flag="f0", base=M - 4, per_run=3),
             Step(WAIT, flag="f0", base=M - 4, per_run=3),         # met exactly by the step above
             Step(WAIT, flag="f1", base=10, per_run=1),            # the counter (set by the host) is far above
             Step(WAIT, flag="f1", base=M - 1000, per_run=1),      # the counter has wrapped past the target
             Step(COPY, ("d", 0), (("s0", 0),), n),
             Step(SEND, ("x0", 0), (("s0", 0),), n, flag="f1", base=1 << 63, per_run=(1 << 63) + 5)]
    for G in (1, 4):
        _, (flags, _) = run_case(dev, "sum", "u8", steps, init, {"d": 1, "x0": 15}, ("run", run, "G", G), G=G, run=run,
                                 flag_init={"f1": 1 << 33})
        assert flags["f0"][:G + 1] == [(M - 4 + 3 * run) & M] * G + [0]
        assert flags["f1"][:G + 1] == [((1 << 63) + run * ((1 << 63) + 5)) & M] * G + [1 << 33]
    assert (M - 4 + 3 * 2) & M == 1  # run 2 wraps


@pytest.mark.parametrize("G", (1, 2, 4))
def test_done_protocol(dev, G):
    """done == run and the ticket 0 after a launch; a second launch on the same
    words publishes its own run."""
    n = 3 * G * 4 + 1
    init = fold_init("sum", "f32", 2, n, seed=3)
    steps = [fold_step(2, n, 0), Step(SIGNAL, flag="f0", base=0, per_run=1)]
    offs = {"d": 4, "s0": 8, "s1": 0}
    _, words = run_case(dev, "sum", "f32", steps, init, offs, ("G", G, "first"), G=G, run=1, done=True)
    assert words[1] == 1
    _, words = run_case(dev, "sum", "f32", steps, init, offs, ("G", G, "second"), G=G, run=7, done=True, words=words)
    assert words[1] == 7
    _, words = run_case(dev, "sum", "f32", steps, init, offs, ("G", G, "no done"), G=G, run=9, words=words)
    assert words[1] == 7 and words[0]["f0"][:G + 1] == [9] * G + [0]


# ---- the loopback chain ----------------------------------------------------

def chain_defer(gloo_amd, steps, ptr, es):
    """The defer bits the executor would set (gloo_hip_interp_batches_ex) for
    this list at these addresses."""
    class Desc(ctypes.Structure):
        _fields_ = [("kind", ctypes.c_int32), ("nsrc", ctypes.c_int32), ("dst", ctypes.c_uint64),
                    ("src", ctypes.c_uint64 * 8), ("bytes", ctypes.c_uint64)]

    class DescEx(ctypes.Structure):
        _fields_ = [("step", Desc), ("nxdst", ctypes.c_int32), ("reserved", ctypes.c_int32),
                    ("xdst", ctypes.c_uint64 * 8)]
    arr = (DescEx * len(steps))()
    for d, s in zip(arr, steps):
        d.step.kind, d.step.nsrc, d.step.bytes = s.kind, len(s.src), s.n * es
        d.step.dst = ptr[s.dst[0]] + s.dst[1] * es if s.dst else 0
        for j, r in enumerate(s.src):
            d.step.src[j] = ptr[r[0]] + r[1] * es
        d.nxdst = len(s.xdst)
        for j, r in enumerate(s.xdst):
            d.xdst[j] = ptr[r[0]] + r[1] * es
    out = (ctypes.c_int * len(steps))()
    f = gloo_amd.lib.gloo_hip_interp_batches_ex
    f.argtypes = [ctypes.POINTER(DescEx), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    assert f(arr, len(steps), out) == 0
    return list(out)


@pytest.mark.parametrize("G", (1, 2, 4))
@pytest.mark.parametrize("dtype", ("f32", "bf16", "u8"))
def test_loopback_chain(dev, dtype, G):
    """COPY (2 extra destinations), FOLD in place, SIGNAL, SEND, WAIT on the
    SEND's flag, FOLD of the inbox, COPY (1 extra destination) in ONE launch,
    runs 1, 2, 3 on the same flags: each run's wait needs that run's send.
    With the executor's defer bits and with none the bytes are the model's.  At
    G > 1 every step has the same n from element 0 (slice g reads only what
    workgroup g wrote); one workgroup also sends a sub-range."""
    gloo_amd, rig = dev
    es = fm.itemsize(dtype)
    kV = 16 // es
    n = 3 * G * kV + 1 + (im.fp_bytes(es) // es if G == 1 else 0)
    O = offsets(es)
    offs = {name: O[i % len(O)] for i, name in enumerate(im.CHAIN_BUFFERS)}
    offs["work"] = es
    init = im.chain_inputs("sum", dtype, n)
    for sub in (None, (kV, n - 2 * kV - 1)) if G == 1 else (None,):
        steps = im.chain(n, sub)
        ptr = {name: rig.raw(name) + guard_rig.GUARD + offs[name] for name in im.CHAIN_BUFFERS}
        defer = chain_defer(gloo_amd, steps, ptr, es)
        assert sum(defer) >= 1 and defer[-1] == 0, defer
        results = []
        for bits in (defer, None):
            words = None
            for run in (1, 2, 3):
                bufs, words = run_case(dev, "sum", dtype, steps, init, offs, (dtype, "G", G, "sub", sub, "run", run,
                                                                              "defer", bits), G=G, run=run, defer=bits,
                                       words=words, done=True)
                assert words[0]["f0"][:G] == [5 + 3 * run] * G and words[0]["f1"][:G] == [100 + 7 * run] * G
            results.append(bufs)
        assert all((results[0][k] == results[1][k]).all() for k in results[0])


@pytest.mark.parametrize("G", (1, 3))
def test_every_flag_of_a_batch_is_published(dev, G):
    """Two waits the host has met, then SEND, SIGNAL, SEND and a COPY that are
    independent of each other: one batch each under the executor's rule.  Every
    flag of the batch holds its value afterwards, not only the last step's."""
    gloo_amd, rig = dev
    n = 3 * G * 16 + 1
    init = {f"s{i}": src_bytes(n, 10 + i) for i in range(3)}
    steps = [Step(WAIT, flag="f0", base=3, per_run=1), Step(WAIT, flag="f1", base=2, per_run=2),
             Step(SEND, ("d", 0), (("s0", 0),), n, flag="f0", base=20, per_run=1),
             Step(SIGNAL, flag="f1", base=30, per_run=1),
             Step(SEND, ("x0", 0), (("s1", 0),), n, flag="f0", base=40, per_run=1),
             Step(COPY, ("x1", 0), (("s2", 0),), n, xdst=(("x2", 0),))]
    offs = {"d": 1, "x0": 15, "x1": 8, "x2": 1, "s0": 0, "s1": 8, "s2": 15}
    ptr = {name: rig.raw(name) + guard_rig.GUARD + offs[name] for name in offs}
    defer = chain_defer(gloo_amd, steps, ptr, 1)
    assert defer == [1, 0, 1, 1, 1, 0]
    for bits in (defer, None):
        _, (flags, _) = run_case(dev, "sum", "u8", steps, init, offs, ("G", G, "defer", bits), G=G, run=2, defer=bits,
                                 flag_init={"f0": 5, "f1": 6})
        assert flags["f0"][:G + 1] == [42] * G + [5] and flags["f1"][:G + 1] == [32] * G + [6]


# ---- the one wait nobody meets ---------------------------------------------

def test_unmet_wait_times_out_and_stops_the_list(dev):
    """The designed behaviour (test_dead_peer_times_out has it end to end): 2 ms
    after the launch err is 1, the COPY and the SIGNAL behind the wait have not
    run, done is not written, and the launch returns normally."""
    n = 1000
    init = {"s0": src_bytes(n, 4), "d": src_bytes(n, 5)}
    steps = [Step(WAIT, flag="f0", base=1, per_run=0), Step(COPY, ("d", 0), (("s0", 0),), n),
             Step(SIGNAL, flag="f1", base=77, per_run=0)]
    assert im.run_steps("sum", "u8", steps, {k: v.copy() for k, v in init.items()}, {"f0": [0], "f1": [0]}, 1).err == 1
    _, (flags, done) = run_case(dev, "sum", "u8", steps, init, {"d": 3, "s0": 0}, "unmet wait", done=True,
                                timeout=2 * 10 ** 5)
    assert done == guard_rig.DONE_INIT and flags["f1"][0] == 0
