"""The public surface of gloo_hip_interp_kernel and gloo_hip_fused_step, without
a GPU: the declarations in include/gloo_amd.h, the step struct against its
ctypes mirror, the Python names, and every refusal, each of which comes before
any HIP call (dummy non-null addresses stand for the buffers)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gloo_amd.h")).read()

DST, SRC, XD, FLAG, ERR, DONE, TICKET, EPOCH = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x50100, 0x50200, 0x50300
OP, DTYPE, PTR, ARG = -1, -2, -3, -4
COPY, SEND, SIGNAL, WAIT, FOLD = range(5)

CUSTOM_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_size_t, ctypes.c_void_p)(lambda *a: None)


def test_header_declares_them():
    assert ("int gloo_hip_interp_kernel(int op, int dtype, const gloo_hip_interp_step_t* steps, int nsteps, uint64_t run,\n"
            "                           int slices, uint64_t timeout_ticks, uint32_t* err, uint64_t* done, unsigned* done_ticket,\n"
            "                           gloo_hip_stream_t stream);") in HEADER
    assert ("int gloo_hip_fused_step(int op, int dtype, void* dst, const void* src, size_t n, const uint64_t* wait_flag,\n"
            "                        uint64_t wait_base, uint64_t wait_per_run, uint64_t timeout_ticks, uint32_t* err,\n"
            "                        uint64_t* sig_flag, uint64_t sig_base, uint64_t sig_per_run, const uint64_t* epoch,\n"
            "                        gloo_hip_stream_t stream);") in HEADER
    assert "synchronous test entry" in " ".join(HEADER.split())
    assert "#define GLOO_HIP_MAX_SRCS 8" in HEADER and "#define GLOO_HIP_MAX_XDSTS 8" in HEADER


def test_step_struct_matches_the_header():
    """Field order and types from the header's typedef; offsets by the C rules
    (natural alignment) against the ctypes mirror."""
    import gloo_amd
    body = re.search(r"typedef struct \{([^}]*)\} gloo_hip_interp_step_t;", HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size_of = {"int32_t": 4, "uint64_t": 8, "uint64_t*": 8, "void*": 8, "const void*": 8}
    want, at = [], 0
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        ctype, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
        for name in [x.strip() for x in names.split(",")]:
            count = 1
            m = re.match(r"(\w+)\[(\w+)\]", name)
            if m:
                name, count = m.group(1), {"GLOO_HIP_MAX_SRCS": 8, "GLOO_HIP_MAX_XDSTS": 8}[m.group(2)]
            sz = size_of[ctype]
            at = (at + sz - 1) // sz * sz
            want.append((name, at, sz * count))
            at += sz * count
    S = gloo_amd.InterpStep
    got = [(name, getattr(S, name).offset, getattr(S, name).size) for name, _ in S._fields_]
    assert got == want
    assert [n for n, _, _ in got] == ["kind", "mode", "nsrc", "defer", "flag", "base", "per_run", "dst", "src", "n",
                                      "nxdst", "reserved", "xdst"]
    assert ctypes.sizeof(S) == (at + 7) // 8 * 8 == 192
    assert (gloo_amd.INTERP_COPY, gloo_amd.INTERP_SEND, gloo_amd.INTERP_SIGNAL, gloo_amd.INTERP_WAIT,
            gloo_amd.INTERP_FOLD) == (0, 1, 2, 3, 4)
    # the numbering of gloo_hip_interp_desc_t
    assert "(0 copy, 1 send, 2 signal,\n * 3 wait, 4 fold)" in HEADER
    assert "/* 0 copy, 1 send, 2 signal, 3 wait, 4 fold (as gloo_hip_interp_desc_t) */" in HEADER


def test_python_names():
    import gloo_amd
    for name in ("gloo_hip_interp_kernel", "gloo_hip_fused_step"):
        assert name in gloo_amd.EXPORTED and hasattr(gloo_amd.lib, name)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert gloo_amd.lib.gloo_hip_interp_kernel.argtypes == [
        ctypes.c_int, ctypes.c_int, ctypes.POINTER(gloo_amd.InterpStep), ctypes.c_int, u64, ctypes.c_int, u64, vp, vp,
        vp, vp]
    assert gloo_amd.lib.gloo_hip_fused_step.argtypes == [
        ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_size_t, vp, u64, u64, u64, vp, vp, u64, u64, vp, vp]
    assert list(inspect.signature(gloo_amd.interp_kernel).parameters) == [
        "op", "dtype", "steps", "err", "run", "slices", "timeout_ticks", "done", "done_ticket", "stream"]
    assert list(inspect.signature(gloo_amd.fused_step).parameters) == [
        "op", "dtype", "dst", "src", "n", "err", "wait_flag", "wait_base", "wait_per_run", "sig_flag", "sig_base",
        "sig_per_run", "epoch", "timeout_ticks", "stream"]


def step(kind, **kw):
    import gloo_amd
    return gloo_amd.interp_step(kind, **kw)


def copy(**kw):
    return step(COPY, **{**dict(dst=DST, src=[SRC], n=4), **kw})


def refused(code, word, steps, op="sum", dtype="f32", err=ERR, **kw):
    import gloo_amd
    with pytest.raises(gloo_amd.GlooHipError) as e:
        gloo_amd.interp_kernel(op, dtype, steps, err, **kw)
    assert e.value.code == code, str(e.value)
    assert word in str(e.value), str(e.value)


def test_interp_launch_arguments():
    import gloo_amd
    L = gloo_amd.lib
    assert L.gloo_hip_interp_kernel(1, 8, None, 1, 1, 1, 1000, ERR, None, None, None) == PTR
    assert b"null step list" in L.gloo_hip_last_error()
    assert L.gloo_hip_interp_kernel(1, 8, None, -1, 1, 1, 1000, ERR, None, None, None) == ARG
    assert b"step count -1" in L.gloo_hip_last_error()
    refused(ARG, "step count 513", [copy()] * 513)
    for g in (0, -1, 257):
        refused(ARG, f"slice count {g}", [copy()], slices=g)
    refused(PTR, "null err", [copy()], err=0)
    refused(ARG, "half a done", [copy()], done=DONE)
    refused(ARG, "half a done", [copy()], done_ticket=TICKET)
    refused(ARG, "timeout_ticks 0", [copy()], timeout_ticks=0)
    refused(ARG, f"timeout_ticks {10 ** 9 + 1}", [copy()], timeout_ticks=10 ** 9 + 1)
    refused(ARG, f"timeout_ticks {2 ** 64 - 1}", [copy()], timeout_ticks=2 ** 64 - 1)


def test_interp_dtype_and_op():
    import gloo_amd
    refused(DTYPE, "dtype", [copy()], dtype=12)
    refused(DTYPE, "dtype", [copy()], dtype=-1)
    refused(OP, "op", [copy()], op=0)
    refused(OP, "op", [copy()], op=8, dtype="i32")
    for op in ("band", "bor", "bxor"):
        for dtype in ("f16", "bf16", "f32", "f64", "f8e4m3", "f8e5m2"):
            refused(OP, f"reduction op {op} is not defined for dtype {dtype}", [copy()], op=op, dtype=dtype)
    custom = gloo_amd.register_op(ctypes.cast(CUSTOM_FN, ctypes.c_void_p).value)
    refused(OP, "built-in", [copy()], op=custom)
    refused(OP, "built-in", [copy()], op=1000 + 12345)


def test_interp_kinds_modes_and_counts():
    refused(ARG, "step 0: unknown kind 5", [step(5, dst=DST, src=[SRC], n=4)])
    refused(ARG, "step 1: unknown kind -1", [copy(), step(-1, dst=DST, src=[SRC], n=4)])
    for mode in (-1, 3):
        refused(ARG, f"step 0: unknown fold mode {mode}", [step(FOLD, dst=DST, src=[SRC] * 2, n=4, mode=mode)])
    for k in (3, 5, 6, 7):
        refused(ARG, f"power-of-two count, not {k}", [step(FOLD, dst=DST, src=[SRC] * k, n=4, mode=2)])
    refused(ARG, "source count 0", [step(FOLD, dst=DST, src=[], n=4)])
    refused(ARG, "source count 9", [step(FOLD, dst=DST, src=[SRC] * 8, n=4, nsrc=9)])
    refused(ARG, "source count -1", [step(FOLD, dst=DST, src=[SRC], n=4, nsrc=-1)])
    refused(ARG, "extra destination count 9", [copy(xdst=[XD] * 8, nxdst=9)])
    refused(ARG, "extra destination count -1", [copy(nxdst=-1)])
    refused(ARG, "no COPY", [step(SEND, dst=DST, src=[SRC], n=4, flag=FLAG, xdst=[XD])])
    refused(ARG, "no COPY", [step(FOLD, dst=DST, src=[SRC], n=4, xdst=[XD])])
    refused(ARG, "no COPY", [step(SIGNAL, flag=FLAG, xdst=[XD])])


def test_interp_flags_and_defer():
    for kind in (SEND, SIGNAL, WAIT):
        refused(PTR, "step 1: null flag", [copy(), step(kind, dst=DST, src=[SRC], n=4)])
    refused(ARG, "step 0: defer bit on the last step", [copy(defer=1)])
    refused(ARG, "step 1: defer bit on the last step", [copy(defer=1), step(SIGNAL, flag=FLAG, defer=1)])
    refused(ARG, "defer bit 2", [copy(defer=2), copy()])
    refused(ARG, "joins a wait", [step(WAIT, flag=FLAG, defer=1), copy()])
    refused(ARG, "joins a wait", [copy(defer=1), step(WAIT, flag=FLAG)])


def test_interp_pointers_and_overlap():
    for kind, kw in ((COPY, {}), (SEND, dict(flag=FLAG)), (FOLD, {})):
        refused(PTR, "step 0: null dst", [step(kind, dst=0, src=[SRC], n=4, **kw)])
        refused(PTR, "dst not aligned", [step(kind, dst=DST + 2, src=[SRC], n=4, **kw)])
        refused(PTR, "null source pointer 0", [step(kind, dst=DST, src=[0], n=4, **kw)])
        refused(PTR, "source 0 not aligned", [step(kind, dst=DST, src=[SRC + 1], n=4, **kw)])
    refused(PTR, "dst not aligned", [copy(dst=DST + 4)], dtype="f64")
    refused(PTR, "null source pointer 2", [step(FOLD, dst=DST, src=[SRC, SRC, 0], n=4)])
    refused(PTR, "source 1 not aligned", [step(FOLD, dst=DST, src=[SRC, SRC + 1], n=4)], dtype="bf16")
    refused(PTR, "null extra destination 1", [copy(xdst=[XD, 0])])
    refused(PTR, "extra destination 2 not aligned", [copy(xdst=[XD, XD, XD + 3])])
    for kind, kw in ((COPY, {}), (SEND, dict(flag=FLAG))):
        refused(ARG, "source overlaps dst", [step(kind, dst=DST, src=[DST], n=4, **kw)])
        refused(ARG, "source overlaps dst", [step(kind, dst=DST, src=[DST + 12], n=4, **kw)])
        refused(ARG, "source overlaps dst", [step(kind, dst=DST + 12, src=[DST], n=4, **kw)])
    refused(ARG, "source overlaps extra destination 1", [copy(xdst=[XD, SRC + 8])])
    import gloo_amd
    # adjacent is not overlapping; a fold may run in place; n == 0 looks at no pointer
    gloo_amd.interp_kernel("sum", "f32", [], ERR)
    gloo_amd.interp_kernel("sum", "f32", [], ERR, slices=256, done=DONE, done_ticket=TICKET, timeout_ticks=10 ** 9)
    assert gloo_amd.lib.gloo_hip_interp_kernel(1, 8, None, 0, 1, 1, 1000, ERR, None, None, None) == 0


def test_every_interp_check_comes_before_the_empty_list():
    import gloo_amd
    L = gloo_amd.lib
    for args, code in (((1, 8, None, 0, 1, 0, 1000, ERR, None, None, None), ARG),
                       ((1, 8, None, 0, 1, 1, 0, ERR, None, None, None), ARG),
                       ((1, 8, None, 0, 1, 1, 1000, None, None, None, None), PTR),
                       ((1, 8, None, 0, 1, 1, 1000, ERR, DONE, None, None), ARG),
                       ((1, 12, None, 0, 1, 1, 1000, ERR, None, None, None), DTYPE),
                       ((5, 8, None, 0, 1, 1, 1000, ERR, None, None, None), OP),
                       ((0, 8, None, 0, 1, 1, 1000, ERR, None, None, None), OP)):
        assert L.gloo_hip_interp_kernel(*args) == code, args


def fused_refused(code, word, *args, **kw):
    import gloo_amd
    with pytest.raises(gloo_amd.GlooHipError) as e:
        gloo_amd.fused_step(*args, **kw)
    assert e.value.code == code, str(e.value)
    assert word in str(e.value), str(e.value)


def test_fused_step_refusals():
    import gloo_amd
    fused_refused(DTYPE, "dtype", "sum", 12, DST, SRC, 4, ERR)
    fused_refused(DTYPE, "dtype", 0, -1, DST, SRC, 4, ERR)
    fused_refused(OP, "op", 8, "i32", DST, SRC, 4, ERR)
    fused_refused(OP, "op", -1, "f32", DST, SRC, 4, ERR)
    for op in ("band", "bor", "bxor"):
        for dtype in ("f16", "bf16", "f32", "f64", "f8e4m3", "f8e5m2"):
            fused_refused(OP, f"reduction op {op} is not defined for dtype {dtype}", op, dtype, DST, SRC, 4, ERR)
    custom = gloo_amd.register_op(ctypes.cast(CUSTOM_FN, ctypes.c_void_p).value)
    fused_refused(OP, "built-in", custom, "f32", DST, SRC, 4, ERR)
    fused_refused(PTR, "null err", "sum", "f32", DST, SRC, 4, 0)
    fused_refused(ARG, "timeout_ticks 0", "sum", "f32", DST, SRC, 4, ERR, timeout_ticks=0)
    fused_refused(ARG, f"timeout_ticks {10 ** 9 + 1}", 0, "u8", DST, SRC, 4, ERR, wait_flag=FLAG,
                  timeout_ticks=10 ** 9 + 1)
    for op in ("sum", 0):
        fused_refused(PTR, "null dst", op, "f32", 0, SRC, 4, ERR)
        fused_refused(PTR, "dst not aligned", op, "f32", DST + 2, SRC, 4, ERR)
        fused_refused(PTR, "dst not aligned", op, "f64", DST + 4, SRC, 4, ERR)
        fused_refused(PTR, "null source", op, "f32", DST, 0, 4, ERR)
        fused_refused(PTR, "source not aligned", op, "bf16", DST, SRC + 1, 4, ERR)
        fused_refused(ARG, "source overlaps dst", op, "f32", DST, DST, 4, ERR)
        fused_refused(ARG, "source overlaps dst", op, "f32", DST, DST + 12, 4, ERR)
    # n == 0 with no flag launches nothing, but only for arguments a launch would accept
    gloo_amd.fused_step("sum", "f32", 0, 0, 0, ERR)
    gloo_amd.fused_step(0, "f8e5m2", DST + 1, SRC + 3, 0, ERR, epoch=EPOCH, timeout_ticks=10 ** 9)
    fused_refused(DTYPE, "dtype", "sum", 99, 0, 0, 0, ERR)
    fused_refused(OP, "not defined for dtype", "band", "f32", 0, 0, 0, ERR)
    fused_refused(PTR, "null err", "sum", "f32", 0, 0, 0, 0)
    fused_refused(ARG, "timeout_ticks 0", "sum", "f32", 0, 0, 0, ERR, timeout_ticks=0)
