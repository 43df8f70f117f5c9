"""The public surface of gloo_hip_fold_kernel, without a GPU: the declaration
in include/gloo_amd.h, the Python names, and every refusal, each of which
comes before any HIP call (dummy non-null addresses stand for the buffers)."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gloo_amd.h")).read()

DST, SRC, FWD, FLAG, TICKET = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
OP, DTYPE, PTR, ARG = -1, -2, -3, -4

# never called: a registered custom op's function (kept alive with the module)
CUSTOM_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_size_t, ctypes.c_void_p)(lambda *a: None)


def test_header_declares_it():
    assert ("int gloo_hip_fold_kernel(int op, int dtype, void* dst, const void* const* srcs, int k, size_t n, int mode,\n"
            "                         void* const* fwd, uint64_t* const* fwd_flags, const uint64_t* fwd_values, int nfwd,\n"
            "                         unsigned* ticket, gloo_hip_stream_t stream);") in HEADER
    assert "#define GLOO_HIP_MAX_SRCS 8" in HEADER


def test_python_names():
    import gloo_amd
    assert "gloo_hip_fold_kernel" in gloo_amd.EXPORTED and hasattr(gloo_amd.lib, "gloo_hip_fold_kernel")
    sig = inspect.signature(gloo_amd.fold_kernel)
    assert list(sig.parameters) == ["op", "dtype", "dst", "srcs", "n", "mode", "fwd", "fwd_flags", "fwd_values",
                                    "ticket", "stream"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"mode": 0, "fwd": (), "fwd_flags": None, "fwd_values": None, "ticket": 0, "stream": 0}
    vp = ctypes.c_void_p
    assert gloo_amd.lib.gloo_hip_fold_kernel.argtypes == [
        ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(vp), ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
        ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, vp, vp]


def refused(code, word, *args, **kw):
    import gloo_amd
    with pytest.raises(gloo_amd.GlooHipError) as e:
        gloo_amd.fold_kernel(*args, **kw)
    assert e.value.code == code, str(e.value)
    assert word in str(e.value), str(e.value)


def test_counts_and_modes():
    refused(ARG, "source count", "sum", "f32", DST, [], 4)
    refused(ARG, "source count", "sum", "f32", DST, [SRC] * 9, 4)
    refused(ARG, "forward count", "sum", "f32", DST, [SRC], 4, fwd=[FWD] * 9)
    refused(ARG, "fold mode", "sum", "f32", DST, [SRC] * 2, 4, mode=3)
    refused(ARG, "fold mode", "sum", "f32", DST, [SRC] * 2, 4, mode=-1)
    for k in (3, 5, 6, 7):
        refused(ARG, "power-of-two", "sum", "f32", DST, [SRC] * k, 4, mode=2)
        refused(ARG, "power-of-two", "sum", "f32", DST, [SRC] * k, 4, mode=2, fwd=[FWD])


def test_negative_forward_count_through_the_c_abi():
    import gloo_amd
    srcs = (ctypes.c_void_p * 1)(SRC)
    assert gloo_amd.lib.gloo_hip_fold_kernel(1, 8, DST, srcs, 1, 4, 0, None, None, None, -1, None, None) == ARG
    assert b"forward count" in gloo_amd.lib.gloo_hip_last_error()


def test_dtype_and_op():
    import gloo_amd
    refused(DTYPE, "dtype", "sum", 12, DST, [SRC], 4)
    refused(DTYPE, "dtype", "sum", -1, DST, [SRC], 4, fwd=[FWD])
    refused(OP, "op", 0, "f32", DST, [SRC], 4)
    refused(OP, "op", 8, "i32", DST, [SRC], 4, fwd=[FWD])
    for op in ("band", "bor", "bxor"):
        for dtype in ("f16", "bf16", "f32", "f64", "f8e4m3", "f8e5m2"):
            for fwd in ((), (FWD,)):
                refused(OP, f"reduction op {op} is not defined for dtype {dtype}", op, dtype, DST, [SRC], 4, fwd=fwd)
    custom = gloo_amd.register_op(ctypes.cast(CUSTOM_FN, ctypes.c_void_p).value)
    assert custom >= 1000
    for fwd in ((), (FWD,)):
        refused(OP, "built-in", custom, "f32", DST, [SRC] * 2, 4, fwd=fwd)
        refused(OP, "built-in", 1000 + 12345, "f32", DST, [SRC] * 2, 4, fwd=fwd)  # not registered


def test_pointers():
    for fwd in ((), (FWD,)):
        refused(PTR, "null dst", "sum", "f32", 0, [SRC], 4, fwd=fwd)
        refused(PTR, "dst not aligned", "sum", "f32", DST + 2, [SRC], 4, fwd=fwd)
        refused(PTR, "dst not aligned", "sum", "f64", DST + 4, [SRC], 4, fwd=fwd)
        refused(PTR, "null source", "sum", "f32", DST, [SRC, 0], 4, fwd=fwd)
        refused(PTR, "source not aligned", "sum", "bf16", DST, [SRC, SRC + 1], 4, fwd=fwd)
    refused(PTR, "forward destination not aligned", "sum", "f32", DST, [SRC], 4, fwd=[FWD, FWD + 2])


def test_forwards_flags_and_ticket():
    refused(ARG, "neither data nor flag", "sum", "f32", DST, [SRC], 4, fwd=[FWD, 0])
    refused(ARG, "neither data nor flag", "sum", "f32", DST, [SRC], 4, fwd=[0], fwd_flags=[0], ticket=TICKET)
    refused(ARG, "without a ticket", "sum", "f32", DST, [SRC], 4, fwd=[FWD], fwd_flags=[FLAG], fwd_values=[1])
    refused(ARG, "without a ticket", "sum", "f32", DST, [SRC], 4, fwd=[FWD, 0], fwd_flags=[0, FLAG])


def test_every_check_comes_before_the_empty_fold():
    """n == 0 is a no-op, but only for arguments that a launch would accept."""
    import gloo_amd
    for mode, k in ((0, 1), (0, 8), (1, 3), (2, 4)):
        gloo_amd.fold_kernel("sum", "f32", DST, [SRC] * k, 0, mode=mode)
        gloo_amd.fold_kernel("max", "f8e5m2", DST + 1, [SRC + 3] * k, 0, mode=mode, fwd=[FWD + 5, 0],
                             fwd_flags=[FLAG, FLAG + 8], fwd_values=[3, 4], ticket=TICKET)
    gloo_amd.fold_kernel("bxor", "i64", DST, [SRC], 0, fwd=[FWD] * 8)
    refused(ARG, "source count", "sum", "f32", DST, [], 0)
    refused(ARG, "power-of-two", "sum", "f32", DST, [SRC] * 3, 0, mode=2)
    refused(DTYPE, "dtype", "sum", 99, DST, [SRC], 0)
    refused(OP, "not defined for dtype", "band", "f32", DST, [SRC], 0)
    refused(PTR, "null dst", "sum", "f32", 0, [SRC], 0)
    refused(PTR, "null source", "sum", "f32", DST, [0], 0)
    refused(ARG, "neither data nor flag", "sum", "f32", DST, [SRC], 0, fwd=[0])
    refused(ARG, "without a ticket", "sum", "f32", DST, [SRC], 0, fwd=[FWD], fwd_flags=[FLAG])
