"""CPU: the FP8 dtypes F8E4M3 (OCP e4m3fn) and F8E5M2 (OCP e5m2) at the C-ABI
boundary — the codes in the Python binding and in include/gloo_amd.h, the
element size, the op x dtype rule (SUM..MIN yes, BAND / BOR / BXOR
GLOO_HIP_EINVAL_OP), the plans (element size 1, as i8), the torch dtype map and
the C++ tags — and the facts of the model (tests/fp8_model.py: torch on the
CPU) that the GPU tests hold the kernels to, pinned here so that the helper
cannot drift.  Nothing here touches the GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fp8_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = {"f8e4m3": 10, "f8e5m2": 11}


def test_codes_python_and_header():
    import gloo_amd
    assert int(gloo_amd.DType.F8E4M3) == 10 and int(gloo_amd.DType.F8E5M2) == 11
    assert int(gloo_amd.DTYPE_NAMES["f8e4m3"]) == 10 and int(gloo_amd.DTYPE_NAMES["f8e5m2"]) == 11
    text = open(os.path.join(ROOT, "include", "gloo_amd.h")).read()
    enum = re.search(r"typedef enum \{([^}]*)\}\s*gloo_hip_dtype_t;", text).group(1)
    values = {k: int(v) for k, v in re.findall(r"GLOO_HIP_(\w+)\s*=\s*(\d+)", enum)}
    assert values["F8E4M3"] == 10 and values["F8E5M2"] == 11 and values["NUM_DTYPES"] == 12
    assert sorted(values.values()) == list(range(13))


def test_dtype_size_is_one_byte():
    import gloo_amd
    for name, code in FP8.items():
        assert gloo_amd.dtype_size(name) == 1
        assert gloo_amd.lib.gloo_hip_dtype_size(code) == 1


def test_dtype_12_is_invalid():
    import gloo_amd
    L = gloo_amd.lib
    assert L.gloo_hip_dtype_size(12) == 0
    assert L.gloo_hip_reduce(1, 12, None, None, 0, None) == -2
    assert L.gloo_hip_reduce_multi(1, 12, None, (ctypes.c_void_p * 1)(None), 1, 0, None) == -2


def test_op_supported():
    import gloo_amd
    S = gloo_amd.lib.gloo_hip_op_supported
    for dt in FP8.values():
        for op in (1, 2, 3, 4):
            assert S(op, dt) == 1, (op, dt)
        for op in (5, 6, 7, 0, 8, 999):
            assert S(op, dt) == 0, (op, dt)
    assert gloo_amd.op_supported("sum", "f8e4m3") is True
    assert gloo_amd.op_supported("min", "f8e5m2") is True
    assert gloo_amd.op_supported("bxor", "f8e5m2") is False


def test_arithmetic_ops_accepted_without_a_gpu():
    import gloo_amd
    L = gloo_amd.lib
    for dt in FP8.values():
        for op in (1, 2, 3, 4):
            assert L.gloo_hip_reduce(op, dt, None, None, 0, None) == 0, (op, dt)
            # a valid op x dtype: the null pointers are the error
            assert L.gloo_hip_reduce(op, dt, None, None, 5, None) == -3, (op, dt)


def test_bxor_on_f8e4m3_is_einval_op():
    """n = 0 and NULL pointers: refused before either is looked at, and the
    message names op and dtype."""
    import gloo_amd
    L = gloo_amd.lib
    arr = (ctypes.c_void_p * 1)(None)
    calls = {
        "reduce": lambda: L.gloo_hip_reduce(7, 10, None, None, 0, None),
        "reduce3": lambda: L.gloo_hip_reduce3(7, 10, None, None, None, 0, None),
        "reduce_multi": lambda: L.gloo_hip_reduce_multi(7, 10, None, arr, 1, 0, None),
        "reduce_staged": lambda: L.gloo_hip_reduce_staged(7, 10, None, None, 0, None, None, 0, None),
    }
    for what, call in calls.items():
        L.gloo_hip_reduce(1, 8, None, None, 0, None)  # a success in between: the message below is this call's
        assert call() == -1, what
        msg = L.gloo_hip_last_error().decode()
        assert "bxor" in msg and "f8e4m3" in msg, (what, msg)
    for op in (5, 6):
        assert L.gloo_hip_reduce(op, 11, None, None, 0, None) == -1
        assert "f8e5m2" in L.gloo_hip_last_error().decode()


@pytest.mark.parametrize("algo,P,n", [("halving_doubling", 5, 10_007), ("ring_chunked", 4, 10_007)])
def test_plans_are_the_i8_plans(algo, P, n):
    import gloo_amd
    from plan_sim import Step, get_plan
    fields = [f for f, _ in Step._fields_]
    for r in range(P):
        for name in FP8:
            got, arena = get_plan(algo, r, P, n, elem_size=gloo_amd.dtype_size(name))
            want, arena_i8 = get_plan(algo, r, P, n, elem_size=gloo_amd.dtype_size("i8"))
            assert arena == arena_i8 and len(got) == len(want) and len(got) > 0
            for i, (g, w) in enumerate(zip(got, want)):
                assert [getattr(g, f) for f in fields] == [getattr(w, f) for f in fields], (r, i)


def test_torch_dtype_map():
    torch = pytest.importorskip("torch")
    import gloo_amd
    assert gloo_amd._torch_dtype_code(torch.empty(1, dtype=torch.float8_e4m3fn)) == gloo_amd.DType.F8E4M3
    assert gloo_amd._torch_dtype_code(torch.empty(1, dtype=torch.float8_e5m2)) == gloo_amd.DType.F8E5M2


# ---- the model's facts -----------------------------------------------------

NAN_COUNTS = {("f8e4m3", "sum"): (1456, 436), ("f8e4m3", "product"): (11140, 10120),
              ("f8e5m2", "sum"): (3038, 2), ("f8e5m2", "product"): (3044, 8)}


@pytest.mark.parametrize("dtype,op", sorted(NAN_COUNTS))
def test_model_nan_counts(dtype, op):
    """Over all 65,536 operand pairs: how many results are NaN, and how many of
    those come from two non-NaN operands (e4m3fn: finite operands overflowing;
    e5m2: inf - inf, 0 * inf)."""
    pytest.importorskip("torch")
    a, b = fp8_model.table()
    c = fp8_model.fp8_op(op, dtype, a, b)
    nan = fp8_model.is_nan(dtype, c)
    special = nan & ~fp8_model.is_nan(dtype, a) & ~fp8_model.is_nan(dtype, b)
    assert (int(nan.sum()), int(special.sum())) == NAN_COUNTS[(dtype, op)]
    fa, fb = fp8_model.widen(dtype, a), fp8_model.widen(dtype, b)
    with np.errstate(all="ignore"):
        r = fa + fb if op == "sum" else fa * fb
    # the project's rule: an f32 NaN is 0x7F whatever the operands' signs
    assert (c[np.isnan(r)] == 0x7F).all()
    if dtype == "f8e4m3":
        # finite operands overflowing keep the result's sign
        over = special & ~np.isnan(r)
        assert over.sum() == special.sum()
        assert (c[over] == np.where(r[over] < 0, 0xFF, 0x7F)).all()
        assert (np.abs(r[over]) > 464).all() and (np.abs(r[~nan]) <= 464).all()
    else:
        assert np.isnan(r[special]).all()
        inf = (c & 0x7F) == 0x7C
        with np.errstate(all="ignore"):
            assert (np.abs(r[inf]) >= 61440).all() and (np.abs(r[~inf & ~nan]) < 61440).all()
        assert (c[inf] == np.where(r[inf] < 0, 0xFC, 0x7C)).all()


def test_model_threshold_bytes():
    torch = pytest.importorskip("torch")
    x = torch.tensor([464.0, 465.0, -464.0, -465.0, 448.0])
    assert x.to(torch.float8_e4m3fn).view(torch.uint8).tolist() == [0x7E, 0x7F, 0xFE, 0xFF, 0x7E]
    y = torch.tensor([61440.0, -61440.0, 61439.0, 57344.0])
    assert y.to(torch.float8_e5m2).view(torch.uint8).tolist() == [0x7C, 0xFC, 0x7B, 0x7B]


def test_model_max_min_copy_raw_bytes():
    pytest.importorskip("torch")
    for dtype in FP8:
        a, b = fp8_model.table()
        fa, fb = fp8_model.widen(dtype, a), fp8_model.widen(dtype, b)
        with np.errstate(all="ignore"):
            assert (fp8_model.fp8_op("max", dtype, a, b) == np.where(fa < fb, b, a)).all()
            assert (fp8_model.fp8_op("min", dtype, a, b) == np.where(fb < fa, b, a)).all()
        # a NaN in a stays, a NaN in b is ignored, max(+0, -0) is +0
        nan = np.uint8(0x7F)
        one = np.uint8(0x38 if dtype == "f8e4m3" else 0x3C)
        assert fp8_model.widen(dtype, np.array([one]))[0] == 1.0
        for op in ("max", "min"):
            assert fp8_model.fp8_op(op, dtype, np.array([nan]), np.array([one]))[0] == nan
            assert fp8_model.fp8_op(op, dtype, np.array([one]), np.array([nan]))[0] == one
        assert fp8_model.fp8_op("max", dtype, np.array([0x00], np.uint8), np.array([0x80], np.uint8))[0] == 0x00


TU = r"""
#include <cstdint>
#include "gloo_amd/hip_allreduce.h"
using gloo_amd::HipReductionFunction;
static_assert(sizeof(gloo_amd::float8_e4m3fn) == 1 && sizeof(gloo_amd::float8_e5m2) == 1, "1-byte tags");
static_assert(gloo_amd::DType<gloo_amd::float8_e4m3fn>::value == 10, "F8E4M3");
static_assert(gloo_amd::DType<gloo_amd::float8_e5m2>::value == 11, "F8E5M2");
static_assert(GLOO_HIP_F8E4M3 == 10 && GLOO_HIP_F8E5M2 == 11 && GLOO_HIP_NUM_DTYPES == 12, "codes");
int main() {
  return HipReductionFunction<gloo_amd::float8_e4m3fn>::sum->type() == gloo_amd::SUM &&
                 HipReductionFunction<gloo_amd::float8_e5m2>::max->type() == gloo_amd::MAX ? 0 : 1;
}
"""


def test_cpp_header_has_the_fp8_tags(tmp_path):
    """gloo_amd::float8_e4m3fn / float8_e5m2 with their DType<> values: a small
    translation unit compiled (not linked, not run) with the flags of
    examples/ (gloo_amd/Makefile)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: gloo_amd/hip_allreduce.h includes the HIP runtime API and needs it to compile")
    src = tmp_path / "fp8_tu.cc"
    src.write_text(TU)
    cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "gloo_amd", "include"), "-c", str(src), "-o", str(tmp_path / "fp8_tu.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
