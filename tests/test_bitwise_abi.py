"""CPU: the bitwise reductions BAND / BOR / BXOR at the C-ABI boundary — the
enum values in the Python binding and in include/gloo_amd.h, the op x dtype
rule (integer dtypes only; a floating dtype is GLOO_HIP_EINVAL_OP before n or
any pointer is looked at), gloo_hip_op_supported, and the C++ face
(HipReductionFunction<T>::band / bor / bxor).  Nothing here touches the GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BITWISE = {"band": 5, "bor": 6, "bxor": 7}
INT_DTYPES = {"i8": 0, "u8": 1, "i32": 2, "u32": 3, "i64": 4, "u64": 5}
FLOAT_DTYPES = {"f16": 6, "bf16": 7, "f32": 8, "f64": 9}


def test_enum_values_python_and_header():
    import gloo_amd
    assert int(gloo_amd.ReductionType.BAND) == 5
    assert int(gloo_amd.ReductionType.BOR) == 6
    assert int(gloo_amd.ReductionType.BXOR) == 7
    text = open(os.path.join(ROOT, "include", "gloo_amd.h")).read()
    enum = re.search(r"typedef enum \{([^}]*)\}\s*gloo_hip_op_t;", text).group(1)
    values = {k: int(v) for k, v in re.findall(r"GLOO_HIP_(\w+)\s*=\s*(\d+)", enum)}
    assert values == {"SUM": 1, "PRODUCT": 2, "MAX": 3, "MIN": 4, "BAND": 5, "BOR": 6, "BXOR": 7}


def test_op_names():
    import gloo_amd
    for name, code in BITWISE.items():
        assert int(gloo_amd.OP_NAMES[name]) == code
    assert set(gloo_amd.OP_NAMES) == {"sum", "product", "max", "min", "band", "bor", "bxor"}


def test_integer_dtypes_accepted_without_a_gpu():
    import gloo_amd
    L = gloo_amd.lib
    assert L.gloo_hip_reduce(5, 2, None, None, 0, None) == 0
    # a valid op x dtype: the null pointers are the error
    assert L.gloo_hip_reduce(6, 2, None, None, 5, None) == -3
    for op in BITWISE.values():
        for dt in INT_DTYPES.values():
            assert L.gloo_hip_reduce(op, dt, None, None, 0, None) == 0, (op, dt)


@pytest.mark.parametrize("op_name,op", sorted(BITWISE.items()))
@pytest.mark.parametrize("dt_name,dt", sorted(FLOAT_DTYPES.items()))
def test_floating_dtypes_are_einval_op(op_name, op, dt_name, dt):
    import ctypes

    import gloo_amd
    L = gloo_amd.lib
    arr = (ctypes.c_void_p * 1)(None)
    calls = {
        "reduce": lambda n: L.gloo_hip_reduce(op, dt, None, None, n, None),
        "reduce3": lambda n: L.gloo_hip_reduce3(op, dt, None, None, None, n, None),
        "reduce_multi": lambda n: L.gloo_hip_reduce_multi(op, dt, None, arr, 1, n, None),
    }
    for what, call in calls.items():
        # before the n == 0 shortcut, and before the pointer checks at n > 0
        for n in (0, 5):
            L.gloo_hip_reduce(1, 8, None, None, 0, None)  # a success in between: the message below is this call's
            assert call(n) == -1, (what, n)
            msg = L.gloo_hip_last_error().decode()
            assert "op" in msg and op_name in msg and dt_name in msg, (what, n, msg)


def test_op_8_is_still_invalid():
    import gloo_amd
    L = gloo_amd.lib
    assert L.gloo_hip_reduce(8, 2, None, None, 0, None) == -1
    assert L.gloo_hip_reduce(8, 8, None, None, 0, None) == -1
    assert L.gloo_hip_reduce(999, 2, None, None, 0, None) == -1


def test_op_supported():
    import gloo_amd
    S = gloo_amd.lib.gloo_hip_op_supported
    for op in (5, 6, 7):
        for dt in INT_DTYPES.values():
            assert S(op, dt) == 1, (op, dt)
        for dt in FLOAT_DTYPES.values():
            assert S(op, dt) == 0, (op, dt)
    for op in (1, 2, 3, 4):
        for dt in range(10):
            assert S(op, dt) == 1, (op, dt)
    for dt in range(10):
        assert S(8, dt) == 0 and S(0, dt) == 0 and S(999, dt) == 0
    for op in range(1, 8):
        assert S(op, 42) == 0 and S(op, -1) == 0
    assert gloo_amd.op_supported("bxor", "u64") is True
    assert gloo_amd.op_supported("bxor", "f32") is False
    assert gloo_amd.op_supported("sum", "bf16") is True


TU = r"""
#include <cstdint>
#include "gloo_amd/hip_allreduce.h"
using gloo_amd::HipReductionFunction;
int main() {
  const HipReductionFunction<int32_t>* f = HipReductionFunction<int32_t>::bxor;
  static_assert(gloo_amd::BAND == 5 && gloo_amd::BOR == 6 && gloo_amd::BXOR == 7, "op codes");
  return f->type() == gloo_amd::BXOR && HipReductionFunction<uint8_t>::band->type() == gloo_amd::BAND &&
                 HipReductionFunction<int64_t>::bor->type() == gloo_amd::BOR ? 0 : 1;
}
"""


def test_cpp_header_names_the_bitwise_functions(tmp_path):
    """HipReductionFunction<T>::band / bor / bxor exist beside sum..max: a
    small translation unit compiled (not linked, not run) with the flags of
    examples/ (gloo_amd/Makefile)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: gloo_amd/hip_allreduce.h includes the HIP runtime API and needs it to compile")
    src = tmp_path / "bitwise_tu.cc"
    src.write_text(TU)
    cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "gloo_amd", "include"), "-c", str(src), "-o", str(tmp_path / "bitwise_tu.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
