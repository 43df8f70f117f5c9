"""CPU: GLOO_HIP_SUM_WIDE (257 = SUM | GLOO_HIP_WIDE) at the C-ABI boundary:
which dtypes take it, that the modifier bit goes with SUM only, and that the
refusal names the op and the dtype before n or a pointer is looked at.
Nothing here touches the GPU."""
import ctypes

import pytest

NARROW = (6, 7, 10, 11)  # f16, bf16, f8e4m3, f8e5m2


def test_op_supported():
    import gloo_amd
    S = gloo_amd.lib.gloo_hip_op_supported
    assert int(gloo_amd.ReductionType.SUM_WIDE) == 257 == gloo_amd.ReductionFunction.sum_wide.type()
    for dt in range(-1, 14):
        assert S(257, dt) == (1 if dt in NARROW else 0), dt
        for op in (0, 2, 3, 4, 5, 6, 7, 8):
            assert S(0x100 | op, dt) == 0, (op, dt)
    assert gloo_amd.op_supported("sum_wide", "bf16") and not gloo_amd.op_supported("sum_wide", "f32")


@pytest.mark.parametrize("n", [0, 5])
def test_f32_is_refused_by_name(n):
    import gloo_amd
    L = gloo_amd.lib
    arr = (ctypes.c_void_p * 3)(None, None, None)
    for call in (lambda: L.gloo_hip_reduce(257, 8, None, None, n, None),
                 lambda: L.gloo_hip_reduce_multi(257, 8, None, arr, 3, n, None),
                 lambda: L.gloo_hip_fold_kernel(257, 8, None, arr, 3, n, 0, None, None, None, 0, None, None)):
        L.gloo_hip_reduce(1, 8, None, None, 0, None)  # a success in between: the message below is this call's
        assert call() == -1
        msg = L.gloo_hip_last_error().decode()
        assert "sum_wide" in msg and "f32" in msg, msg
    for dt in NARROW:  # the four dtypes pass: n == 0 is a success, a null pointer the error otherwise
        assert L.gloo_hip_reduce_multi(257, dt, None, arr, 3, n, None) == (0 if n == 0 else -3), dt
