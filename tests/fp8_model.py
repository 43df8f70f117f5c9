"""The model of the FP8 dtypes (include/gloo_amd.h): torch on the CPU, i.e.
c10::Float8_e4m3fn / c10::Float8_e5m2, on raw bytes.

SUM / PRODUCT: widen both operands to f32, one f32 op, c10's rounding back
(nearest even, overflow not saturated); where the f32 result is a NaN the byte
is 0x7F (the project's rule: torch's own byte there carries an operand's sign
that one x86 build picked).  MAX / MIN: (a < b) ? b : a and (b < a) ? b : a
compared in f32, the raw operand byte copied.

Shared by tests/test_fp8_abi.py (which pins the model's facts) and
tests/test_fp8_gpu.py (which holds the kernels to it)."""
import numpy as np

FORMATS = {"f8e4m3": "float8_e4m3fn", "f8e5m2": "float8_e5m2"}
CODES = {"f8e4m3": 10, "f8e5m2": 11}
OPS = ("sum", "product", "max", "min")


def widen(dtype, x_u8):
    """f32 values of raw bytes (numpy in, numpy out)."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(x_u8, dtype=np.uint8))
    return x.view(getattr(torch, FORMATS[dtype])).float().numpy()


def fp8_op(op, dtype, a_u8, b_u8):
    """c = a op b on raw bytes; uint8 arrays of equal shape."""
    import torch
    dt = getattr(torch, FORMATS[dtype])
    a = torch.from_numpy(np.ascontiguousarray(a_u8, dtype=np.uint8).copy())
    b = torch.from_numpy(np.ascontiguousarray(b_u8, dtype=np.uint8).copy())
    fa, fb = a.view(dt).float(), b.view(dt).float()
    if op in ("sum", "product"):
        r = fa + fb if op == "sum" else fa * fb
        want = torch.where(torch.isnan(r), torch.tensor(0x7F, dtype=torch.uint8), r.to(dt).view(torch.uint8))
    elif op == "max":
        want = torch.where(fa < fb, b, a)
    elif op == "min":
        want = torch.where(fb < fa, b, a)
    else:
        raise ValueError(op)
    return want.numpy()


def fold_left(op, dtype, xs):
    """((x0 op x1) op x2) ..., rounding to the format after every op."""
    acc = np.ascontiguousarray(xs[0], dtype=np.uint8).copy()
    for x in xs[1:]:
        acc = fp8_op(op, dtype, acc, x)
    return acc


def fold_right(op, dtype, xs):
    """x0 op (x1 op (... op x_last))."""
    acc = np.ascontiguousarray(xs[-1], dtype=np.uint8).copy()
    for x in xs[-2::-1]:
        acc = fp8_op(op, dtype, x, acc)
    return acc


class ModelOracle:
    """Stands in for tests/plan_sim.py's `oracle` (reduce3 only)."""

    @staticmethod
    def reduce3(op, dtype, a, b):
        return fp8_op(op, dtype, a, b)


def table():
    """Every operand pair: a[i] = i >> 8, b[i] = i & 255, 65,536 elements."""
    i = np.arange(65536, dtype=np.uint32)
    return (i >> 8).astype(np.uint8), (i & 255).astype(np.uint8)


def is_nan(dtype, x_u8):
    m = np.asarray(x_u8) & 0x7F
    return m == 0x7F if dtype == "f8e4m3" else m > 0x7C


def is_finite(dtype, x_u8):
    m = np.asarray(x_u8) & 0x7F
    return m != 0x7F if dtype == "f8e4m3" else m < 0x7C


def small_bytes(dtype, bound=16.0):
    """The finite bytes with |v| <= bound, both zeros included."""
    b = np.arange(256, dtype=np.uint8)
    v = widen(dtype, b)
    return b[is_finite(dtype, b) & (np.abs(v) <= bound)]


def draw_small(rng, dtype, shape, bound=16.0):
    return rng.choice(small_bytes(dtype, bound), size=shape).astype(np.uint8)
