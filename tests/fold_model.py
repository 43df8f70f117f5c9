"""The model of a k-source fold (reduce.hip fold_elem / fold_tile / tree_fold)
on numpy storage arrays, and the inputs the fold tests feed it.  CPU only; it
never calls the library under test.

fold(op, dtype, srcs, mode) is built from the 3-operand models the suite
already trusts: oracle.reduce3 (the C restatement of gloo/math.h; its f16 max /
min follows the CUDA-twin rule tests/test_reduce_gpu.py::expected documents)
for the ten classic dtypes, fp8_model.fp8_op for the two FP8 dtypes, and numpy
& | ^ on the unsigned view for the bitwise ops.  Orders:
  mode 0 (left):    acc = op(acc, s_j), j = 1 .. k-1
  mode 1 (reverse): acc = op(s_j, acc), j = 1 .. k-1
  mode 2 (tree):    level by level, v[j] = op(v[2j], v[2j+1]); k a power of two

Inputs: `mixed` (magnitudes spread over several decades, so that the
association of a sum shows in the rounding), `specials` (signed quiet /
signalling NaNs, zeros, infinities, +-1 and 2: max / min and the f16 NaN rule
return an operand's own bits, so the operand order shows), and full-range
random bytes for the integers.  tests/test_fold_model.py pins that these
inputs tell the three orders apart where IEEE arithmetic lets them differ.
"""
import numpy as np

import fp8_model
import oracle

STORAGE = {name: npt for name, (_, npt) in oracle.DTYPES.items()}
STORAGE.update({"f8e4m3": np.uint8, "f8e5m2": np.uint8})
DTYPES = tuple(STORAGE)
INTEGERS = ("i8", "u8", "i32", "u32", "i64", "u64")
FLOATS = tuple(d for d in DTYPES if d not in INTEGERS)
ARITH = ("sum", "product", "max", "min")
BITWISE = ("band", "bor", "bxor")
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def itemsize(dtype):
    return np.dtype(STORAGE[dtype]).itemsize


def ops_of(dtype):
    return ARITH + (BITWISE if dtype in INTEGERS else ())


def op2(op, dtype, a, b):
    """c = a op b on storage arrays, by the trusted 3-operand model."""
    if op in BITWISE:
        if dtype not in INTEGERS:
            raise ValueError(f"{op} on {dtype}")
        u = UNSIGNED[itemsize(dtype)]
        ua, ub = np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u)
        r = ua & ub if op == "band" else ua | ub if op == "bor" else ua ^ ub
        return r.view(STORAGE[dtype])
    if dtype in fp8_model.FORMATS:
        return fp8_model.fp8_op(op, dtype, a, b)
    return oracle.reduce3(op, dtype, a, b)


def fold(op, dtype, srcs, mode):
    """The fold of `srcs` (storage arrays of equal length) in `mode`'s order."""
    k = len(srcs)
    v = [np.ascontiguousarray(s, dtype=STORAGE[dtype]).copy() for s in srcs]
    if mode == 2:
        if k & (k - 1):
            raise ValueError("tree fold needs a power-of-two count")
        while len(v) > 1:
            v = [op2(op, dtype, v[2 * j], v[2 * j + 1]) for j in range(len(v) // 2)]
        return v[0]
    acc = v[0]
    for s in v[1:]:
        acc = op2(op, dtype, s, acc) if mode == 1 else op2(op, dtype, acc, s)
    return acc


def bits(x):
    """The unsigned view of a storage array (NaN-proof comparison)."""
    x = np.ascontiguousarray(x)
    return x.view(UNSIGNED[x.dtype.itemsize])


def mixed(dtype, n, rng):
    """Normal values times a power of ten; the 16-bit formats get fewer
    decades (their sums stay finite) and FP8 the finite bytes up to 16."""
    if dtype in INTEGERS:
        return integers(dtype, n, rng)
    if dtype in fp8_model.FORMATS:
        return fp8_model.draw_small(rng, dtype, n)
    wide = dtype in ("f32", "f64")
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n) if wide else \
        rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)
    if dtype == "f16":
        return x.astype(np.float16).view(np.uint16)
    if dtype == "bf16":
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return x.astype(STORAGE[dtype])


# exponent bits, mantissa bits of the IEEE-like formats
LAYOUT = {"f16": (5, 10), "bf16": (8, 7), "f32": (8, 23), "f64": (11, 52)}


def special_patterns(dtype):
    """Signed quiet and signalling NaNs (two payloads each), +-0, +-inf, +-1, 2."""
    e, m = LAYOUT[dtype]
    sign = 1 << (e + m)
    exp_all = ((1 << e) - 1) << m
    quiet = 1 << (m - 1)
    one = ((1 << (e - 1)) - 1) << m
    two = (1 << (e - 1)) << m
    pos = [exp_all | quiet, exp_all | quiet | 1, exp_all | (quiet >> 1), exp_all | 1,  # qNaN x 2, sNaN x 2
           0, exp_all, one]
    return np.array(pos + [p | sign for p in pos] + [two], dtype=UNSIGNED[(1 + e + m) // 8])


def specials(dtype, n, rng):
    """A random choice of special_patterns; FP8: every byte value; integers:
    full-range random bytes."""
    if dtype in INTEGERS:
        return integers(dtype, n, rng)
    if dtype in fp8_model.FORMATS:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rng.choice(special_patterns(dtype), size=n).view(STORAGE[dtype])


def integers(dtype, n, rng):
    return rng.integers(0, 256, n * itemsize(dtype), dtype=np.uint8).view(STORAGE[dtype])


def inputs(op, dtype, k, n, rng):
    """The k sources the GPU tests use for (op, dtype): `specials` for max /
    min and for f16 sum / product (the NaN-payload rule), `mixed` otherwise.
    Never two NaNs of different payload into f32 / f64 sum / product: no
    golden pins those bits."""
    gen = specials if op in ("max", "min") or (dtype == "f16" and op in ("sum", "product")) else mixed
    return [gen(dtype, n, rng) for _ in range(k)]
