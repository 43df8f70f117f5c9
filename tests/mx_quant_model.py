"""The numpy model of include/gloo_amd.h "MX quantise and wide-output fold", on top of mx_model.  Wide arrays are
np.float32, np.float16, or bf16 as np.uint16 bits; wide results are returned as bits (np.uint32 / np.uint16)."""
import numpy as np

from mx_model import BLOCK_BYTES, EMAX, NAN_BYTE, TABLE, codes, pack

DTYPES = ("f32", "f16", "bf16")
CANONICAL_NAN = {"f32": 0x7FC00000, "f16": 0x7E00, "bf16": 0x7FC0}


def quantise(fmt, x):
    """(nblocks, 32) wide values -> (element bytes, scale bytes): mx_model.fold's steps behind the accumulation."""
    table, emax = TABLE[fmt], EMAX[fmt]
    x = np.asarray(x)  # widened exactly
    a = ((x.astype(np.uint32) << 16).view(np.float32) if x.dtype == np.uint16 else x.astype(np.float32)).reshape(-1, 32)
    nan_block = ~np.isfinite(a).all(1)
    fin = np.where(np.isfinite(a), a, np.float32(0))
    F = (np.abs(fin).max(1).view(np.uint32) >> 23).astype(np.int64)
    Xout = np.maximum(F - emax, 0)
    inv = ((254 - Xout) << 23).astype(np.uint32).view(np.float32)  # 2^(127 - X_out)
    finite = table[: table.size // 2][np.isfinite(table[: table.size // 2])]  # ascending magnitudes, index = code
    q = np.minimum(np.abs(fin * inv[:, None]).astype(np.float64), finite[-1])
    hi = np.minimum(np.searchsorted(finite, q, "left"), finite.size - 1)
    lo = np.maximum(hi - 1, 0)
    mid = (finite[lo] + finite[hi]) / 2
    code = np.where((q < mid) | ((q == mid) & (lo % 2 == 0)), lo, hi)  # nearest, ties to the even mantissa
    code = code | np.signbit(a).astype(np.int64) << (3 if fmt == "mxfp4_e2m1" else 7)
    out = pack(fmt, code).reshape(-1, BLOCK_BYTES[fmt])
    out[nan_block] = NAN_BYTE[fmt]
    return out.reshape(-1), np.where(nan_block, 255, Xout).astype(np.uint8)


def fold_wide(fmt, dtype, srcs):
    """k (element bytes, scale bytes) pairs in list order -> the bits of nblocks * 32 elements of `dtype`."""
    a = None
    with np.errstate(invalid="ignore", over="ignore"):
        for elems, X in srcs:
            X = np.asarray(X, np.uint32)
            scale = np.where(X == 0, 0x00400000, X << 23).astype(np.uint32).view(np.float32)  # 2^(X - 127); 255: inf
            v = TABLE[fmt][codes(fmt, elems)].astype(np.float32) * scale[:, None]
            v[X == 255] = np.nan
            a = v if a is None else a + v
        assert a.dtype == np.float32
        bits = a.view(np.uint32).astype(np.uint64)
        if dtype == "bf16":  # round to nearest even on the bits; an inf stays
            bits = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
        elif dtype == "f16":
            bits = a.astype(np.float16).view(np.uint16)
    out = np.where(np.isnan(a), CANONICAL_NAN[dtype], bits)
    return out.astype(np.uint32 if dtype == "f32" else np.uint16).reshape(-1)
