"""The numpy model of the MX block-scaled sum (include/gloo_amd.h "MX
block-scaled sum").  Element tables and every integer step are exact; the
multiplies and the accumulation are sequential np.float32 operations."""
import numpy as np

FORMATS = ("mxfp8_e4m3", "mxfp8_e5m2", "mxfp4_e2m1")
EMAX = {"mxfp8_e4m3": 8, "mxfp8_e5m2": 15, "mxfp4_e2m1": 2}
BLOCK_BYTES = {"mxfp8_e4m3": 32, "mxfp8_e5m2": 32, "mxfp4_e2m1": 16}
NAN_BYTE = {"mxfp8_e4m3": 0x7F, "mxfp8_e5m2": 0x7F, "mxfp4_e2m1": 0x00}  # e2m1 has no NaN: the scale carries it


def _table(bits, mbits, bias, fn):
    """float64 value of every code of a sign / exponent / mantissa format of `bits` bits."""
    c = np.arange(1 << bits)
    e, m = (c >> mbits) & ((1 << (bits - 1 - mbits)) - 1), c & ((1 << mbits) - 1)
    mag = np.where(e == 0, m * 2.0 ** (1 - bias - mbits), (1 + m * 2.0 ** -mbits) * 2.0 ** (e - bias))
    if bits == 8 and fn:       # e4m3fn: no infinity, S.1111.111 is NaN
        mag[(c & 0x7F) == 0x7F] = np.nan
    elif bits == 8:            # e5m2: IEEE-like
        mag[(e == 31) & (m == 0)], mag[(e == 31) & (m != 0)] = np.inf, np.nan
    return np.where(c >> (bits - 1) == 1, -mag, mag)


TABLE = {"mxfp8_e4m3": _table(8, 3, 7, True), "mxfp8_e5m2": _table(8, 2, 15, False), "mxfp4_e2m1": _table(4, 1, 1, False)}


def codes(fmt, elem_bytes):
    """(nblocks, 32) element codes; MXFP4: element 2i is the low nibble of byte i."""
    b = np.asarray(elem_bytes, np.uint8).reshape(-1, BLOCK_BYTES[fmt])
    return b if fmt != "mxfp4_e2m1" else np.stack([b & 15, b >> 4], -1).reshape(-1, 32)


def pack(fmt, c):
    c = c.astype(np.uint8)
    return (c if fmt != "mxfp4_e2m1" else c[:, 0::2] | c[:, 1::2] << 4).reshape(-1)


def fold(fmt, srcs):
    """srcs: k (element bytes, scale bytes) pairs in list order -> (element bytes, scale bytes)."""
    table, emax = TABLE[fmt], EMAX[fmt]
    a = None
    with np.errstate(invalid="ignore", over="ignore"):
        for elems, X in srcs:
            X = np.asarray(X, np.uint32)
            scale = np.where(X == 0, 0x00400000, X << 23).astype(np.uint32).view(np.float32)  # 2^(X - 127); 255: inf
            v = table[codes(fmt, elems)].astype(np.float32) * scale[:, None]
            v[X == 255] = np.nan
            a = v if a is None else a + v
    assert a.dtype == np.float32
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
