"""The numpy model of include/gloo_amd.h "MX stochastic rounding", on top of mx_model / mx_quant_model: their
accumulation, NaN block and scale steps as they are, the elements step of a finite block replaced."""
import numpy as np

import mx_quant_model as qm
from mx_model import BLOCK_BYTES, TABLE, pack

U, M32 = np.uint64, np.uint64(0xFFFFFFFF)


def fmix32(h):
    """MurmurHash3's finaliser on uint64 arrays holding 32-bit values."""
    h = (h ^ h >> U(16)) * U(0x85EBCA6B) & M32
    h = (h ^ h >> U(13)) * U(0xC2B2AE35) & M32
    return h ^ h >> U(16)


def r16(seed, n):
    """R16(i) for i < n."""
    seed, p = U(seed % 2 ** 64), np.arange(n, dtype=U) >> U(1)
    W = fmix32((((p & M32) ^ fmix32(seed & M32) ^ seed >> U(32)) + U(0x9E3779B9) * (p >> U(32))) & M32)
    return np.where(np.arange(n) % 2 == 0, W & U(0xFFFF), W >> U(16)).astype(np.int64)


def requantise(fmt, a, seed):
    """(nblocks, 32) f32 accumulators -> (element bytes, scale bytes)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 32)
    elems, X = qm.quantise(fmt, a)  # the scale and NaN block steps; the elements of finite blocks are replaced below
    finite = TABLE[fmt][: TABLE[fmt].size // 2]
    finite = finite[np.isfinite(finite)]  # ascending magnitudes, index = code
    inv = ((254 - np.where(X == 255, 0, X).astype(np.uint32)) << 23).view(np.float32)  # 2^(127 - X_out)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.minimum(np.abs(np.where(np.isfinite(a), a, np.float32(0)) * inv[:, None]).astype(np.float64), finite[-1])
    hi = np.searchsorted(finite, q, "left")
    lo = np.where(finite[hi] == q, hi, hi - 1)
    frac16 = np.floor((q - finite[lo]) / np.where(hi == lo, 1.0, finite[hi] - finite[lo]) * 65536).astype(np.int64)
    code = np.where(frac16 + r16(seed, a.size).reshape(-1, 32) >= 65536, hi, lo)
    out = pack(fmt, code | np.signbit(a).astype(np.int64) << (3 if fmt == "mxfp4_e2m1" else 7)).reshape(-1, BLOCK_BYTES[fmt])
    out[X == 255] = elems.reshape(-1, BLOCK_BYTES[fmt])[X == 255]
    return out.reshape(-1), X


def quantise(fmt, x, seed):
    """mx_quant_model.quantise with stochastic rounding: (nblocks, 32) wide values -> (element bytes, scale bytes)."""
    x = np.asarray(x)
    return requantise(fmt, (x.astype(np.uint32) << 16).view(np.float32) if x.dtype == np.uint16 else x.astype(np.float32), seed)


def fold(fmt, srcs, seed):
    """mx_model.fold with stochastic rounding: the f32 wide fold's accumulators, requantised."""
    return requantise(fmt, qm.fold_wide(fmt, "f32", srcs).view(np.float32), seed)
