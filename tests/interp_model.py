"""The model of the one-launch plan interpreter (reduce.hip plan_interp_kernel,
signal.h InterpStep) on numpy byte arrays, built on tests/fold_model.py, and
the shapes tests/test_interp_kernel_gpu.py runs.  CPU only; it never calls the
library under test.

run_steps() executes a step list in order over WHOLE ranges: a sliced launch
(G workgroups, each on its own slice of every step) must not change a byte.
  COPY   dst and every xdst := src                     (bytes)
  SEND   dst := src, then flag[g] := value, g < G
  SIGNAL flag[g] := value, g < G
  WAIT   met when flag[g] - value >= 0 as a signed 64-bit difference for every
         g < G; an unmet wait stops the list and sets err
  FOLD   dst := fold_model.fold(op, dtype, sources, mode)
value = (base + run * per_run) mod 2^64.  Reaching the end: done = run, the
ticket word 0.  A buffer is (name, element offset); flags are name -> a list
of words.

slice_bounds() is the model's own statement of what workgroup g of G takes of
an n-element step: q = ceil(ceil(n / G) / kV) * kV elements per slice, kV = 16
/ es, lo = min(n, g q), hi = min(n, lo + q).

Shapes: with CP = 65536 bytes per copy pass and FP = 8192 (1-byte types) or
32768 bytes per fold pass -- the defaults of GLOO_AMD_INTERP_BLOCK (512) x
GLOO_AMD_INTERP_COPY_UNROLL (8) / GLOO_AMD_INTERP_FOLD_UNROLL (4; 1 for
1-byte types) x 16 -- copy_sizes / fold_sizes straddle one packet and one
pass and end beyond two passes with a packet and a ragged tail.
"""
import collections

import numpy as np

import fold_model as fm

COPY, SEND, SIGNAL, WAIT, FOLD = range(5)
M64 = (1 << 64) - 1

Step = collections.namedtuple("Step", "kind dst src n mode flag base per_run xdst",
                              defaults=(None, (), 0, 0, None, 0, 0, ()))
Result = collections.namedtuple("Result", "err done ticket stopped written")

CP = 65536
SLICE_COUNTS = (1, 2, 3, 4, 8)
MANY_SLICES = 256


def fp_bytes(es):
    return 8192 if es == 1 else 32768


def copy_sizes(es):
    """Elements.  u8: the byte sizes; wider types: the pass boundary only."""
    if es == 1:
        return [1, 15, 16, 17, CP - 1, CP, CP + 1, 2 * CP + 16 + 3]
    return [CP // es - 1, CP // es, CP // es + 1, 2 * (CP // es) + 16 // es + 3]


def fold_sizes(es):
    kV, F = 16 // es, fp_bytes(es) // es
    out = []
    for n in (1, kV - 1, kV, kV + 1, F - 1, F, F + 1, 2 * F + kV + 3):
        if n > 0 and n not in out:
            out.append(n)
    return out


def sliced_sizes(G, es):
    """Several packets and one element over; slices 2 and up empty; n a multiple of q."""
    kV = 16 // es
    return [3 * G * kV + 1, kV + 1, 2 * G * kV]


def gpu_shapes():
    """Every (n, G, es) the GPU tests run a data step at."""
    out = set()
    for es in (1, 2, 4, 8):
        for n in copy_sizes(es) + fold_sizes(es) + [fp_bytes(es) // es + 16 // es + 3]:
            out.add((n, 1, es))
        for G in SLICE_COUNTS + (MANY_SLICES,):
            for n in sliced_sizes(G, es):
                out.add((n, G, es))
    return sorted(out)


def slice_bounds(n, G, es):
    kV = 16 // es
    per = -(-n // G)
    q = -(-per // kV) * kV
    return [(min(n, g * q), min(n, min(n, g * q) + q)) for g in range(G)]


def value(s, run):
    return (s.base + run * s.per_run) & M64


def met(word, target):
    """flag - target >= 0 as a signed 64-bit difference."""
    return ((int(word) - int(target)) & M64) < (1 << 63)


def run_steps(op, dtype, steps, bufs, flags, run, G=1):
    """Runs `steps` on bufs (name -> uint8 array, modified in place) and flags
    (name -> list of words, modified in place)."""
    es = fm.itemsize(dtype)
    written = {k: np.zeros(v.size, bool) for k, v in bufs.items()}

    def span(ref, n):
        name, off = ref
        assert (off + n) * es <= bufs[name].size, (ref, n)
        return bufs[name][off * es:(off + n) * es]

    def store(ref, data):
        span(ref, data.size // es)[:] = data
        written[ref[0]][ref[1] * es:ref[1] * es + data.size] = True

    for i, s in enumerate(steps):
        if s.kind == WAIT:
            if not all(met(flags[s.flag][g], value(s, run)) for g in range(G)):
                return Result(1, None, 0, i, written)
            continue
        if s.kind in (COPY, SEND):
            assert len(s.src) == 1 and (s.kind == COPY or not s.xdst)
            data = span(s.src[0], s.n).copy()
            for d in (s.dst,) + tuple(s.xdst):
                store(d, data)
        elif s.kind == FOLD:
            srcs = [span(r, s.n).copy().view(fm.STORAGE[dtype]) for r in s.src]
            store(s.dst, np.ascontiguousarray(fm.fold(op, dtype, srcs, s.mode)).view(np.uint8))
        else:
            assert s.kind == SIGNAL
        if s.kind in (SEND, SIGNAL):
            for g in range(G):
                flags[s.flag][g] = value(s, run)
    return Result(0, run & M64, 0, len(steps), written)


_cases = {}


def fold_case(op, dtype, k, n, seed=0):
    """The k sources of fold_model.inputs for (op, dtype), computed once."""
    key = (op, dtype, k, n, seed)
    if key not in _cases:
        rng = np.random.default_rng([seed, k, n, fm.DTYPES.index(dtype), fm.ops_of(dtype).index(op)])
        _cases[key] = fm.inputs(op, dtype, k, n, rng)
    return _cases[key]


def modes_of(k):
    return (0, 1, 2) if k & (k - 1) == 0 else (0, 1)


# The loopback chain: every kind of step in ONE list, each wait met by an
# earlier step of the same list.
CHAIN_BUFFERS = ("in", "work", "x1", "x2", "s1", "s2", "inbox", "out", "out2", "x3")
CHAIN_SOURCES = ("in", "s1", "s2", "inbox")  # what holds data before the launch
F0_SEQ, F1_SEQ = (5, 3), (100, 7)            # (base, per_run)


def chain(n, sub=None):
    """sub = (a, m): the SEND moves elements [a, a + m) only (one workgroup;
    the rest of the inbox keeps what it held)."""
    a, m = sub if sub else (0, n)
    return [
        Step(COPY, ("work", 0), (("in", 0),), n, xdst=(("x1", 0), ("x2", 0))),
        Step(FOLD, ("work", 0), (("work", 0), ("s1", 0), ("s2", 0)), n, mode=0),
        Step(SIGNAL, flag="f0", base=F0_SEQ[0], per_run=F0_SEQ[1]),
        Step(SEND, ("inbox", a), (("work", a),), m, flag="f1", base=F1_SEQ[0], per_run=F1_SEQ[1]),
        Step(WAIT, flag="f1", base=F1_SEQ[0], per_run=F1_SEQ[1]),
        Step(FOLD, ("out", 0), (("work", 0), ("inbox", 0)), n, mode=0),
        Step(COPY, ("out2", 0), (("out", 0),), n, xdst=(("x3", 0),)),
    ]


def chain_inputs(op, dtype, n, seed=0):
    """name -> bytes of the chain's four sources (the inbox's prior content included)."""
    srcs = fold_case(op, dtype, 4, n, seed=100 + seed)
    return {name: np.ascontiguousarray(s).view(np.uint8).copy() for name, s in zip(CHAIN_SOURCES, srcs)}


def chain_buffers(inputs, n, es):
    """Fresh model buffers: the sources, and zeros for everything a step writes first."""
    return {name: inputs[name].copy() if name in inputs else np.zeros(n * es, np.uint8) for name in CHAIN_BUFFERS}
