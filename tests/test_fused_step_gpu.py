"""GPU, one process: gloo_hip_fused_step (reduce.hip fused_small_kernel, the
step [wait] -> dst op= src -> [signal] in one one-workgroup launch) against
tests/fold_model.py, bit for bit.

The workgroup is 512 lanes: n = 1, 511, 512, 513 and 1027 (two strides and a
bit).  dst and src sit at different element-aligned residues past a 256-byte
boundary; the ranges are disjoint, so there is no in-place form.  Forms: no
flag; a wait the host has met exactly; a wait whose counter is above its target;
a signal; both.  A sequence value is base + epoch * per_run (mod 2^64) with
epoch a device word holding 0, 3 or 2^40, or base alone without one.  Every
wait but the last test's is met before the launch (timeout 10^7 ticks); that
one is never met and gives up after 2 * 10^5 ticks (2 ms).

The harness is tests/guard_rig.py, as tests/test_interp_kernel_gpu.py: guard
bytes around both buffers and every control word, dst pre-filled by the step's
first operand, the source checked unmodified.
"""
import numpy as np
import pytest

import fold_model as fm
import guard_rig
import interp_model as im

pytestmark = pytest.mark.gpu

SIZES = (1, 511, 512, 513, 1027)
FORMS = ("none", "wait met", "wait below", "signal", "both")
EPOCHS = (None, 0, 3, 1 << 40)
WAIT_SEQ, SIG_SEQ = (1 << 50, 7), (im.M64 - 10, 1 << 20)  # (base, per_run)


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gloo_amd
    import hip_rt
    hip_rt.set_device(0)
    rig = guard_rig.Rig(hip_rt, guard_rig.GUARD + 16 + max(SIZES) * 8 + guard_rig.GUARD)
    epoch = hip_rt.malloc(8)
    yield gloo_amd, rig, epoch
    hip_rt.free(epoch)
    rig.close()


def seq(pair, epoch):
    return (pair[0] + (epoch or 0) * pair[1]) & im.M64


def operands(op, dtype, n):
    if op == 0:
        rng = np.random.default_rng([11, n, fm.DTYPES.index(dtype)])
        return [fm.integers(dtype, n, rng) for _ in range(2)]
    return im.fold_case(op, dtype, 2, n, seed=5)


def run_step(dev, op, dtype, n, form, epoch, doff, soff, what, timeout=10 ** 7, unmet=False):
    gloo_amd, rig, epoch_word = dev
    es = fm.itemsize(dtype)
    d, s = operands(op, dtype, n)
    want = s if op == 0 else fm.op2(op, dtype, d, s)
    waits, signals = form in ("wait met", "wait below", "both") or unmet, form in ("signal", "both")
    wt, sv = seq(WAIT_SEQ, epoch), seq(SIG_SEQ, epoch)
    counter = 0 if unmet else wt + (1 << 62) if form == "wait below" else wt
    flags = {"f0": [counter & im.M64] * guard_rig.NW, "f1": [99] * guard_rig.NW}
    rig.set_words(flags)
    if epoch is not None:
        rig.rt.h2d(epoch_word, np.array([epoch], np.uint64))
    dp, sp = rig.place("d", doff, d), rig.place("s", soff, s)
    gloo_amd.fused_step(op, dtype, dp, sp, n, rig.words + guard_rig.ERR,
                        wait_flag=rig.flag_ptr("f0") if waits else 0, wait_base=WAIT_SEQ[0], wait_per_run=WAIT_SEQ[1],
                        sig_flag=rig.flag_ptr("f1") if signals else 0, sig_base=SIG_SEQ[0], sig_per_run=SIG_SEQ[1],
                        epoch=epoch_word if epoch is not None else 0, timeout_ticks=timeout)
    rig.rt.synchronize()
    rig.check("d", doff, d if unmet else want, what, es)
    rig.check("s", soff, s, what, es)
    if signals and not unmet:
        flags["f1"][0] = sv
    rig.check_words(flags, guard_rig.DONE_INIT, 0, 1 if unmet else 0, what)
    if epoch is not None:
        assert int(rig.rt.d2h(epoch_word, np.empty(1, np.uint64))[0]) == epoch


def residues(es):
    """(dst, src) byte offsets at different residues of 16."""
    return [(es % 16, 0), (0, 16 - es), (16 - es, 8 % 16 if es < 8 else 0)]


@pytest.mark.parametrize("dtype,op", [(d, o) for d in fm.DTYPES for o in fm.ops_of(d) + (0,)])
def test_every_dtype_and_op(dev, dtype, op):
    """Every size in every form; the epoch forms and the offsets rotate."""
    es = fm.itemsize(dtype)
    R = residues(es)
    for i, n in enumerate(SIZES):
        for j, form in enumerate(FORMS):
            doff, soff = R[(i + j) % len(R)]
            assert doff % 16 != soff % 16
            run_step(dev, op, dtype, n, form, EPOCHS[(i + j) % len(EPOCHS)], doff, soff, (dtype, op, "n", n, form))


@pytest.mark.parametrize("dtype,op", [("f32", "sum"), ("u8", 0), ("bf16", "max")])
def test_every_form_under_every_epoch(dev, dtype, op):
    es = fm.itemsize(dtype)
    for form in FORMS:
        for epoch in EPOCHS:
            for n in (513, 1027):
                run_step(dev, op, dtype, n, form, epoch, es, 16 - es if es < 8 else 0, (dtype, op, form, "epoch", epoch))
    assert seq(SIG_SEQ, 3) < 1 << 32 and seq(WAIT_SEQ, 1 << 40) == (1 << 50) + 7 * (1 << 40)  # one wraps, one is scaled


def test_unmet_wait_times_out(dev):
    """2 ms: err is 1, dst is untouched and the flag is not signalled."""
    for op, epoch in (("sum", None), (0, 3)):
        run_step(dev, op, "f32", 1027, "both", epoch, 4, 8, ("unmet wait", op), timeout=2 * 10 ** 5, unmet=True)
