"""GPU: the pipelined halving-doubling through the Gloo-surface bridge.

oracle/_ref/hd_pipelined_test (tests/bridge/hd_pipelined_test.cc, built by
oracle/hd_pipelined.mk against the reference's own headers and objects) builds
gloo::HipAllreduceHalvingDoublingPipelined<float> and
gloo::HipAllreduceHalvingDoubling<float>(..., pipelineBroadcastAndReduce) from
a gloo::Context, checks which algorithm code each constructor selected, and
checks the outputs of every pointer against the closed form of
gloo/test/base_test.h:184-236 (P = 2, k = 2, n = 1000; and P = 3, k = 3).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "oracle", "_ref", "hd_pipelined_test")


@pytest.mark.gpu
def test_bridge_pipelined_program_on_gpu():
    pytest.importorskip("torch")
    if not os.path.exists(PROGRAM):
        pytest.skip("oracle/_ref/hd_pipelined_test not built (needs the reference at build time)")
    r = subprocess.run([PROGRAM], capture_output=True, text=True, timeout=120)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and lines and all(l.startswith("ok") for l in lines), r.stdout[-3000:] + r.stderr[-2000:]
    assert len(lines) == 5, r.stdout
    assert any(l.startswith("ok   HalvingDoublingPipelined/P2/k2/n1000") for l in lines), r.stdout
