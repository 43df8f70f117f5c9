"""CPU: the public surface of gloo_hip_quantise_mx_sr and gloo_hip_reduce_mx_sr: their twins' refusals under their own
names, before any GPU call (dummy non-null addresses stand for the buffers)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST, DSC, SRC, SSC = 0x100000, 0x200000, 0x300000, 0x400000
DTYPE, PTR, ARG = -2, -3, -4
LIB_TU = r"""
#include "gloo_amd/hip_allreduce.h"
void f(void* e, uint8_t* s, float* w, uint64_t seed, hipStream_t st) {
  gloo_amd::quantiseMx(GLOO_HIP_MXFP4_E2M1, GLOO_HIP_F32, {e, s}, w, 7, seed, st);
  gloo_amd::reduceMx(GLOO_HIP_MXFP8_E5M2, {e, s}, {{e, s}, {e, s}}, 7, seed, st);
}
"""


def test_exported_and_bound():
    import gloo_amd
    for name in ("gloo_hip_quantise_mx_sr", "gloo_hip_reduce_mx_sr"):
        assert name in gloo_amd.EXPORTED and hasattr(gloo_amd.lib, name)
    for fmt in range(3):  # nothing to do: no pointer is looked at
        assert gloo_amd.lib.gloo_hip_quantise_mx_sr(fmt, 8, None, None, None, 0, 1, None) == 0
        assert gloo_amd.lib.gloo_hip_reduce_mx_sr(fmt, None, None, None, None, 8, 0, 1, None) == 0


@pytest.mark.parametrize("call,code,word", [
    (lambda g: g.quantise_mx_ptr(3, "f32", DST, DSC, SRC, 4, seed=5), DTYPE, "quantise_mx_sr: unknown MX format 3"),
    (lambda g: g.quantise_mx_ptr(0, "f32", 0, DSC, SRC, 4, seed=5), PTR, "quantise_mx_sr: dst_elems is null"),
    (lambda g: g.quantise_mx_ptr(0, "f32", DST, DSC, DST, 4, seed=5), ARG, "quantise_mx_sr: dst_elems 0x100000 overlaps src"),
    (lambda g: g.reduce_mx_ptr(3, DST, DSC, [SRC], [SSC], 4, seed=5), DTYPE, "reduce_mx_sr: unknown MX format 3"),
    (lambda g: g.reduce_mx_ptr(0, DST, DSC, [SRC] * 9, [SSC] * 9, 4, seed=5), ARG, "reduce_mx_sr: source count 9"),
    (lambda g: g.reduce_mx_ptr(0, 0, DSC, [SRC], [SSC], 4, seed=2 ** 64 - 1), PTR, "reduce_mx_sr: dst_elems is null"),
    (lambda g: g.reduce_mx_ptr(0, DST, DSC, [DST + 16], [SSC], 4, seed=5), ARG,  # in place is the same address only
     "reduce_mx_sr: dst_elems 0x100000 overlaps src_elems[0]"),
])
def test_refusals(call, code, word):
    import gloo_amd
    with pytest.raises(gloo_amd.GlooHipError) as e:
        call(gloo_amd)
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_cpp_seed_forms_compile(tmp_path):
    (tmp_path / "mx_sr_tu.cc").write_text(LIB_TU)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gloo_amd", "include"), str(tmp_path / "mx_sr_tu.cc")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
