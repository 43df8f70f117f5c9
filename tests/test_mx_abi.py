"""CPU: the public surface of the MX block-scaled sum (gloo_hip_reduce_mx):
every refusal comes before any GPU call, with its status and a last-error text
that names the value (dummy non-null addresses stand for the buffers)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST, DSC, SRC, SSC = 0x100000, 0x200000, 0x300000, 0x400000  # 64 KiB apart per source below
DTYPE, PTR, ARG = -2, -3, -4


def call(fmt=0, dst=DST, dsc=DSC, k=2, nblocks=4, **kw):
    import gloo_amd
    src = kw.get("src", [SRC + 0x10000 * j for j in range(k)])
    ssc = kw.get("ssc", [SSC + 0x10000 * j for j in range(k)])
    gloo_amd.reduce_mx_ptr(fmt, dst, dsc, src, ssc, nblocks)


@pytest.mark.parametrize("code,word,kw", [
    (DTYPE, "format 3", dict(fmt=3)),
    (ARG, "count 9", dict(k=9, nblocks=0)),                             # before the length is looked at
    (PTR, "dst_elems is null", dict(dst=0)),
    (PTR, "src_elems[1] is null", dict(src=[SRC, 0])),
    (PTR, "src_scales[0] is null", dict(ssc=[0, SSC])),
    (PTR, "dst_elems 0x100008", dict(dst=DST + 8)),
    (PTR, "src_elems[1] 0x300004", dict(src=[SRC + 0x10000, SRC + 4])),
    (ARG, "overlaps src_elems[1]", dict(src=[SRC, DST])),               # in place is source 0 only
    (ARG, "overlaps src_elems[0]", dict(src=[DST + 32, SRC])),          # ... and the same address
    (ARG, "overlaps src_scales[1]", dict(ssc=[SSC, DSC + 3])),
    (ARG, "overlaps dst_scales", dict(dsc=DST + 127)),
])
def test_refusals(code, word, kw):
    import gloo_amd
    with pytest.raises(gloo_amd.GlooHipError) as e:
        call(**kw)
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_supported_names_and_the_empty_call():
    import gloo_amd
    for fmt in range(3):  # nothing to do: no pointer is looked at
        assert gloo_amd.lib.gloo_hip_reduce_mx(fmt, None, None, None, None, 8, 0, None) == 0
    assert [gloo_amd.lib.gloo_hip_mx_supported(f) for f in (0, 1, 2, 3)] == [1, 1, 1, 0]
    assert gloo_amd.mx_supported("mxfp4_e2m1") and not gloo_amd.mx_supported(-1)
    assert [int(f) for f in gloo_amd.MXFormat] == [0, 1, 2] == sorted(int(v) for v in gloo_amd.MX_FORMAT_NAMES.values())
    assert all(t > 0 for t in gloo_amd.MX_TILE_BLOCKS.values()) and gloo_amd.lib.gloo_hip_mx_tile_blocks(3) == 0


LIB_TU = r"""
#include "gloo_amd/hip_allreduce.h"
static_assert(GLOO_HIP_MXFP8_E4M3 == 0 && GLOO_HIP_MXFP8_E5M2 == 1 && GLOO_HIP_MXFP4_E2M1 == 2, "codes");
void f(void* e, uint8_t* s, hipStream_t st) {
  gloo_amd::reduceMx(GLOO_HIP_MXFP4_E2M1, {e, s}, {{e, s}, {e, s}}, 7, st);
  (void)gloo_hip_mx_supported(GLOO_HIP_MXFP8_E5M2);
}
"""


def test_cpp_front_end_compiles(tmp_path):
    src = tmp_path / "mx_tu.cc"
    src.write_text(LIB_TU)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gloo_amd", "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
