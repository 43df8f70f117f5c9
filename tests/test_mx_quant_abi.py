"""CPU: the public surface of gloo_hip_quantise_mx and gloo_hip_reduce_mx_wide: every refusal comes before any GPU
call, with its status and a last-error text that names the value (dummy non-null addresses stand for the buffers)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST, DSC, SRC, SSC = 0x100000, 0x200000, 0x300000, 0x400000  # 64 KiB apart per source below
DTYPE, PTR, ARG = -2, -3, -4
F32, I32 = 8, 2


def quantise(fmt=0, dtype=F32, dst=DST, dsc=DSC, src=SRC, nblocks=4):
    import gloo_amd
    gloo_amd.quantise_mx_ptr(fmt, dtype, dst, dsc, src, nblocks)


def fold(fmt=0, dtype=F32, dst=DST, k=2, nblocks=4, **kw):
    import gloo_amd
    src = kw.get("src", [SRC + 0x10000 * j for j in range(k)])
    ssc = kw.get("ssc", [SSC + 0x10000 * j for j in range(k)])
    gloo_amd.reduce_mx_wide_ptr(fmt, dtype, dst, src, ssc, nblocks)


@pytest.mark.parametrize("call,code,word,kw", [
    (quantise, DTYPE, "format 3", dict(fmt=3)),
    (quantise, DTYPE, "dtype 2", dict(dtype=I32, nblocks=0)),            # before the length is looked at
    (quantise, PTR, "dst_elems is null", dict(dst=0)),
    (quantise, PTR, "dst_scales is null", dict(dsc=0)),
    (quantise, PTR, "src is null", dict(src=0)),
    (quantise, PTR, "src 0x300008", dict(src=SRC + 8)),
    (quantise, PTR, "dst_elems 0x100004", dict(dst=DST + 4)),
    (quantise, ARG, "dst_elems 0x100000 overlaps src", dict(src=DST)),   # no in-place form
    (quantise, ARG, "dst_elems 0x100000 overlaps src", dict(src=DST - 496)),
    (quantise, ARG, "dst_scales 0x3001ff overlaps src", dict(dsc=SRC + 511)),
    (quantise, ARG, "overlaps dst_scales", dict(dsc=DST + 127)),
    (fold, DTYPE, "format 3", dict(fmt=3)),
    (fold, DTYPE, "dtype 2", dict(dtype=I32)),
    (fold, ARG, "count 0", dict(k=0)),
    (fold, ARG, "count 9", dict(k=9, nblocks=0)),
    (fold, PTR, "dst is null", dict(dst=0)),
    (fold, PTR, "src_elems[1] is null", dict(src=[SRC, 0])),
    (fold, PTR, "src_scales[0] is null", dict(ssc=[0, SSC])),
    (fold, PTR, "dst 0x100008", dict(dst=DST + 8)),
    (fold, PTR, "src_elems[1] 0x300004", dict(src=[SRC + 0x10000, SRC + 4])),
    (fold, ARG, "overlaps src_elems[0]", dict(src=[DST, SRC])),          # no in-place form either
    (fold, ARG, "overlaps src_elems[1]", dict(src=[SRC, DST + 496])),
    (fold, ARG, "overlaps src_scales[1]", dict(ssc=[SSC, DST + 511])),
])
def test_refusals(call, code, word, kw):
    import gloo_amd
    with pytest.raises(gloo_amd.GlooHipError) as e:
        call(**kw)
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_the_empty_call_and_the_tile_queries():
    import gloo_amd
    for fmt in range(3):  # nothing to do: no pointer is looked at
        for dtype in (6, 7, F32):
            assert gloo_amd.lib.gloo_hip_quantise_mx(fmt, dtype, None, None, None, 0, None) == 0
            assert gloo_amd.lib.gloo_hip_reduce_mx_wide(fmt, dtype, None, None, None, 8, 0, None) == 0
            assert gloo_amd.mx_quantise_tile_blocks(fmt, dtype) > 0 and gloo_amd.mx_wide_tile_blocks(fmt, dtype) > 0
    for query in (gloo_amd.mx_quantise_tile_blocks, gloo_amd.mx_wide_tile_blocks):
        assert query(3, "f32") == 0 and query(0, "i32") == 0 and query(0, "f64") == 0


LIB_TU = r"""
#include "gloo_amd/hip_allreduce.h"
void f(void* e, uint8_t* s, float* w, hipStream_t st) {
  gloo_amd::quantiseMx(GLOO_HIP_MXFP4_E2M1, GLOO_HIP_F32, {e, s}, w, 7, st);
  gloo_amd::reduceMxWide(GLOO_HIP_MXFP8_E5M2, GLOO_HIP_BF16, w, {{e, s}, {e, s}}, 7, st);
  (void)gloo_hip_mx_quantise_tile_blocks(GLOO_HIP_MXFP8_E4M3, GLOO_HIP_F16);
  (void)gloo_hip_mx_wide_tile_blocks(GLOO_HIP_MXFP8_E4M3, GLOO_HIP_F16);
}
"""


def test_cpp_front_end_compiles(tmp_path):
    src = tmp_path / "mx_quant_tu.cc"
    src.write_text(LIB_TU)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "gloo_amd", "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
