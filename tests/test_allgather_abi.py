"""The public surface of the allgather collective, without a GPU: the option
struct's layout against include/gloo_amd.h, the Python names, the refusals
that need no peer, and a syntax-only compile of the C++ front ends (the
library-side classes of hip_allreduce.h; the Gloo-side ones of gloo_bridge.h /
gloo_collectives.h where the reference's headers are present)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gloo_amd.h")).read()
CTYPES_OF = {"int": ctypes.c_int, "void*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32,
             "gloo_hip_stream_t": ctypes.c_void_p, "constsize_t*": ctypes.POINTER(ctypes.c_size_t)}


def header_fields():
    body = re.search(r"typedef struct \{([^}]*)\}\s*gloo_hip_allgather_options_t;", HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(.+?)\s*(\w+)", decl)
            out.append((m.group(2), m.group(1).replace(" ", "")))
    return out


def test_struct_layout_matches_the_header():
    import gloo_amd
    fields = header_fields()
    assert [n for n, _ in fields] == ["dtype", "input", "output", "elements", "counts", "tag", "stream"]
    assert [n for n, _ in gloo_amd.AllgatherOptions._fields_] == [n for n, _ in fields]
    for (name, ctype), (_, py) in zip(fields, gloo_amd.AllgatherOptions._fields_):
        assert CTYPES_OF[ctype] is py, name

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, CTYPES_OF[t]) for n, t in fields]
    assert ctypes.sizeof(FromHeader) == ctypes.sizeof(gloo_amd.AllgatherOptions) == 56
    assert [getattr(FromHeader, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 40, 48]
    assert [getattr(gloo_amd.AllgatherOptions, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 40, 48]


def test_header_names_the_enum_the_step_and_the_functions():
    assert re.search(r"GLOO_HIP_ALGO_ALLGATHER\s*=\s*13\b", HEADER)
    assert re.search(r"GLOO_HIP_STEP_LOCAL_GATHER\s*=\s*12\b", HEADER)
    assert "int gloo_hip_allgather(gloo_hip_context_t ctx, const gloo_hip_allgather_options_t* opts);" in HEADER
    assert "int gloo_hip_gather_fanout_kernel(void* const* dsts, int n, const void* const* srcs, int k, size_t bytes," \
        in HEADER


def test_python_names():
    import gloo_amd
    assert gloo_amd.ALGORITHMS["allgather"] == 13
    for name in ("gloo_hip_allgather", "gloo_hip_gather_fanout_kernel"):
        assert name in gloo_amd.EXPORTED and hasattr(gloo_amd.lib, name)
    sig = inspect.signature(gloo_amd.allgather)
    assert list(sig.parameters) == ["ctx", "output", "elements", "dtype", "input", "counts", "tag", "stream"]
    assert sig.parameters["input"].default is None and sig.parameters["counts"].default is None
    assert list(inspect.signature(gloo_amd.gather_fanout_kernel).parameters) == \
        ["dsts", "srcs", "nbytes", "blocks", "stream"]


def test_nothing_to_gather_and_bad_arguments_without_a_gpu():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:allgather_abi")
    try:
        gloo_amd.allgather(ctx, 0x1000, 0, "f32")                  # no elements: nothing to do
        gloo_amd.allgather(ctx, 0x1000, 5, "f32", counts=[0])      # `elements` ignored, counts all zero
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.allgather(ctx, 0x1000, 4, 99)
        assert e.value.code == -4 and "dtype" in str(e.value)
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.allgather(ctx, 0, 4, "f32")
        assert e.value.code == -4 and "null output" in str(e.value)
        with pytest.raises(gloo_amd.GlooHipError) as e:            # the mesh flag, before any exchange
            gloo_amd.Algorithm(ctx, 13 | 0x100, "bxor", "f32", [0x1000, 0x2000], 4)
        assert e.value.code == -4 and str(13 | 0x100) in str(e.value)
    finally:
        ctx.close()


LIB_TU = r"""
#include <cstdint>
#include "gloo_amd/hip_allreduce.h"
static_assert(GLOO_HIP_ALGO_ALLGATHER == 13, "code");
static_assert(GLOO_HIP_STEP_LOCAL_GATHER == 12, "step");
void f(const std::shared_ptr<gloo_amd::Context>& c, const float* a, const float* b, float* out, hipStream_t s) {
  gloo_amd::HipAllgatherRing<float> x(c, {a, b}, out, 16);
  gloo_amd::HipAllgatherRing<float, gloo_amd::HipHostWorkspace<float>> y(c, {a}, out, 16, {s, s});
  x.run();
  y.run();
  gloo_amd::HipAllgatherRing<gloo_amd::float8_e5m2> z(c, {reinterpret_cast<const gloo_amd::float8_e5m2*>(a)},
                                                      reinterpret_cast<gloo_amd::float8_e5m2*>(out), 16, {s});
  gloo_amd::Algorithm* base = &z;
  base->run();
  gloo_amd::AllgatherOptions o(c);
  o.setInput(const_cast<float*>(a), 16);
  o.setOutput(out, 64);
  o.setTag(3);
  o.setStream(s);
  gloo_amd::allgather(o);
  gloo_amd::AllgathervOptions v(c);
  v.setOutput(out, std::vector<size_t>{1, 0, 7});
  gloo_amd::allgatherv(v);
}
"""

GLOO_TU = r"""
#include <cstdint>
#include "gloo_amd/gloo_collectives.h"
void f(const std::shared_ptr<gloo::Context>& c, const float* a, const float* b, float* out, hipStream_t s) {
  // the reference constructor's argument order (gloo/allgather_ring.h:28-32)
  gloo::HipAllgatherRing<float> x(c, std::vector<const float*>{a, b}, out, 16);
  gloo::HipAllgatherRing<int64_t, gloo::HipHostWorkspace<int64_t>> y(
      c, std::vector<const int64_t*>{reinterpret_cast<const int64_t*>(a)}, reinterpret_cast<int64_t*>(out), 2,
      std::vector<hipStream_t>{s, s});
  gloo::Algorithm* base = &x;
  base->run();
  y.run();
  gloo::AllgatherOptions o(c);
  o.setInput(const_cast<float*>(a), 16);
  o.setOutput(out, 64);
  gloo::hip::allgather(o);
  gloo::hip::allgather(o, s);
  gloo::AllgathervOptions v(c);
  v.setInput(const_cast<float*>(a), 1);
  v.setOutput(out, std::vector<size_t>{1, 0, 7});
  gloo::hip::allgatherv(v);
  gloo::hip::allgatherv(v, s);
}
"""


def compile_only(tmp_path, compiler, text, extra):
    src = tmp_path / "allgather_tu.cc"
    src.write_text(text)
    cmd = [compiler, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "gloo_amd", "include")] + extra + [str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cpp_library_side_compiles(tmp_path):
    """gloo_amd::HipAllgatherRing<T>, gloo_amd::allgather and allgatherv."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: gloo_amd/hip_allreduce.h includes the HIP runtime API and needs it to compile")
    compile_only(tmp_path, hipcc, LIB_TU, ["--offload-arch=gfx950"])


def test_cpp_gloo_side_compiles(tmp_path):
    """gloo::HipAllgatherRing<T> (a gloo::Algorithm) and gloo::hip::allgather /
    allgatherv over the reference's own option structs: compiled against the
    reference's headers, where they are present (as oracle/Makefile's REF)."""
    ref = os.environ.get("REF", "/root/reference")
    if not os.path.exists(os.path.join(ref, "gloo", "allgatherv.h")):
        pytest.skip("the reference's headers are absent")
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs a C++ compiler and the HIP runtime API headers")
    compile_only(tmp_path, cxx, GLOO_TU, ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + ref, "-w"])
