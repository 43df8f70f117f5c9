"""The public surface of the broadcast collective, without a GPU: the option
struct's layout against include/gloo_amd.h, the Python names, and a
syntax-only compile of the C++ front ends (the library-side classes of
hip_allreduce.h; the Gloo-side ones of gloo_bridge.h / gloo_collectives.h
where the reference's headers are present)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gloo_amd.h")).read()
CTYPES_OF = {"int": ctypes.c_int, "void*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32,
             "gloo_hip_stream_t": ctypes.c_void_p}


def header_fields():
    body = re.search(r"typedef struct \{([^}]*)\}\s*gloo_hip_broadcast_options_t;", HEADER).group(1)
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
    assert [n for n, _ in fields] == ["dtype", "input", "output", "elements", "root", "tag", "stream"]
    assert [n for n, _ in gloo_amd.BroadcastOptions._fields_] == [n for n, _ in fields]
    for (name, ctype), (_, py) in zip(fields, gloo_amd.BroadcastOptions._fields_):
        assert CTYPES_OF[ctype] is py, name

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, CTYPES_OF[t]) for n, t in fields]
    assert ctypes.sizeof(FromHeader) == ctypes.sizeof(gloo_amd.BroadcastOptions) == 48
    for n, _ in fields:
        assert getattr(FromHeader, n).offset == getattr(gloo_amd.BroadcastOptions, n).offset
    assert [getattr(FromHeader, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 36, 40]


def test_header_names_the_enum_the_function_and_the_unused_op():
    assert re.search(r"GLOO_HIP_ALGO_BROADCAST\s*=\s*12\b", HEADER)
    assert "int gloo_hip_broadcast(gloo_hip_context_t ctx, const gloo_hip_broadcast_options_t* opts);" in HEADER
    assert "NOT USED" in HEADER  # `op` of a broadcast


def test_python_names():
    import gloo_amd
    assert gloo_amd.ALGORITHMS["broadcast"] == 12
    assert "gloo_hip_broadcast" in gloo_amd.EXPORTED and "gloo_hip_fanout_kernel" in gloo_amd.EXPORTED
    assert hasattr(gloo_amd.lib, "gloo_hip_broadcast") and hasattr(gloo_amd.lib, "gloo_hip_fanout_kernel")
    import inspect
    sig = inspect.signature(gloo_amd.broadcast)
    assert list(sig.parameters) == ["ctx", "output", "elements", "dtype", "root", "input", "tag", "stream"]
    assert sig.parameters["input"].default is None and sig.parameters["tag"].default == 0
    alg = inspect.signature(gloo_amd.Algorithm.__init__).parameters
    assert alg["root"].default is None and alg["root_pointer"].default is None


def test_function_style_refuses_a_bad_root_without_a_gpu():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:bcast_abi")
    try:
        with pytest.raises(gloo_amd.GlooHipError) as e:
            gloo_amd.broadcast(ctx, 0x1000, 4, "f32", root=3)
        assert e.value.code == -4 and "root rank 3 " in str(e.value)
        gloo_amd.broadcast(ctx, 0x1000, 0, "f32", root=0)  # no elements: nothing to do
    finally:
        ctx.close()


LIB_TU = r"""
#include <cstdint>
#include "gloo_amd/hip_allreduce.h"
static_assert(GLOO_HIP_ALGO_BROADCAST == 12, "code");
void f(const std::shared_ptr<gloo_amd::Context>& c, float* a, float* b, hipStream_t s) {
  gloo_amd::HipBroadcastOneToAll<float> x(c, {a, b}, 16);
  gloo_amd::HipBroadcastOneToAll<float, gloo_amd::HipHostWorkspace<float>> y(c, {a, b}, 16, 1, 1, {s, s});
  x.run();
  y.run();
  gloo_amd::HipBroadcastOneToAll<gloo_amd::float8_e5m2> z(c, {reinterpret_cast<gloo_amd::float8_e5m2*>(a)}, 16, 0);
  gloo_amd::Algorithm* base = &z;
  base->run();
  gloo_amd::BroadcastOptions o(c);
  o.setInput(a, 16);
  o.setOutput(b, 16);
  o.setRoot(1);
  o.setTag(3);
  o.setStream(s);
  gloo_amd::broadcast(o);
}
"""

GLOO_TU = r"""
#include <cstdint>
#include "gloo_amd/gloo_collectives.h"
void f(const std::shared_ptr<gloo::Context>& c, float* a, float* b, hipStream_t s) {
  // the reference constructor's argument order (gloo/cuda_broadcast_one_to_all.h:20-27)
  gloo::HipBroadcastOneToAll<float> x(c, std::vector<float*>{a, b}, 16, 1, 1, std::vector<hipStream_t>{s, s});
  gloo::HipBroadcastOneToAll<int64_t, gloo::HipHostWorkspace<int64_t>> y(
      c, std::vector<int64_t*>{reinterpret_cast<int64_t*>(a)}, 2);
  gloo::Algorithm* base = &x;
  base->run();
  y.run();
  gloo::BroadcastOptions o(c);
  o.setInput(a, 16);
  o.setOutput(b, 16);
  o.setRoot(0);
  gloo::hip::broadcast(o);
  gloo::hip::broadcast(o, s);
}
"""


def compile_only(tmp_path, compiler, text, extra):
    src = tmp_path / "bcast_tu.cc"
    src.write_text(text)
    cmd = [compiler, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "gloo_amd", "include")] + extra + [str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cpp_library_side_compiles(tmp_path):
    """gloo_amd::HipBroadcastOneToAll<T> and gloo_amd::broadcast(BroadcastOptions)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: gloo_amd/hip_allreduce.h includes the HIP runtime API and needs it to compile")
    compile_only(tmp_path, hipcc, LIB_TU, ["--offload-arch=gfx950"])


def test_cpp_gloo_side_compiles(tmp_path):
    """gloo::HipBroadcastOneToAll<T> (a gloo::Algorithm) and gloo::hip::broadcast
    over the reference's own BroadcastOptions: compiled against the
    reference's headers, where they are present (as oracle/Makefile's REF)."""
    ref = os.environ.get("REF", "/root/reference")
    if not os.path.exists(os.path.join(ref, "gloo", "broadcast.h")):
        pytest.skip("the reference's headers are absent")
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs a C++ compiler and the HIP runtime API headers")
    compile_only(tmp_path, cxx, GLOO_TU, ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + ref, "-w"])
