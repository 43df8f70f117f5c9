"""The public surface of the gather and scatter collectives, without a GPU: the
option structs' layouts against include/gloo_amd.h, the enum values and the
input-index encoding, the Python names, every refusal of the C entry points
(none needs a peer), and a syntax-only compile of the C++ front ends (the
library-side functions of hip_allreduce.h; the Gloo-side ones of
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
             "gloo_hip_stream_t": ctypes.c_void_p, "constsize_t*": ctypes.POINTER(ctypes.c_size_t),
             "void*const*": ctypes.POINTER(ctypes.c_void_p)}


def header_fields(struct):
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct + ";", HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(.+?)\s*(\w+)", decl)
            out.append((m.group(2), m.group(1).replace(" ", "")))
    return out


@pytest.mark.parametrize("struct, py, names, offsets, size", [
    ("gloo_hip_gather_options_t", "GatherOptions",
     ["dtype", "root", "input", "output", "elements", "counts", "tag", "stream"], [0, 4, 8, 16, 24, 32, 40, 48], 56),
    ("gloo_hip_scatter_options_t", "ScatterOptions",
     ["dtype", "root", "output", "inputs", "elements", "tag", "stream"], [0, 4, 8, 16, 24, 32, 40], 48),
])
def test_struct_layouts_match_the_header(struct, py, names, offsets, size):
    import gloo_amd
    cls = getattr(gloo_amd, py)
    fields = header_fields(struct)
    assert [n for n, _ in fields] == names
    assert [n for n, _ in cls._fields_] == names
    for (name, ctype), (_, pyt) in zip(fields, cls._fields_):
        assert CTYPES_OF[ctype] is pyt, name

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, CTYPES_OF[t]) for n, t in fields]
    assert ctypes.sizeof(FromHeader) == ctypes.sizeof(cls) == size
    assert [getattr(FromHeader, n).offset for n in names] == offsets
    assert [getattr(cls, n).offset for n in names] == offsets


def test_header_names_the_enums_the_encoding_and_the_functions():
    assert re.search(r"GLOO_HIP_ALGO_GATHER\s*=\s*15\b", HEADER)
    assert re.search(r"GLOO_HIP_ALGO_SCATTER\s*=\s*16\b", HEADER)
    assert re.search(r"GLOO_HIP_ALGO_ALLTOALL\s*=\s*14\b", HEADER)  # untouched
    assert re.search(r"#define GLOO_HIP_FROM_INPUTS 4\b", HEADER)   # input 0 keeps its encoding
    assert re.search(r"#define GLOO_HIP_INPUT_SHIFT 8\b", HEADER)
    assert "#define GLOO_HIP_INPUT(q)" in HEADER and "#define GLOO_HIP_INPUT_OF(flags)" in HEADER
    assert "#define GLOO_HIP_COUNT_PER_RANK ((size_t)-1)" in HEADER
    assert "int gloo_hip_gather(gloo_hip_context_t ctx, const gloo_hip_gather_options_t* opts);" in HEADER
    assert "int gloo_hip_scatter(gloo_hip_context_t ctx, const gloo_hip_scatter_options_t* opts);" in HEADER


def test_python_names():
    import gloo_amd
    assert gloo_amd.ALGORITHMS["gather"] == 15 and gloo_amd.ALGORITHMS["scatter"] == 16
    assert gloo_amd.COUNT_PER_RANK == (1 << 64) - 1
    for name in ("gloo_hip_gather", "gloo_hip_scatter"):
        assert name in gloo_amd.EXPORTED and hasattr(gloo_amd.lib, name)
    sig = inspect.signature(gloo_amd.gather)
    assert list(sig.parameters) == ["ctx", "input", "elements", "dtype", "root", "output", "counts", "tag", "stream"]
    assert sig.parameters["output"].default is None and sig.parameters["counts"].default is None
    sig = inspect.signature(gloo_amd.scatter)
    assert list(sig.parameters) == ["ctx", "output", "elements", "dtype", "root", "inputs", "tag", "stream"]
    assert sig.parameters["inputs"].default is None


def refused(fn, *a, **kw):
    import gloo_amd
    with pytest.raises(gloo_amd.GlooHipError) as e:
        fn(*a, **kw)
    assert e.value.code == -4, str(e.value)
    return str(e.value)


def test_gather_refusals_and_nothing_to_gather_without_a_gpu():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:gather_abi")
    try:
        gloo_amd.gather(ctx, 0x1000, 0, "f32", 0, output=0x2000)               # no elements: nothing to do
        gloo_amd.gather(ctx, 0x1000, 5, "f32", 0, output=0x2000, counts=[0])   # `elements` ignored, counts all zero
        assert "dtype" in refused(gloo_amd.gather, ctx, 0x1000, 4, 99, 0, output=0x2000)
        assert "root rank 1 outside [0, 1)" in refused(gloo_amd.gather, ctx, 0x1000, 4, "f32", 1, output=0x2000)
        assert "root rank -1" in refused(gloo_amd.gather, ctx, 0x1000, 4, "f32", -1, output=0x2000)
        assert "null input" in refused(gloo_amd.gather, ctx, 0, 4, "f32", 0, output=0x2000)
        assert "null output on the root" in refused(gloo_amd.gather, ctx, 0x1000, 4, "f32", 0)
        assert "too large" in refused(gloo_amd.gather, ctx, 0x1000, 0, "u8", 0, output=0x2000, counts=[1 << 31])
        # the algorithm entry points: the mesh flag, a root, a negative count, NULL recv_elems, the pointer count
        A = gloo_amd.Algorithm
        assert str(15 | 0x100) in refused(A, ctx, 15 | 0x100, "bxor", "f32", [0x1000, 0x2000], 4, recv_elems=[0])
        assert "root rank 3" in refused(A, ctx, "gather", "sum", "f32", [0x1000, 0x2000], 4, recv_elems=[3])
        assert "negative count -7" in refused(A, ctx, "gather", "sum", "f32", [0x1000, 0x2000], 0, recv_elems=[0, -7])
        assert "not 1 pointers" in refused(A, ctx, "gather", "sum", "f32", [0x1000], 4, recv_elems=[0])
        assert "not 3 pointers" in refused(A, ctx, "gather", "sum", "f32", [0x1000, 0x2000, 0x3000], 4, recv_elems=[0])
        assert "one stream" in refused(A, ctx, "gather", "sum", "f32", [0x1000, 0x2000], 4, recv_elems=[0],
                                       streams=[1, 2])
        vp = ctypes.c_void_p
        arr, h = (vp * 2)(0x1000, 0x2000), vp()
        rc = gloo_amd.lib.gloo_hip_algorithm_create_ws(ctx._h, 15, 0, int(gloo_amd.DType.F32), arr, 2, 4, None, None, 0,
                                                       ctypes.byref(h))
        assert rc == -4 and b"recv_elems is NULL" in gloo_amd.lib.gloo_hip_last_error()
    finally:
        ctx.close()


def test_scatter_refusals_and_nothing_to_scatter_without_a_gpu():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:scatter_abi")
    try:
        gloo_amd.scatter(ctx, 0x1000, 0, "f32", 0, inputs=[0x2000])            # no elements: nothing to do
        assert "dtype" in refused(gloo_amd.scatter, ctx, 0x1000, 4, 99, 0, inputs=[0x2000])
        assert "root rank 1 outside [0, 1)" in refused(gloo_amd.scatter, ctx, 0x1000, 4, "f32", 1, inputs=[0x2000])
        assert "null output" in refused(gloo_amd.scatter, ctx, 0, 4, "f32", 0, inputs=[0x2000])
        assert "the root has no inputs" in refused(gloo_amd.scatter, ctx, 0x1000, 4, "f32", 0)
        assert "null input for rank 0" in refused(gloo_amd.scatter, ctx, 0x1000, 4, "f32", 0, inputs=[0])
        A = gloo_amd.Algorithm
        assert str(16 | 0x100) in refused(A, ctx, 16 | 0x100, "bxor", "f32", [0x1000, 0x2000], 4, recv_elems=[0])
        assert "root rank 2" in refused(A, ctx, "scatter", "sum", "f32", [0x1000, 0x2000], 4, recv_elems=[2])
        assert "not 1 pointers" in refused(A, ctx, "scatter", "sum", "f32", [0x1000], 4, recv_elems=[0])
        vp = ctypes.c_void_p
        arr, h = (vp * 2)(0x1000, 0x2000), vp()
        rc = gloo_amd.lib.gloo_hip_algorithm_create_ws(ctx._h, 16, 0, int(gloo_amd.DType.F32), arr, 2, 4, None, None, 0,
                                                       ctypes.byref(h))
        assert rc == -4 and b"recv_elems is NULL" in gloo_amd.lib.gloo_hip_last_error()
    finally:
        ctx.close()


def test_the_alltoall_code_is_still_refused_by_the_executor():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:rooted_abi_a2a")
    try:
        assert "unknown algorithm" in refused(gloo_amd.Algorithm, ctx, 14, "sum", "f32", [0x1000], 4)
    finally:
        ctx.close()


LIB_TU = r"""
#include <cstdint>
#include "gloo_amd/hip_allreduce.h"
static_assert(GLOO_HIP_ALGO_GATHER == 15 && GLOO_HIP_ALGO_SCATTER == 16, "codes");
static_assert(GLOO_HIP_INPUT_OF(GLOO_HIP_FROM_INPUTS | GLOO_HIP_INPUT(7)) == 7, "input index");
static_assert((GLOO_HIP_FROM_INPUTS | GLOO_HIP_INPUT(0)) == GLOO_HIP_FROM_INPUTS, "input 0 keeps its encoding");
void f(const std::shared_ptr<gloo_amd::Context>& c, float* a, float* b, float* out, hipStream_t s) {
  gloo_amd::GatherOptions g(c);
  g.setInput(a, 16);
  g.setOutput(out, 64);
  g.setRoot(1);
  g.setTag(3);
  g.setStream(s);
  gloo_amd::gather(g);
  gloo_amd::GathervOptions v(c);
  v.setInput(a, 1);
  v.setOutput(out, std::vector<size_t>{1, 0, 7});
  v.setRoot(0);
  gloo_amd::gatherv(v);
  gloo_amd::GathervOptions w(c);  // a rank without an output
  w.setInput(a, 7);
  w.setCounts({1, 0, 7});
  w.setRoot(0);
  gloo_amd::gatherv(w);
  gloo_amd::ScatterOptions t(c);
  t.setInputs(std::vector<float*>{a, b}, 16);
  t.setOutput(out, 16);
  t.setRoot(0);
  t.setTag(4);
  t.setStream(s);
  gloo_amd::scatter(t);
}
"""

GLOO_TU = r"""
#include <cstdint>
#include "gloo_amd/gloo_collectives.h"
void f(const std::shared_ptr<gloo::Context>& c, float* a, float* b, float* out, hipStream_t s) {
  gloo::GatherOptions g(c);
  g.setInput(a, 16);
  g.setOutput(out, 64);
  g.setRoot(1);
  gloo::hip::gather(g);
  gloo::hip::gather(g, s);
  gloo::GathervOptions v(c);
  v.setInput(a, 1);
  v.setOutput(out, std::vector<size_t>{1, 0, 7});
  v.setRoot(0);
  gloo::hip::gatherv(v);
  gloo::hip::gatherv(v, s);
  gloo::ScatterOptions t(c);
  t.setInputs(std::vector<float*>{a, b}, 16);
  t.setOutput(out, 16);
  t.setRoot(0);
  gloo::hip::scatter(t);
  gloo::hip::scatter(t, s);
}
"""


def compile_only(tmp_path, compiler, text, extra):
    src = tmp_path / "gather_scatter_tu.cc"
    src.write_text(text)
    cmd = [compiler, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "gloo_amd", "include")] + extra + [str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cpp_library_side_compiles(tmp_path):
    """gloo_amd::gather, gatherv and scatter."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: gloo_amd/hip_allreduce.h includes the HIP runtime API and needs it to compile")
    compile_only(tmp_path, hipcc, LIB_TU, ["--offload-arch=gfx950"])


def reference_dir():
    """Where the reference's headers are: $REF, else oracle/Makefile's default."""
    ref = os.environ.get("REF")
    if not ref:
        m = re.search(r"^REF \?= (\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), flags=re.M)
        ref = m.group(1) if m else ""
    return ref


def test_cpp_gloo_side_compiles(tmp_path):
    """gloo::hip::gather / gatherv / scatter over the reference's own option
    classes: compiled against the reference's headers, where they are present."""
    ref = reference_dir()
    if not os.path.exists(os.path.join(ref, "gloo", "gatherv.h")):
        pytest.skip("the reference's headers are absent")
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs a C++ compiler and the HIP runtime API headers")
    compile_only(tmp_path, cxx, GLOO_TU, ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + ref, "-w"])
