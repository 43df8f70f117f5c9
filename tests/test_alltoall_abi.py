"""The public surface of the alltoall collective, without a GPU: the options
struct's layout against include/gloo_amd.h, the two entry points, the Python
names, every refusal the C entries make before any exchange (on a one-rank
context, none needs a peer), the generic create's standing refusal of code 14,
and a syntax-only compile of the C++ front ends (the library-side functions of
hip_allreduce.h; the Gloo-side ones of gloo_collectives.h where the
reference's headers are present).  The C++ front ends are covered by
compilation only."""
import ctypes
import inspect
import os
import re
import shutil

import pytest

from test_gather_scatter_abi import compile_only, header_fields, reference_dir, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gloo_amd.h")).read()
NAMES = ["dtype", "input", "output", "elements", "in_counts", "out_counts", "matrix", "tag", "stream"]
CTYPES_OF = {"int": ctypes.c_int, "void*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32,
             "gloo_hip_stream_t": ctypes.c_void_p, "constsize_t*": ctypes.POINTER(ctypes.c_size_t)}


def test_struct_layout_matches_the_header():
    import gloo_amd
    fields = header_fields("gloo_hip_alltoall_options_t")
    assert [n for n, _ in fields] == NAMES
    assert [n for n, _ in gloo_amd.AlltoallOptions._fields_] == NAMES
    for (name, ctype), (_, pyt) in zip(fields, gloo_amd.AlltoallOptions._fields_):
        assert CTYPES_OF[ctype] is pyt, name
    offsets = [0, 8, 16, 24, 32, 40, 48, 56, 64]
    assert [getattr(gloo_amd.AlltoallOptions, n).offset for n in NAMES] == offsets
    assert ctypes.sizeof(gloo_amd.AlltoallOptions) == 72


def test_header_declares_the_entries():
    assert re.search(r"GLOO_HIP_ALGO_ALLTOALL\s*=\s*14\b", HEADER)
    assert "A PLAN ONLY" not in HEADER
    assert "int gloo_hip_alltoall(gloo_hip_context_t ctx, const gloo_hip_alltoall_options_t* opts);" in HEADER
    flat = re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", HEADER))
    assert ("int gloo_hip_alltoall_create(gloo_hip_context_t ctx, int dtype, void* input, void* output, size_t count, "
            "const int* matrix , gloo_hip_stream_t stream, int workspace, gloo_hip_algorithm_t* out);") in flat
    assert "int gloo_hip_alltoall_lists(int rank, int size, const int* matrix, int* lists);" in flat


def test_python_names():
    import gloo_amd
    assert "alltoall" not in gloo_amd.ALGORITHMS  # the generic Algorithm has no name for code 14
    for name in ("gloo_hip_alltoall", "gloo_hip_alltoall_create", "gloo_hip_alltoall_lists"):
        assert name in gloo_amd.EXPORTED and hasattr(gloo_amd.lib, name)
    sig = inspect.signature(gloo_amd.alltoall)
    assert list(sig.parameters) == ["ctx", "input", "output", "elements", "dtype", "in_counts", "out_counts", "matrix",
                                    "tag", "stream"]
    for name in ("in_counts", "out_counts", "matrix"):
        assert sig.parameters[name].default is None
    assert issubclass(gloo_amd.Alltoall, gloo_amd.Algorithm)


def test_nothing_to_move_returns_without_a_gpu():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:alltoall_abi_zero")
    try:
        gloo_amd.alltoall(ctx, 0, 0, 0, "f32")                                        # even, no elements, no buffers
        gloo_amd.alltoall(ctx, 0x1000, 0x2000, 0, "f32")
        gloo_amd.alltoall(ctx, 0x1000, 0x2000, 5, "u8", matrix=[[0]])                 # `elements` ignored
        gloo_amd.alltoall(ctx, 0, 0, 5, "u8", in_counts=[0], out_counts=[0])         # the exchange, then nothing
        gloo_amd.alltoall(ctx, 0x1000, 0x1000, 0, "u8", in_counts=[0], out_counts=[0], matrix=[0])
    finally:
        ctx.close()


def test_function_style_refusals_name_the_value():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:alltoall_abi_func")
    a2a = gloo_amd.alltoall
    try:
        assert "unknown dtype 99" in refused(a2a, ctx, 0x1000, 0x2000, 4, 99)
        assert "null input with 4 elements" in refused(a2a, ctx, 0, 0x2000, 4, "f32")
        assert "null output with 4 elements" in refused(a2a, ctx, 0x1000, 0, 4, "f32")
        assert "null input with 7 elements" in refused(a2a, ctx, 0, 0x2000, 0, "u8", matrix=[7])
        assert "null output with 3 elements" in refused(a2a, ctx, 0x1000, 0, 0, "u8", in_counts=[3], out_counts=[3])
        # 4 f32 at 0x1000 end at 0x1010: one shared byte is refused, none is not
        text = refused(a2a, ctx, 0x1000, 0x100f, 4, "f32")
        assert "overlap" in text and "0x1000" in text and "0x100f" in text and "+16" in text
        assert "overlap" in refused(a2a, ctx, 0x1000, 0x1000, 4, "f32")
        assert "overlap" in refused(a2a, ctx, 0x1008, 0x1000, 0, "u8", matrix=[9])
        assert "in_counts is given without out_counts" in refused(a2a, ctx, 0x1000, 0x2000, 0, "u8", in_counts=[3])
        assert "out_counts is given without in_counts" in refused(a2a, ctx, 0x1000, 0x2000, 0, "u8", out_counts=[3])
        big = 1 << 31
        assert f"in_count {big} for rank 0 is too large" in refused(a2a, ctx, 0x1000, 0x2000, 0, "u8", in_counts=[big],
                                                                   out_counts=[big])
        assert f"out_count {big} for rank 0 is too large" in refused(a2a, ctx, 0x1000, 0x2000, 0, "u8", in_counts=[3],
                                                                    out_counts=[big])
        assert f"count {big} from rank 0 to rank 0 is too large" in refused(a2a, ctx, 0x1000, 0x2000, 0, "u8",
                                                                           matrix=[big])
        assert "own block has in_count 3 but out_count 4" in refused(a2a, ctx, 0x1000, 0x2000, 0, "u8", in_counts=[3],
                                                                     out_counts=[4])
        assert "in_counts[0] is 4 but the matrix has 5 from rank 0 to rank 0" in refused(
            a2a, ctx, 0x1000, 0x2000, 0, "u8", in_counts=[4], out_counts=[4], matrix=[5])
        # the front end's own checks of what a C pointer cannot carry (its code is 1, not the library's -4)
        for kw, text in ((dict(in_counts=[1, 2], out_counts=[1]), "2 in_counts for 1 ranks"),
                         (dict(matrix=[[1, 2], [3, 4]]), "4 entries for 1 ranks"),
                         (dict(in_counts=[-2], out_counts=[1]), "negative in_count -2")):
            with pytest.raises(gloo_amd.GlooHipError) as e:
                a2a(ctx, 0x1000, 0x2000, 0, "u8", **kw)
            assert e.value.code == 1 and text in str(e.value)
    finally:
        ctx.close()


def test_algorithm_object_refusals_name_the_value():
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:alltoall_abi_algo")
    A = gloo_amd.Alltoall
    try:
        assert "unknown dtype 99" in refused(A, ctx, 99, 0x1000, 0x2000, count=4)
        assert "null input with 4 elements" in refused(A, ctx, "f32", 0, 0x2000, count=4)
        assert "null output with 6 elements" in refused(A, ctx, "u8", 0x1000, 0, matrix=[6])
        assert "overlap" in refused(A, ctx, "f64", 0x1000, 0x101f, count=4)
        vp, h = ctypes.c_void_p, ctypes.c_void_p()
        m = (ctypes.c_int * 1)(-3)
        rc = gloo_amd.lib.gloo_hip_alltoall_create(ctx._h, int(gloo_amd.DType.U8), vp(0x1000), vp(0x2000), 0, m, None, 0,
                                                   ctypes.byref(h))
        assert rc == -4 and b"negative count -3 from rank 0 to rank 0" in gloo_amd.lib.gloo_hip_last_error()
        rc = gloo_amd.lib.gloo_hip_alltoall_create(ctx._h, int(gloo_amd.DType.U8), vp(0x1000), vp(0x2000), 4, None, None,
                                                   0, None)
        assert rc == -4 and b"null argument" in gloo_amd.lib.gloo_hip_last_error()
    finally:
        ctx.close()


@pytest.mark.parametrize("algo", [14, 14 | 0x100])
def test_the_generic_create_still_calls_the_code_unknown(algo):
    import gloo_amd
    ctx = gloo_amd.Context(0, 1, "mem:alltoall_abi_generic")
    try:
        text = refused(gloo_amd.Algorithm, ctx, algo, "sum", "f32", [0x1000, 0x2000], 4)
        assert "unknown algorithm" in text and "gloo_hip_alltoall_create" in text
        text = refused(gloo_amd.Algorithm, ctx, algo, "sum", "f32", [0x1000, 0x2000], 4, streams=[1, 2])
        assert "unknown algorithm" in text
    finally:
        ctx.close()


def test_lists_entry_checks_its_arguments():
    import gloo_amd
    L = gloo_amd.lib.gloo_hip_alltoall_lists
    m, out = (ctypes.c_int * 4)(1, 2, 3, 4), (ctypes.c_int * 4)()
    assert L(1, 2, m, out) == 0 and list(out) == [3, 4, 2, 4]
    for args, text in (((0, 2, None, out), b"null"), ((0, 2, m, None), b"null"), ((2, 2, m, out), b"rank 2 outside"),
                       ((-1, 2, m, out), b"rank -1 outside"), ((0, 0, m, out), b"size 0"),
                       ((0, 1 << 20, m, out), b"out of range")):
        assert L(*args) == -4 and text in gloo_amd.lib.gloo_hip_last_error(), args


LIB_TU = r"""
#include <cstdint>
#include "gloo_amd/hip_allreduce.h"
static_assert(GLOO_HIP_ALGO_ALLTOALL == 14, "code");
void f(const std::shared_ptr<gloo_amd::Context>& c, float* in, float* out, hipStream_t s) {
  gloo_amd::AlltoallOptions a(c);
  a.setInput(in, 64);
  a.setOutput(out, 64);
  a.setTag(3);
  a.setStream(s);
  gloo_amd::alltoall(a);
  gloo_amd::AlltoallvOptions v(c);
  v.setInput(in, std::vector<size_t>{1, 0, 7});
  v.setOutput(out, std::vector<size_t>{1, 2, 3});
  v.setTag(4);
  v.setStream(s);
  gloo_amd::alltoallv(v);
  v.setMatrix(std::vector<int>{1, 0, 7, 2, 0, 0, 3, 0, 0});
  gloo_amd::alltoallv(v);
  gloo_hip_alltoall_options_t o{};
  o.matrix = nullptr;
  (void)o;
  int lists[6];
  (void)gloo_hip_alltoall_lists(0, 3, v.matrix_.data(), lists);
}
"""

GLOO_TU = r"""
#include <cstdint>
#include "gloo_amd/gloo_collectives.h"
void f(const std::shared_ptr<gloo::Context>& c, float* in, float* out, hipStream_t s) {
  gloo::AlltoallOptions a(c);
  a.setInput(in, 64);
  a.setOutput(out, 64);
  a.setTag(3);
  gloo::hip::alltoall(a);
  gloo::hip::alltoall(a, s);
  gloo::AlltoallvOptions v(c);
  v.setInput(in, std::vector<int64_t>{1, 0, 7});
  v.setOutput(out, std::vector<int64_t>{1, 2, 3});
  gloo::hip::alltoallv(v);
  gloo::hip::alltoallv(v, s);
}
"""


def test_cpp_library_side_compiles(tmp_path):
    """gloo_amd::alltoall and alltoallv over AlltoallOptions / AlltoallvOptions (compiled, not run)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: gloo_amd/hip_allreduce.h includes the HIP runtime API and needs it to compile")
    compile_only(tmp_path, hipcc, LIB_TU, ["--offload-arch=gfx950"])


def test_cpp_gloo_side_compiles(tmp_path):
    """gloo::hip::alltoall / alltoallv over the reference's own option classes:
    compiled against the reference's headers, where they are present (not run)."""
    ref = reference_dir()
    if not os.path.exists(os.path.join(ref, "gloo", "alltoallv.h")):
        pytest.skip("the reference's headers are absent")
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs a C++ compiler and the HIP runtime API headers")
    compile_only(tmp_path, cxx, GLOO_TU, ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + ref, "-w"])
