"""Whether two processes on this system can share device memory of any size
(TEST INFRASTRUCTURE).  Two small rank processes on the system HIP runtime
make a context and let it try a dma-buf import between them
(Context.agree_on_sharing, gloo_amd/include/gloo_amd/ipc.h): where the
runtime refuses it, memory is shared through hipIpc handles, which cannot
open 2 GiB or more.  Asked once per test session."""
import functools
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["GLOO_AMD_ROOT"])
sys.path.insert(0, os.path.join(os.environ["GLOO_AMD_ROOT"], "tests"))
import gloo_amd, hip_rt
hip_rt.set_device(0)
ctx = gloo_amd.Context(int(sys.argv[1]), 2, sys.argv[2], device=0, timeout_ms=20000)
print("ANYSIZE", int(ctx.agree_on_sharing()), flush=True)
ctx.close()
"""


@functools.lru_cache(maxsize=None)
def processes_share_any_size():
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.py")
        open(w, "w").write(WORKER)
        env = dict(os.environ, GLOO_AMD_ROOT=ROOT)
        procs = [subprocess.Popen([sys.executable, w, str(r), "file:" + os.path.join(d, "s")], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
        outs = [p.communicate(timeout=60) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(e[-2000:] for _, e in outs)
    answers = {o.split("ANYSIZE", 1)[1].split()[0] for o, _ in outs}
    assert len(answers) == 1, outs
    return answers == {"1"}
