"""csrc/handles.hpp and csrc/ctx_state.hpp, the owning handles and the context's state by lifetime, on their own.

tests/cpp/ctx_state_check.cpp is a stand-alone host program (the headers need no HIP).  It defines the raw
device allocation over malloc / free with a count of live bytes, and checks DevBuf (alloc over a live buffer,
move construction and assignment, self-move, reset, assign from a vector, arrays of handles), PinBuf and Event
over counting stubs of their own, and that a filled
MeshState / PartitionState assigned from a default one holds no byte and has every scalar at the value the mesh
teardown used to write by hand.  It is built with g++ -Wall -Wextra -Werror, once plainly and once with the
address (leak detection on) and undefined-behaviour sanitizers.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "continuum-mechanics-mfem_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_ctx_state_headers(tmp_path, flags):
    src = os.path.join(ROOT, "tests", "cpp", "ctx_state_check.cpp")
    exe = str(tmp_path / "ctx_state_check")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, "-o", exe, src]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ctx state ok"), r.stdout[-2000:] + r.stderr[-2000:]
