"""csrc/krylov_host.hpp, the host side the GMRES and BiCGStab drivers share, checked on its own.

tests/cpp/krylov_host_check.cpp is a stand-alone host program (the header needs no HIP).  It drives LagPoll, the
lag-one host poll, over a fake in-order queue whose step i posts "done iff i >= s", for every poll interval
k = 1 .. 8 and stop step s = 0 .. 40, in the BiCGStab shape (a post every k-th step, four slots in turn) and the
GMRES shape (cycles of m = 1, 5, 7, 30 steps, a post forced on a cycle's last step, reset() at its end, then the
synchronous check on event 0): every wait is for the previous post's record and that event has not been recorded
again; the slot read is the previous post's, never the current one's, and nothing queued since writes it; the
loop leaves at the first post whose predecessor's step is >= s; the steps queued past s are q + k - s (q the
first polled step >= s), at most 2k - 1, and in a GMRES cycle never more than the cycle holds; post n since a
reset records event n & 1.  pick_ept is compared with a brute-force restatement for constant and per-EPT resident
counts, the 129^3 case of its comment included.  Built with g++ -Wall -Wextra -Werror, once plainly and once with
the address and undefined-behaviour sanitizers.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "continuum-mechanics-mfem_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_krylov_host_header(tmp_path, flags):
    src = os.path.join(ROOT, "tests", "cpp", "krylov_host_check.cpp")
    exe = str(tmp_path / "krylov_host_check")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, "-o", exe, src]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("krylov host ok"), r.stdout[-2000:] + r.stderr[-2000:]
