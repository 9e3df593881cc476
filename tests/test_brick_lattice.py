"""csrc/brick_lattice.hpp, the index rules of the brick lattice, checked on their own.

tests/cpp/brick_lattice_check.cpp is a stand-alone host program (the header needs no HIP): brick_holders, the
1-8 (brick, patch position) pairs that hold a lattice dof, against a brute-force list in the fixed summation
order (lower brick first per axis, z outermost) for every dof of full and cut lattices of the patch sides in
use, and xcd_order as a permutation that gives every XCD a contiguous range.  It is built with g++ -Wall
-Wextra -Werror, once plainly and once with the address and undefined-behaviour sanitizers.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "continuum-mechanics-mfem_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_brick_lattice_header(tmp_path, flags):
    src = os.path.join(ROOT, "tests", "cpp", "brick_lattice_check.cpp")
    exe = str(tmp_path / "brick_lattice_check")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, "-o", exe, src]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("brick lattice ok"), r.stdout[-2000:] + r.stderr[-2000:]
