"""csrc/options.hpp, the table behind cdfem_set_option, checked on its own.

tests/cpp/options_check.cpp is a stand-alone host program (the header needs no HIP): for every key, on a
default Options, the default, the accepted values stored in the right member, the nearest refused values
leaving it unchanged and returning exactly the refusal's text, and the refusal of an unknown and of a null
key, against expectations written out by hand.  It is built with g++ -Wall -Wextra -Werror, once plainly
and once with the address and undefined-behaviour sanitizers.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "continuum-mechanics-mfem_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_options_header(tmp_path, flags):
    src = os.path.join(ROOT, "tests", "cpp", "options_check.cpp")
    exe = str(tmp_path / "options_check")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, "-o", exe, src]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "options ok", r.stdout[-2000:] + r.stderr[-2000:]
