"""Compile-time resources of the matrix-free nonlinear form's kernel (csrc/nl_tensor.hip k_nl_tensor<DIM, P, MODE>),
from the compiler's own remarks (tools/resource_usage.sh; no GPU): the five spaces (quads p = 1..3, hexes
p = 1, 2) in the three modes (residual, Jacobian action, diagonal), none of them with scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not found")
def test_nl_tensor_resources():
    cmd = ["bash", os.path.join(ROOT, "tools", "resource_usage.sh"), "csrc/nl_tensor.hip", "k_nl_tensor"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0
    print(p.stdout)
    rows = {}
    for line in p.stdout.splitlines():
        name, vgpr, agpr, scratch, occ, lds = line.rsplit(" ", 5)
        m = re.search(r"k_nl_tensor<(\d+), (\d+), (\d+)>", name) or re.search(r"k_nl_tensorILi(\d+)ELi(\d+)ELi(\d+)E", name)
        assert m, name
        rows[tuple(int(g) for g in m.groups())] = tuple(int(v) for v in (vgpr, agpr, scratch, occ, lds))
    spaces = [(2, 1), (2, 2), (2, 3), (3, 1), (3, 2)]
    assert sorted(rows) == sorted((d, q, mode) for d, q in spaces for mode in range(3))
    for key, (vgpr, agpr, scratch, occ, lds) in rows.items():
        assert scratch == 0, key          # no instantiation spills
        assert lds <= 65536 and occ >= 1, key
