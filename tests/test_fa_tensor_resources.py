"""Compile-time resources of the tensor full-assembly element kernel (csrc/fa_tensor.hip k_tensor_elem<DIM, P>),
from the compiler's own remarks (tools/resource_usage.sh; no GPU): the six spaces (quads p = 1..4, hexes
p = 1, 2), none of them with scratch, each within the LDS of a CU and resident at least once per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not found")
def test_fa_tensor_resources():
    cmd = ["bash", os.path.join(ROOT, "tools", "resource_usage.sh"), "csrc/fa_tensor.hip", "k_tensor_elem"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0
    print(p.stdout)
    rows = {}
    for line in p.stdout.splitlines():
        name, vgpr, agpr, scratch, occ, lds = line.rsplit(" ", 5)
        m = re.search(r"k_tensor_elem<(\d+), (\d+)>", name) or re.search(r"k_tensor_elemILi(\d+)ELi(\d+)E", name)
        assert m, name
        rows[tuple(int(g) for g in m.groups())] = tuple(int(v) for v in (vgpr, agpr, scratch, occ, lds))
    assert sorted(rows) == [(2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2)]
    for key, (vgpr, agpr, scratch, occ, lds) in rows.items():
        assert scratch == 0, key          # no instantiation spills
        assert lds <= 65536 and occ >= 1, key
