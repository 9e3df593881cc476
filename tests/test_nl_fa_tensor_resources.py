"""Compile-time resources of the assembled tensor Jacobian's row kernel (csrc/nl_fa_tensor.hip
k_nl_tensor_elem<DIM, P>), from the compiler's own remarks (tools/resource_usage.sh; no GPU): the five spaces
(quads p = 1..3, hexes p = 1, 2), none of them with scratch, each within the LDS of a CU and resident at least
once per SIMD.  The point pass and the face kernel of the same file are held to the same."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SPACES = [(2, 1), (2, 2), (2, 3), (3, 1), (3, 2)]


def usage(kernel):
    cmd = ["bash", os.path.join(ROOT, "tools", "resource_usage.sh"), "csrc/nl_fa_tensor.hip", kernel]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0
    print(p.stdout)
    rows = {}
    for line in p.stdout.splitlines():
        name, vgpr, agpr, scratch, occ, lds = line.rsplit(" ", 5)
        m = re.search(kernel + r"<(\d+), (\d+)>", name) or re.search(kernel + r"ILi(\d+)ELi(\d+)E", name)
        assert m, name
        rows[tuple(int(g) for g in m.groups())] = tuple(int(v) for v in (vgpr, agpr, scratch, occ, lds))
    return rows


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not found")
@pytest.mark.parametrize("kernel", ["k_nl_tensor_elem", "k_nl_tensor_point", "k_bdr_lf_tensor"])
def test_nl_fa_tensor_resources(kernel):
    rows = usage(kernel)
    assert sorted(rows) == SPACES
    for key, (vgpr, agpr, scratch, occ, lds) in rows.items():
        assert scratch == 0, key          # no instantiation spills
        assert lds <= 65536 and occ >= 1, key
