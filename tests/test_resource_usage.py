"""Compile-time resources of the uniform p = 2 brick CG apply (brick_um.hip k_brick_cg<XF, BF, FULL, UD>), from
the compiler's own remarks (tools/resource_usage.sh; no GPU), for the default build (3 waves per SIMD) and for
the one-round build (-DCDFEM_BUM_ONE_ROUND=1).  All 16 bricks of a CU are resident at once only at <= 128
registers per lane and <= 10,240 B of LDS per workgroup (160 KB per CU / 16), and a spill to scratch would cost
more than residency gives: no instantiation of either build may use scratch.  The bench runs
<XF, BF, FULL, UD> = <1, 1, 1, 1> (the betanom fold from the partial vector), <1, 2, 1, 1> under cg_beta_sum."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _flags(name):
    """(XF, BF, FULL, UD) of a demangled or mangled k_brick_cg instantiation name."""
    m = re.search(r"k_brick_cg<(true|false), (\d+), (true|false), (true|false)>", name)
    if m:
        return (m.group(1) == "true", int(m.group(2)), m.group(3) == "true", m.group(4) == "true")
    m = re.search(r"k_brick_cgILb([01])ELi(\d+)ELb([01])ELb([01])E", name)
    assert m, name
    return (m.group(1) == "1", int(m.group(2)), m.group(3) == "1", m.group(4) == "1")


def _rows(out):
    rows = {}
    for line in out.splitlines():
        name, vgpr, agpr, scratch, occ, lds = line.rsplit(" ", 5)
        rows[_flags(name)] = tuple(int(v) for v in (vgpr, agpr, scratch, occ, lds))
    return rows


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc not found")
def test_brick_um_resources():
    cmd = ["bash", os.path.join(ROOT, "tools", "resource_usage.sh"), "csrc/brick_um.hip", "k_brick_cg"]
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, RU_FLAGS=f))
             for f in ("", "-DCDFEM_BUM_ONE_ROUND=1")]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs)
    default, one_round = (_rows(o) for o in outs)
    print(outs[0], outs[1], sep="\n")
    for rows in (default, one_round):
        assert len(rows) == 24  # XF, FULL, UD x BF 0, 1, 2
        for flags, (vgpr, agpr, scratch, occ, lds) in rows.items():
            assert scratch == 0, flags   # no instantiation spills
            assert lds <= 10240, flags   # 16 workgroups per CU fit by LDS everywhere
    # the default build: the bench's instantiation holds 3 waves per SIMD (<= 168 registers), one LDS patch
    vgpr, agpr, scratch, occ, lds = default[(True, 1, True, True)]
    assert vgpr + agpr <= 168 and occ >= 3 and lds <= 5832 + 8 * 65 + 8
    assert all(r[3] <= 3 for r in default.values())
    # the one-round build: the bench's instantiations at 4 waves, as every table instantiation but those of a
    # partial box's first apply
    for flags in ((True, 1, True, True), (True, 2, True, True)):
        vgpr, agpr, scratch, occ, lds = one_round[flags]
        assert vgpr + agpr <= 128 and scratch == 0 and occ == 4 and lds <= 10240
    four = sorted(f for f, r in one_round.items() if r[3] == 4)
    assert four == sorted(f for f in one_round if f[3] and not (f[1] != 0 and not f[0] and not f[2]))
