#!/usr/bin/env python3
"""Make tests/golden/reference_reader_output.npz: what the product reader gives on the reference's
own mesh files, recorded once so that tests/test_reference_inputs.py needs no file outside the
repository.

Test infrastructure.  Input: the directory that holds the reference's unit_square.msh and
unit_circle.msh (the files tests/golden/make_reference_meshes.py reads), and a built libcdfem.so.
Output, per mesh <name> in {square, circle}:
  <name>_topo_vxyz / _topo_ev / _topo_bv / _topo_ba   cdfem_gmsh_topology of the reference's file
  <name>_space_verts / _space_dofmap / _space_ess / _space_dof_xyz / _space_bdr_mask
                                                      cdfem.gmsh_mesh(file, 3): the order-3 space
  <name>_raw_sha256   str   JSON {array name: sha256 of its bytes} of make_reference_meshes.parse_msh
                            of the file ("physical": sha256 of its JSON text)

usage: python tests/golden/make_reference_reader_output.py REFERENCE_MESH_DIR
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))

RAW_KEYS = ("node_id", "node_xyz", "elem_id", "elem_type", "elem_phys", "elem_geom", "elem_nodes")
SPACE_KEYS = ("verts", "dofmap", "ess", "dof_xyz", "bdr_mask")
ORDER = 3


def raw_digests(m):
    """sha256 of every array of a parsed mesh (parse_msh layout) and of its physical-names JSON."""
    d = {k: hashlib.sha256(np.ascontiguousarray(m[k]).tobytes()).hexdigest() for k in RAW_KEYS}
    d["physical"] = hashlib.sha256(json.dumps(m["physical"]).encode()).hexdigest()
    return d


def main(ref_dir):
    import cdfem
    import make_reference_meshes as MK
    from test_reference_inputs import _topology
    arrays = {}
    for name, fn in MK.FILES.items():
        path = os.path.join(ref_dir, fn)
        for k, v in zip(("vxyz", "ev", "bv", "ba"), _topology(path)):
            arrays[f"{name}_topo_{k}"] = v
        m = cdfem.gmsh_mesh(path, ORDER)
        for k in SPACE_KEYS:
            arrays[f"{name}_space_{k}"] = np.asarray(getattr(m, k))
        arrays[f"{name}_raw_sha256"] = np.array(json.dumps(raw_digests(MK.parse_msh(path))))
    out = os.path.join(HERE, "reference_reader_output.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
