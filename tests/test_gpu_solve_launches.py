"""The loop structure and the profiling brackets of the four Krylov drivers (csrc/solve.hip).

Every case solves with profiling on, rel_tol = abs_tol = 0 and a fixed max_iter, then reads how many timed
intervals cdfem_profile_read holds per kernel id, and the iteration count.  A bracket lost, doubled or moved
to another launch, a loop leaving a check early or late, or a driver taking another path changes a count.

EXPECTED was recorded by running run_case of this file on the library of commit 9a6263b (the drivers still
in capi.hip, written out one by one); it is not derived from the code under test."""
import numpy as np
import pytest

import cdfem
from oracle import oracle as O

pytestmark = pytest.mark.gpu
C3 = (1.0, -2.0, 0.5)
KERNELS = (("apply", cdfem.K_APPLY), ("e2l", cdfem.K_E2L), ("update", cdfem.K_UPDATE),
           ("direction", cdfem.K_DIRECTION), ("orth", cdfem.K_ORTH))

BOX8 = dict(mesh=("box", (8, 8, 8), 2, 0.0, True))
CASES = {
    # brick CG: the loop crosses one check boundary and stops inside the second
    "brick_cg": dict(BOX8, solve=dict(method="cg", max_iter=20, check_every=16)),
    "brick_cg_kron_noxfold": dict(BOX8, options=dict(pa_uniform=0, cg_xfold=0),
                                  solve=dict(method="cg", max_iter=20, check_every=16)),
    # generic CG with the direction pass
    "generic_cg": dict(mesh=("box", (5, 6, 7), 2, 0.1, False), solve=dict(method="cg", max_iter=20, check_every=16)),
    # block CG, and the fused CG with ho_dfold
    "block_cg": dict(mesh=("box", (4, 4, 4), 3, 0.0, True), options=dict(ho_brick=1),
                     solve=dict(method="cg", max_iter=20, check_every=16)),
    "fused_cg": dict(mesh=("box", (4, 4, 4), 3, 0.0, True), options=dict(ho_brick=0, cg_fused=1),
                     solve=dict(method="cg", max_iter=20, check_every=16)),
    "gmres_pb": dict(BOX8, options=dict(gm_pb=1), solve=dict(method="gmres", restart=5, max_iter=12)),
    "gmres_poll1": dict(BOX8, options=dict(gm_pb=0, gm_poll=1), solve=dict(method="gmres", restart=5, max_iter=12)),
    "bicgstab_pb": dict(BOX8, options=dict(gm_pb=1), solve=dict(method="bicgstab", max_iter=8, check_every=3)),
    "bicgstab_mult": dict(BOX8, options=dict(gm_pb=0), solve=dict(method="bicgstab", max_iter=8, check_every=3)),
    # assembled: 4^3 x 6 tetrahedra, P2
    "gmres_ilu": dict(mesh=("tets", 4, 2), solve=dict(method="gmres", pc="ilu", restart=5, max_iter=7)),
}
DEFAULTS = dict(pa_uniform=1, cg_xfold=1, ho_brick=1, cg_fused=1, gm_pb=1, gm_poll=4)

EXPECTED = {
    "brick_cg": {'apply': 21, 'e2l': 21, 'update': 20, 'direction': 0, 'orth': 0, 'iterations': 20},
    "brick_cg_kron_noxfold": {'apply': 21, 'e2l': 21, 'update': 20, 'direction': 0, 'orth': 0, 'iterations': 20},
    "generic_cg": {'apply': 21, 'e2l': 21, 'update': 20, 'direction': 20, 'orth': 0, 'iterations': 20},
    "block_cg": {'apply': 21, 'e2l': 21, 'update': 20, 'direction': 0, 'orth': 0, 'iterations': 20},
    "fused_cg": {'apply': 21, 'e2l': 21, 'update': 20, 'direction': 0, 'orth': 0, 'iterations': 20},
    "gmres_pb": {'apply': 17, 'e2l': 2, 'update': 3, 'direction': 0, 'orth': 15, 'iterations': 12},
    "gmres_poll1": {'apply': 15, 'e2l': 15, 'update': 3, 'direction': 0, 'orth': 13, 'iterations': 12},
    "bicgstab_pb": {'apply': 16, 'e2l': 0, 'update': 25, 'direction': 0, 'orth': 0, 'iterations': 8},
    "bicgstab_mult": {'apply': 16, 'e2l': 16, 'update': 25, 'direction': 0, 'orth': 0, 'iterations': 8},
    "gmres_ilu": {'apply': 11, 'e2l': 0, 'update': 2, 'direction': 0, 'orth': 10, 'iterations': 7},
}


def run_case(ctx, case):
    """Counts of timed intervals per kernel id, and the result's iterations, of one case."""
    kind = case["mesh"][0]
    if kind == "box":
        _, shape, p, pert, structured = case["mesh"]
        om = O.BoxMesh(3, shape, p, perturb=pert)
        ctx.upload_mesh(cdfem.Mesh(3, p, om.verts, om.dofmap, om.nl, om.ess))
        if structured:
            ctx.set_structured(*shape)
        nl, ess = om.nl, om.ess
    else:
        _, n, p = case["mesh"]
        gm = cdfem.kuhn_mesh(3, n, p)
        ctx.upload_mesh(gm)
        nl, ess = gm.nl, gm.ess
    opts = case.get("options", {})
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        setup = ctx.pa_setup if kind == "box" else ctx.fa_setup
        setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
        rng = np.random.default_rng(3)
        u = np.zeros(nl)
        u[ess] = rng.uniform(-1, 1, len(ess))
        _, B = ctx.form_linear_system(u, rng.uniform(-1, 1, nl))
        ctx.set_option("profile_mask", -1)
        ctx.profile(True)
        kw = dict(pc="jacobi", rel_tol=0.0, abs_tol=0.0)
        kw.update(case["solve"])
        _, info = ctx.solve(B, **kw)
        out = {name: ctx.profile_read(k)[1] for name, k in KERNELS}
        out["iterations"] = info["iterations"]
        return out
    finally:
        ctx.profile(False)
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_counts(gpu_ctx, name):
    got = run_case(gpu_ctx, CASES[name])
    print(name, got)
    assert got == EXPECTED[name]
