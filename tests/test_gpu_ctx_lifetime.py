"""One context carried through meshes of every kind computes what a fresh context computes, bit for bit.

cdfem_ctx keeps its per-mesh state in MeshState / PartitionState (csrc/ctx_state.hpp); a new upload resets
them to their defaults.  A buffer or flag that survived an upload would send the next mesh down a stale path.
Context A runs, in this order: an 8^3 p = 2 structured box (brick CG), Kuhn tetrahedra n = 4 P2 (assembled,
GMRES(5) + ILU), a 4^3 p = 3 structured box (block CG), a perturbed (5, 6, 7) p = 2 box (generic path,
BiCGStab), the first case again, an upload that is refused after the old mesh was freed, and the first case
once more.  After each case the solution and the result (converged, iterations, the two norms; not the wall
time) must equal, bitwise, those of the same case on a context created for it alone.  The solves are
bitwise repeatable (tests/test_gpu_parity.py), so any difference is state carried over.
"""
import numpy as np
import pytest

import cdfem
from oracle import oracle as O

pytestmark = pytest.mark.gpu
C3 = (1.0, -2.0, 0.5)

CASES = {
    "brick_cg": dict(mesh=("box", (8, 8, 8), 2, 0.0, True), solve=dict(method="cg", max_iter=20)),
    "gmres_ilu": dict(mesh=("tets", 4, 2), solve=dict(method="gmres", pc="ilu", restart=5, max_iter=7)),
    "block_cg": dict(mesh=("box", (4, 4, 4), 3, 0.0, True), solve=dict(method="cg", max_iter=20)),
    "generic_bicgstab": dict(mesh=("box", (5, 6, 7), 2, 0.1, False),
                             solve=dict(method="bicgstab", max_iter=8, check_every=3)),
}
ORDER = ["brick_cg", "gmres_ilu", "block_cg", "generic_bicgstab", "brick_cg", "refused_upload", "brick_cg"]


def run_case(ctx, case):
    """The solution and the result of one case: upload, setup, linear system, solve."""
    if case["mesh"][0] == "box":
        _, shape, p, pert, structured = case["mesh"]
        om = O.BoxMesh(3, shape, p, perturb=pert)
        ctx.upload_mesh(cdfem.Mesh(3, p, om.verts, om.dofmap, om.nl, om.ess))
        if structured:
            ctx.set_structured(*shape)
        nl, ess, setup = om.nl, om.ess, ctx.pa_setup
    else:
        _, n, p = case["mesh"]
        gm = cdfem.kuhn_mesh(3, n, p)
        ctx.upload_mesh(gm)
        nl, ess, setup = gm.nl, gm.ess, ctx.fa_setup
    setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    rng = np.random.default_rng(3)
    u = np.zeros(nl)
    u[ess] = rng.uniform(-1, 1, len(ess))
    _, B = ctx.form_linear_system(u, rng.uniform(-1, 1, nl))
    kw = dict(pc="jacobi", rel_tol=0.0, abs_tol=0.0)
    kw.update(case["solve"])
    x, info = ctx.solve(B, **kw)
    return x, {k: info[k] for k in ("converged", "iterations", "final_norm", "initial_norm")}


@pytest.fixture(scope="module")
def fresh():
    """Each case on a context of its own, created for it and closed after (computed once, never changed)."""
    if cdfem.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on an MI355X")
    ref = {}
    for name, case in CASES.items():
        with cdfem.Context(0) as ctx:
            ref[name] = run_case(ctx, case)
        ref[name][0].setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def ctx_a(fresh):
    ctx = cdfem.Context(0)
    yield ctx
    ctx.close()


def refused_upload(ctx):
    """An essential list that holds nl: refused by the range check, which runs after the old mesh is freed."""
    om = O.BoxMesh(3, (2, 2, 2), 1)
    ess = np.append(np.asarray(om.ess, dtype=np.int32), np.int32(om.nl))
    with pytest.raises(cdfem.CdfemError) as e:
        ctx.upload_mesh(cdfem.Mesh(3, 1, om.verts, om.dofmap, om.nl, ess))
    assert e.value.code == cdfem.ERR_ARG, e.value
    with pytest.raises(cdfem.CdfemError) as e:  # no mesh is left behind
        ctx.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    assert e.value.code == cdfem.ERR_STATE, e.value


@pytest.mark.parametrize("step", range(len(ORDER)), ids=[f"{i}_{n}" for i, n in enumerate(ORDER)])
def test_reused_context_equals_fresh(ctx_a, fresh, step):
    name = ORDER[step]
    if name == "refused_upload":
        refused_upload(ctx_a)
        return
    x, info = run_case(ctx_a, CASES[name])
    x0, info0 = fresh[name]
    print(name, info, "differing entries:", int(np.count_nonzero(x.view(np.uint64) != x0.view(np.uint64))))
    assert info["iterations"] == CASES[name]["solve"]["max_iter"]
    assert {k: np.float64(v).tobytes() for k, v in info.items()} == {k: np.float64(v).tobytes() for k, v in info0.items()}
    assert np.array_equal(x.view(np.uint64), x0.view(np.uint64))
