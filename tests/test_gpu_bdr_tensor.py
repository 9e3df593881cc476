"""The boundary linear form on quad / hex faces (cdfem_bdr_* on tensor meshes; csrc/nl_fa_tensor.hip
k_bdr_lf_tensor, then k_bdr_gather) against the numpy restatement tests/nonlinear_tensor_bdr_ref.py, which
tests/test_nonlinear_tensor_bdr_ref.py pins, and the reference driver's set-up end to end: the Neumann flux on
x = 0 through the boundary form, essential dofs on x = 1, Newton with GMRES + ILU(0) on the assembled Jacobian.

Meshes: nonlinear_tensor_ref.MESHES with perturb = 0.2 (the hex faces inside the boundary planes are bilinear in
their own plane: sigma varies over them).  Facets: all of x = 0 (side 0), y = 1 (side 1) and, on hexes, z = 0.
Tolerances: 1e-14 for point coordinates of a unit box, 1e-13 of max |b| for the load.

End to end, the restatement's rn / r0 with its own boundary load (direct solves):
    quad2, set A   1, 6.2e-2, 2.9e-4, 1.0e-8, 3.1e-15     rel_tol 1e-7
    hex1,  set B   1, 1.1e-1, 8.5e-4, 5.2e-8, 1.7e-15     rel_tol 1e-6 (|R| = 1.3e-6 at the stop, abs_tol 1e-10)
so no iterate is within a factor 10 of a threshold; history and solution tolerances are
tests/test_gpu_nonlinear_pa.py's."""
import copy
import functools

import numpy as np
import pytest

import cdfem
import nonlinear_tensor_bdr_ref as B
import nonlinear_tensor_ref as T

pytestmark = pytest.mark.gpu

ALL_MESHES = ["quad1", "quad2", "quad3", "hex1", "hex2", "hex2L"]
E2E = {("quad2", "A"): 1e-7, ("hex1", "B"): 1e-6}


@functools.lru_cache(maxsize=None)
def problem(mesh_name, set_name):
    """the mesh on the set's domain, the restatement's form (essential dofs on x = 1), the set, those dofs, and
    the facets: x = 0, y = 1 and (hexes) z = 0, concatenated; the first n0 are the x = 0 plane"""
    m, F, prm, ed = T.problem(mesh_name, set_name, ess=True)
    s = prm["scale"]
    planes = [(0, 0.0), (1, s)] + ([(2, 0.0)] if m.dim == 3 else [])
    ef = [B.plane_facets(m, axis, value, tol=1e-12 * s) for axis, value in planes]
    e, f = np.concatenate([x[0] for x in ef]), np.concatenate([x[1] for x in ef])
    return m, F, prm, ed, e, f, len(ef[0][0])


def context(m, ess=()):
    mm = copy.copy(m)
    mm.ess = np.asarray(ess, dtype=np.int32)
    return cdfem.Context(0).upload_mesh(mm)


def variable(prm):
    s = prm["scale"]
    return lambda X: prm["flux"] * (1.0 + 2.0 * X[:, 1] / s + np.sin(3.0 * X[:, -1] / s))


@pytest.mark.parametrize("set_name", ["A", "B"])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_rule_points_and_load(name, set_name):
    m, F, prm, ed, e, f, n0 = problem(name, set_name)
    assert n0 > 0 and len(e) > n0 and set(f) == ({0, 3, 4} if m.dim == 3 else {0, 3})
    xr = B.quadrature_points(m, e, f)
    const = lambda X: np.full(len(X), prm["flux"])
    with context(m) as ctx:                                   # cdfem_bdr_set needs only a mesh
        ctx.bdr_set(e, f)
        assert ctx.bdr_rule_size() == B.rule_size(m.dim, m.order) == xr.shape[1]
        x = ctx.bdr_quadrature_points()
        dx = np.abs(x - xr).max() / prm["scale"]
        for label, g in (("constant", const), ("variable", variable(prm))):
            gq = np.array([g(xt) for xt in x])
            b = ctx.bdr_lf_assemble(gq)
            br = B.boundary_load(m, e, f, g)
            db = np.abs(b - br).max() / np.abs(br).max()
            print(f"{name} {set_name} {label}: points {dx:.2e} load {db:.2e}")
            assert db <= 1e-13
            assert np.array_equal(b, ctx.bdr_lf_assemble(gq))  # ascending facet order, no atomics
            off = np.setdiff1d(np.arange(m.nl), np.unique(np.concatenate([m.dofmap[ee][B.facet_dofs(m.dim, m.order, ff)]
                                                                          for ee, ff in zip(e, f)])))
            assert np.all(b[off] == 0.0)
        assert dx <= 1e-14
        # a second facet list replaces the first: the x = 0 plane alone, the measure of that side
        ctx.bdr_set(e[:n0], f[:n0])
        total = ctx.bdr_lf_assemble(np.ones((n0, ctx.bdr_rule_size()))).sum()
        assert abs(total - prm["scale"] ** (m.dim - 1)) <= 1e-13 * prm["scale"] ** (m.dim - 1)


def test_status_codes():
    m = T.build_mesh("hex1")
    with context(m) as ctx:
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.bdr_rule_size()
        assert e.value.code == cdfem.ERR_STATE
        for elem, face in (([m.ne], [0]), ([-1], [0]), ([0], [6]), ([0], [-1])):
            with pytest.raises(cdfem.CdfemError) as e:
                ctx.bdr_set(np.array(elem), np.array(face))
            assert e.value.code == cdfem.ERR_ARG
        ctx.bdr_set(np.array([0]), np.array([5]))
        assert ctx.bdr_rule_size() == 4
    q = T.build_mesh("quad2")
    with context(q) as ctx:
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.bdr_set(np.array([0]), np.array([4]))
        assert e.value.code == cdfem.ERR_ARG
        ctx.bdr_set(np.array([0]), np.array([3]))
        ctx.comm_init_host(0, 2, lambda a: None, lambda *a: None)
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.bdr_set(np.array([0]), np.array([3]))
        assert e.value.code == cdfem.ERR_UNSUPPORTED
    with cdfem.Context(0).upload_mesh(cdfem.box_mesh(2, 2, 4)) as ctx:   # outside the spaces of the nonlinear form
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.bdr_set(np.array([0]), np.array([0]))
        assert e.value.code == cdfem.ERR_UNSUPPORTED


@pytest.mark.parametrize("assembled", [True, False], ids=["fa", "pa"])
@pytest.mark.parametrize("mesh_name,set_name", list(E2E))
def test_driver_setup_end_to_end(mesh_name, set_name, assembled):
    """flux on x = 0 through bdr_lf_assemble into nl_set_rhs, essential dofs on x = 1, Newton with GMRES + ILU(0)
    through nl_fa_setup (and with Jacobi through nl_pa_setup: the form serves both), against the restatement's
    Newton with the restatement's load"""
    m, F0, prm, ed, e, f, n0 = problem(mesh_name, set_name)
    e, f = e[:n0], f[:n0]
    rel_tol = E2E[(mesh_name, set_name)]
    F = copy.copy(F0)
    F.g = B.boundary_load(m, e, f, lambda X: np.full(len(X), prm["flux"]))
    F.u_old = prm["u_old"].copy()
    ref = F.newton(prm["u_old"].copy(), abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol)
    with context(m, ed) as ctx:
        (ctx.nl_fa_setup if assembled else ctx.nl_pa_setup)(**prm["coeffs"])
        ctx.nl_set_old(prm["u_old"])
        ctx.bdr_set(e, f)
        g = ctx.bdr_lf_assemble(np.full((n0, ctx.bdr_rule_size()), prm["flux"]))
        dg = np.abs(g - F.g).max() / np.abs(F.g).max()
        ctx.nl_set_rhs(g)
        u, info, hist = ctx.newton_solve(prm["u_old"], abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol, method="gmres",
                                         pc="ilu" if assembled else "jacobi", lin_rel_tol=1e-13, lin_abs_tol=0.0,
                                         lin_max_iter=50000)
    assert info["converged"] and info["iterations"] == ref["iterations"]
    du = np.linalg.norm(u - ref["u"]) / np.linalg.norm(ref["u"])
    rr, r0 = np.array(ref["residual"]), ref["r0"]
    sel = rr > 1e-6 * r0
    dh = (np.abs(hist["residual"][sel] - rr[sel]) / rr[sel]).max()
    print(f"{mesh_name} {set_name} assembled={assembled}: load {dg:.2e} iterations {info['iterations']} du {du:.2e} "
          f"history {dh:.2e} linear {list(hist['linear_iterations'])}")
    assert dg <= 1e-13 and du <= 1e-10 and dh <= T.HISTORY_TOL
    assert np.array_equal(u[ed], prm["u_old"][ed])
