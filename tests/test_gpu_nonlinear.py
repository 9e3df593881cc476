"""The nonlinear heat form, its boundary load and the device-resident Newton solve (csrc/nl_kernels.hip,
csrc/newton.hip) against the numpy restatement tests/nonlinear_ref.py, which tests/test_nonlinear_ref.py pins.

Meshes (nonlinear_ref.build_mesh): perturbed Kuhn triangles n = 6 (72 elements: two 64-element blocks, the
second partial) at P1 and P2, perturbed Kuhn tetrahedra n = 3 (162 elements) at P1 and P2, and P3 triangles on
the reference's unit square (938 triangles, 4,342 dofs).  Tolerances are the project's ladder: 1e-13 of the
largest entry for a residual, a load, matrix values, Mult and diagonal; 1e-10 relative L2 for two solves both
taken to 1e-13; 1e-8 for a solve at the reference's own stopping tolerance.

Residual histories: compared where the restatement's norm exceeds 1e-6 r0.  The restatement run with a direct
solve and run with the oracle's GMRES(30) at 1e-13 (Jacobi, ILU(0)) differ in those norms by at most 5.5e-10
relative over the six Newton cases below (measured; nonlinear_ref.HISTORY_SPREAD); the HIP path, which differs
in summation order as well, is allowed 100 times that: 5.5e-8 (nonlinear_ref.HISTORY_TOL)."""
import copy
import functools

import numpy as np
import pytest

import cdfem
import nonlinear_ref as N

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def problem(mesh_name, set_name):
    """mesh on the set's domain, restatement form (no essential dofs) with u_old and g, the x = 0 facets, set"""
    return N.newton_problem(mesh_name, set_name)


@functools.lru_cache(maxsize=None)
def ref_newton(mesh_name, set_name, rel_tol=None, freq=1):
    m, F, _, prm = problem(mesh_name, set_name)
    F.u_old = prm["u_old"].copy()
    return F.newton(prm["u_old"].copy(), abs_tol=N.NEWTON_ABS_TOL,
                    rel_tol=N.NEWTON_REL_TOL[set_name] if rel_tol is None else rel_tol, jacobian_rebuild_freq=freq)


def smooth_u(m, prm):
    """a smooth non-polynomial state, different from u_old"""
    xyz = N.dof_coords(m) / prm["scale"]
    return prm["u_old"] + 0.3 * np.cos(2.0 * xyz[:, 0] + xyz[:, 1]) * np.exp(0.5 * xyz[:, -1])


def context(m, ess):
    mm = copy.copy(m)
    mm.ess = np.asarray(ess, dtype=np.int32)
    return cdfem.Context(0).upload_mesh(mm)


def flux_values(ctx, prm, variable=False):
    """the set's constant flux at the boundary rule's points, or a non-polynomial one of the same size"""
    x = ctx.bdr_quadrature_points() / prm["scale"]
    return prm["flux"] * ((1.0 + 2.0 * x[..., 1] + np.sin(3.0 * x[..., -1])) if variable else np.ones(x.shape[:2]))


def setup(ctx, mesh_name, set_name, with_g=True):
    """nl_setup, u_old, and the Neumann load through the boundary form; returns the load"""
    m, F, (e, f), prm = problem(mesh_name, set_name)
    ctx.nl_setup(**prm["coeffs"])
    ctx.nl_set_old(prm["u_old"])
    ctx.bdr_set(e, f)
    b = ctx.bdr_lf_assemble(flux_values(ctx, prm))
    ctx.nl_set_rhs(b if with_g else None)
    return b


def rel_inf(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


FORM_CASES = [("tri1", "A"), ("tri2", "A"), ("tri2", "B"), ("tet1", "A"), ("tet2", "A"), ("tet2", "B"), ("square3", "A")]


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
@pytest.mark.parametrize("with_ess", [False, True], ids=["free", "ess"])
@pytest.mark.parametrize("mesh_name,set_name", FORM_CASES)
def test_residual_and_boundary_load(mesh_name, set_name, with_ess, with_g):
    m, F0, (e, f), prm = problem(mesh_name, set_name)
    ess = m.ess if with_ess else ()
    F = N.HeatForm(m, ess=ess, **prm["coeffs"])
    F.u_old = prm["u_old"]
    u = smooth_u(m, prm)
    with context(m, ess) as ctx:
        b = setup(ctx, mesh_name, set_name, with_g)
        # the load: constant flux against the restatement's, and a non-polynomial one
        db = rel_inf(b, F0.g)
        gv = ctx.bdr_lf_assemble(flux_values(ctx, prm, variable=True))
        s = prm["scale"]
        gr = N.boundary_load(m, e, f, lambda X: prm["flux"] * (1.0 + 2.0 * X[:, 1] / s + np.sin(3.0 * X[:, -1] / s)))
        dv = rel_inf(gv, gr)
        assert ctx.bdr_rule_size() == len(N.facet_rule(m.dim, m.order)[1])
        if with_g:
            F.g = F0.g
        R = ctx.nl_residual(u)
        dR = rel_inf(R, F.residual(u))
        print(f"{mesh_name} {set_name} ess={with_ess} g={with_g}: load {db:.2e} {dv:.2e} residual {dR:.2e}")
        assert db <= 1e-13 and dv <= 1e-13 and dR <= 1e-13
        if with_ess:
            assert np.all(R[np.asarray(m.ess)] == 0.0)
        assert np.array_equal(R, ctx.nl_residual(u))  # fixed summation orders


@pytest.mark.parametrize("with_ess", [False, True], ids=["free", "ess"])
@pytest.mark.parametrize("mesh_name,set_name", FORM_CASES)
def test_jacobian(mesh_name, set_name, with_ess):
    """after nl_gradient the assembled operator is J(u): pattern exact, values, Mult and diagonal to 1e-13"""
    m, _, _, prm = problem(mesh_name, set_name)
    ess = m.ess if with_ess else ()
    F = N.HeatForm(m, ess=ess, **prm["coeffs"])
    F.u_old = prm["u_old"]
    u = smooth_u(m, prm)
    J = F.jacobian(u, eliminated=False)
    Jc = F.eliminate(J)
    v = np.random.default_rng(5).uniform(-1.0, 1.0, m.nl)
    with context(m, ess) as ctx:
        setup(ctx, mesh_name, set_name)
        ctx.nl_gradient(u)
        rp, cols, vals = ctx.fa_csr()
        _, _, vals_c = ctx.fa_csr(constrained=True)
        assert np.array_equal(rp, J.indptr) and np.array_equal(cols, J.indices)
        scale = np.abs(J.data).max()
        dJ, dJc = np.abs(vals - J.data).max() / scale, np.abs(vals_c - Jc.data).max() / scale
        dm = rel_inf(ctx.mult(v), J @ v)
        ve = v.copy()
        ve[np.asarray(ess, dtype=np.int64)] = 0.0
        yc = Jc @ ve
        yc[np.asarray(ess, dtype=np.int64)] = v[np.asarray(ess, dtype=np.int64)]
        dmc = rel_inf(ctx.mult(v, constrained=True), yc)
        dd = rel_inf(ctx.diagonal(), J.diagonal())
        print(f"{mesh_name} {set_name} ess={with_ess}: J {dJ:.2e} Jc {dJc:.2e} mult {dm:.2e} {dmc:.2e} diag {dd:.2e}")
        assert max(dJ, dJc, dm, dmc, dd) <= 1e-13


@pytest.mark.parametrize("mesh_name", ["tri1", "tri2", "tet1", "tet2", "square3"])
def test_jacobian_linear_limit_is_fa_setup(mesh_name):
    """a1 = m1 = 0: the new element kernel against the shipped one, fa_setup(kappa = a0, mass = m0 / dt)"""
    m, _, _, prm = problem(mesh_name, "A")
    dt, a0, m0 = 0.1, 2.0, 3.0
    with context(m, m.ess) as ctx, context(m, m.ess) as lin:
        ctx.nl_setup(dt=dt, a0=a0, a1=0.0, m0=m0, m1=0.0)
        ctx.nl_set_old(prm["u_old"])
        ctx.nl_gradient(smooth_u(m, prm))
        lin.fa_setup(kinds=cdfem.DIFFUSION | cdfem.MASS, kappa=a0, mass=m0 / dt)
        for con in (False, True):
            (rp, cols, vals), (rp2, cols2, vals2) = ctx.fa_csr(con), lin.fa_csr(con)
            assert np.array_equal(rp, rp2) and np.array_equal(cols, cols2)
            d = np.abs(vals - vals2).max() / np.abs(vals2).max()
            print(f"{mesh_name} constrained={con}: {d:.2e}")
            assert d <= 1e-13


def check_against(ref, u, info, hist, u_tol):
    assert info["converged"] and info["status"] == cdfem.OK
    assert info["iterations"] == ref["iterations"]
    du = np.linalg.norm(u - ref["u"]) / np.linalg.norm(ref["u"])
    rr, r0 = np.array(ref["residual"]), ref["r0"]
    assert len(hist["residual"]) == len(rr) == info["iterations"] + 1
    sel = rr > 1e-6 * r0
    dh = (np.abs(hist["residual"][sel] - rr[sel]) / rr[sel]).max()
    print(f"iterations {info['iterations']} du {du:.2e} history {dh:.2e} linear {list(hist['linear_iterations'])} "
          f"timers {info['residual_seconds']:.4f} {info['jacobian_seconds']:.4f} {info['linear_seconds']:.4f}")
    assert du <= u_tol and dh <= N.HISTORY_TOL
    assert info["initial_residual"] == pytest.approx(r0, rel=1e-12)
    assert info["final_residual"] == hist["residual"][-1] and hist["update"][-1] == 0.0
    assert info["linear_iterations"] == int(hist["linear_iterations"].sum())
    ru = np.array(ref["update"])
    assert np.abs(hist["update"][:-1] - ru).max() <= 1e-8 * ru.max()
    assert info["initial_update_norm"] == pytest.approx(ref["du0"], rel=1e-8)


@pytest.mark.parametrize("pc", ["ilu", "jacobi"])
@pytest.mark.parametrize("set_name", ["A", "B"])
@pytest.mark.parametrize("mesh_name", ["tri2", "square3", "tet2"])
def test_newton(mesh_name, set_name, pc):
    """GMRES(30) + ILU(0) / Jacobi at 1e-13: the restatement's iteration count, u to 1e-10, the history"""
    m, _, _, prm = problem(mesh_name, set_name)
    ref = ref_newton(mesh_name, set_name)
    with context(m, ()) as ctx:
        setup(ctx, mesh_name, set_name)
        u, info, hist = ctx.newton_solve(prm["u_old"], abs_tol=N.NEWTON_ABS_TOL, rel_tol=N.NEWTON_REL_TOL[set_name],
                                         method="gmres", pc=pc, lin_rel_tol=1e-13, lin_abs_tol=0.0, lin_max_iter=50000)
        print(mesh_name, set_name, pc, end=" ")
        check_against(ref, u, info, hist, 1e-10)


def test_newton_reference_linear_options():
    """the reference's own linear options (Input/petsc_nonlinear.opts: GMRES, rtol 1e-10, atol 1e-12, max_it
    2000, bjacobi / ILU(0)) on its own coefficients (set B): iterations equal, solution to 1e-8"""
    m, _, _, prm = problem("tri2", "B")
    ref = ref_newton("tri2", "B")
    with context(m, ()) as ctx:
        setup(ctx, "tri2", "B")
        u, info, hist = ctx.newton_solve(prm["u_old"], method="gmres", pc="ilu", lin_rel_tol=1e-10, lin_abs_tol=1e-12,
                                         lin_max_iter=2000)
        du = np.linalg.norm(u - ref["u"]) / np.linalg.norm(ref["u"])
        print(f"iterations {info['iterations']} du {du:.2e}")
        assert info["converged"] and info["iterations"] == ref["iterations"] and du <= 1e-8


def test_three_backward_euler_steps():
    """set A on P2 triangles, u_old taken from the previous solution on the device: each step's iteration count
    equals the restatement's, the final state agrees to 1e-10"""
    m, F, _, prm = problem("tri2", "A")
    F.u_old = prm["u_old"].copy()
    ur = prm["u_old"].copy()
    with context(m, ()) as ctx:
        setup(ctx, "tri2", "A")
        du = ctx.to_device(prm["u_old"])
        for step in range(3):
            F.u_old = ur.copy()
            r = F.newton(ur, abs_tol=N.NEWTON_ABS_TOL, rel_tol=N.THREE_STEP_REL_TOL)
            ur = r["u"]
            ctx.nl_set_old(du, where=cdfem.DEVICE)
            info, hist = ctx.newton_solve_device(du, abs_tol=N.NEWTON_ABS_TOL, rel_tol=N.THREE_STEP_REL_TOL, pc="ilu",
                                                 lin_rel_tol=1e-13, lin_abs_tol=0.0, lin_max_iter=50000)
            print(step, info["iterations"], hist["residual"])
            assert info["converged"] and info["iterations"] == r["iterations"]
        u = ctx.from_device(du, m.nl)
        ctx.free(du)
        F.u_old = prm["u_old"].copy()
        d = np.linalg.norm(u - ur) / np.linalg.norm(ur)
        print(f"final {d:.2e}")
        assert d <= 1e-10


def test_jacobian_rebuild_freq_2():
    m, _, _, prm = problem("tri2", "A")
    ref = ref_newton("tri2", "A", freq=2)
    with context(m, ()) as ctx:
        setup(ctx, "tri2", "A")
        u, info, hist = ctx.newton_solve(prm["u_old"], rel_tol=N.NEWTON_REL_TOL["A"], jacobian_rebuild_freq=2, pc="ilu",
                                         lin_rel_tol=1e-13, lin_abs_tol=0.0, lin_max_iter=50000)
        check_against(ref, u, info, hist, 1e-10)
        assert info["iterations"] == 4


def test_max_iter_1_and_bitwise_repeat():
    """max_iter = 1: CDFEM_ERR_NOT_CONVERGED with iterations = 1, converged = 0 and the history filled; two
    identical Newton solves are bitwise equal (no atomics anywhere)"""
    m, _, _, prm = problem("tet2", "A")
    with context(m, ()) as ctx:
        setup(ctx, "tet2", "A")
        kw = dict(rel_tol=N.NEWTON_REL_TOL["A"], pc="jacobi", lin_rel_tol=1e-13, lin_abs_tol=0.0, lin_max_iter=50000)
        u1, info, hist = ctx.newton_solve(prm["u_old"], max_iter=1, **kw)
        assert info["status"] == cdfem.ERR_NOT_CONVERGED and not info["converged"] and info["iterations"] == 1
        assert len(hist["residual"]) == 1 and hist["update"][0] > 0 and hist["linear_iterations"][0] > 0
        assert "Newton" in info["message"]
        assert not np.array_equal(u1, prm["u_old"])  # the one update was taken
        with pytest.raises(cdfem.CdfemError):
            ctx.newton_solve(prm["u_old"], max_iter=1, raise_on_fail=True, **kw)
        ua, ia, ha = ctx.newton_solve(prm["u_old"], **kw)
        ub, ib, hb = ctx.newton_solve(prm["u_old"], **kw)
        assert ia["converged"] and np.array_equal(ua, ub)
        assert np.array_equal(ha["residual"], hb["residual"]) and np.array_equal(ha["update"], hb["update"])
        assert np.array_equal(ha["linear_iterations"], hb["linear_iterations"])


def test_linear_solve_failure_ends_newton():
    """a linear solve that does not converge ends the Newton solve: NOT_CONVERGED, the iteration named"""
    m, _, _, prm = problem("tri2", "A")
    with context(m, ()) as ctx:
        setup(ctx, "tri2", "A")
        u, info, hist = ctx.newton_solve(prm["u_old"], pc="jacobi", lin_rel_tol=1e-13, lin_abs_tol=0.0, lin_max_iter=3)
        assert info["status"] == cdfem.ERR_NOT_CONVERGED and not info["converged"] and info["iterations"] == 0
        assert "Newton iteration 0" in info["message"]
        assert np.array_equal(u, prm["u_old"])


def test_status_codes():
    box = cdfem.box_mesh(2, 4, 2)
    with cdfem.Context(0).upload_mesh(box) as ctx:
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_setup(dt=0.1, a0=1.0, a1=0.5, m0=1.0, m1=0.5)
        assert e.value.code == cdfem.ERR_UNSUPPORTED
    m, _, (fe, ff), prm = problem("tri2", "A")
    with context(m, ()) as ctx:
        for call in (lambda: ctx.nl_residual(prm["u_old"]), lambda: ctx.nl_gradient(prm["u_old"]),
                     lambda: ctx.newton_solve(prm["u_old"]), lambda: ctx.nl_set_old(prm["u_old"]),
                     lambda: ctx.bdr_rule_size()):
            with pytest.raises(cdfem.CdfemError) as e:
                call()
            assert e.value.code == cdfem.ERR_STATE
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_setup(dt=0.0, a0=1.0, a1=0.5, m0=1.0, m1=0.5)
        assert e.value.code == cdfem.ERR_ARG
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.bdr_set(np.array([m.ne]), np.array([0]))
        assert e.value.code == cdfem.ERR_ARG
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.bdr_set(np.array([0]), np.array([3]))
        assert e.value.code == cdfem.ERR_ARG
        setup(ctx, "tri2", "A")
        assert ctx.rule_size(cdfem.RULE_NONLINEAR) == 12
        # a context with a two-rank host communicator is refused
        ctx.comm_init_host(0, 2, lambda a: None, lambda *a: None)
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.newton_solve(prm["u_old"])
        assert e.value.code == cdfem.ERR_UNSUPPORTED


def test_linear_path_undisturbed():
    """after a Newton solve a plain fa_setup + solve on the same context gives a fresh context's results, bitwise"""
    m, _, _, prm = problem("tri2", "A")
    b = np.random.default_rng(7).uniform(-1.0, 1.0, m.nl)

    def linear(ctx):
        ctx.fa_setup(kinds=cdfem.DIFFUSION | cdfem.CONVECTION | cdfem.MASS, kappa=0.1, conv=(1.0, -2.0, 0.0), mass=1.0)
        _, B = ctx.form_linear_system(np.zeros(m.nl), b)
        out = [ctx.fa_csr(True)[2], ctx.mult(b)]
        for pc in ("jacobi", "ilu"):
            x, info = ctx.solve(B, method="gmres", pc=pc, rel_tol=1e-10, abs_tol=1e-12, max_iter=500)
            assert info["converged"]
            out += [x, np.array([info["iterations"]])]
        return out

    with context(m, m.ess) as ctx, context(m, m.ess) as fresh:
        setup(ctx, "tri2", "A")
        _, info, _ = ctx.newton_solve(prm["u_old"], rel_tol=N.NEWTON_REL_TOL["A"])
        assert info["converged"]
        for a, c in zip(linear(ctx), linear(fresh)):
            assert np.array_equal(a, c)
        # and the nonlinear form is still there afterwards
        assert np.abs(ctx.nl_residual(prm["u_old"])).max() > 0.0
