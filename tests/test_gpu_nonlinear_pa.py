"""The matrix-free nonlinear heat form on quads and hexes (cdfem_nl_pa_setup; csrc/nl_tensor.hip k_nl_tensor,
csrc/newton.hip) against the numpy restatement tests/nonlinear_tensor_ref.py, which
tests/test_nonlinear_tensor_ref.py pins.

Meshes (nonlinear_tensor_ref.MESHES): cdfem.box_mesh with perturb = 0.2, non-cubic, their element counts no
multiple of a workgroup's 28 / 16 / 10 elements; hex2L has 60 elements (6 workgroups).  Sets A and B are
nonlinear_ref's, set B on the mesh scaled by 0.01; essential dofs are none or the x = 1 face.  Tolerances are the
project's ladder: 1e-13 of the largest entry for a residual, 1e-13 of max |J| |v|_inf for Mult and the diagonal,
1e-10 relative L2 for two solves both taken to 1e-13.  Residual histories are compared where the restatement's
norm exceeds 1e-6 r0, within nonlinear_tensor_ref.HISTORY_TOL (100 times the spread measured between the
restatement's direct and GMRES runs)."""
import copy
import functools

import numpy as np
import pytest

import cdfem
import nonlinear_tensor_ref as T

pytestmark = pytest.mark.gpu

ALL_MESHES = ["quad1", "quad2", "quad3", "hex1", "hex2", "hex2L"]
LIN = dict(method="gmres", pc="jacobi", lin_rel_tol=1e-13, lin_abs_tol=0.0, lin_max_iter=50000)


@functools.lru_cache(maxsize=None)
def problem(mesh_name, set_name, ess, perturb=0.2):
    """mesh on the set's domain, restatement form with u_old and the load, the set, the essential dofs"""
    return T.problem(mesh_name, set_name, ess=ess, perturb=perturb)


@functools.lru_cache(maxsize=None)
def ref_newton(mesh_name, set_name, rel_tol, freq=1, perturb=0.2):
    m, F, prm, ed = problem(mesh_name, set_name, True, perturb)
    F.u_old = prm["u_old"].copy()
    return F.newton(prm["u_old"].copy(), abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol, jacobian_rebuild_freq=freq)


def smooth_u(m, prm):
    """a smooth non-polynomial state, different from u_old"""
    xyz = T.dof_coords(m) / prm["scale"]
    amp = 0.3 if prm["scale"] == 1.0 else 2.0
    return prm["u_old"] + amp * np.cos(2.0 * xyz[:, 0] + xyz[:, 1]) * np.exp(0.5 * xyz[:, -1])


def context(m, ess, structured=None):
    mm = copy.copy(m)
    mm.ess = np.asarray(ess, dtype=np.int32)
    ctx = cdfem.Context(0).upload_mesh(mm)
    if structured:
        ctx.set_structured(*structured)
    return ctx


def setup(ctx, F, prm, with_g=True):
    ctx.nl_pa_setup(**prm["coeffs"])
    ctx.nl_set_old(prm["u_old"])
    ctx.nl_set_rhs(F.g if with_g else None)


def rel_inf(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("name", ALL_MESHES)
def test_rule(name):
    """CDFEM_RULE_NONLINEAR: (p + 2)^2 / (p + 3)^3 points, the restatement's, q lexicographic with qx fastest"""
    m, F, prm, _ = problem(name, "A", False)
    with context(m, ()) as ctx:
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.rule_size(cdfem.RULE_NONLINEAR)
        assert e.value.code == cdfem.ERR_STATE
        setup(ctx, F, prm)
        nq = ctx.rule_size(cdfem.RULE_NONLINEAR)
        assert nq == {"quad1": 9, "quad2": 16, "quad3": 25, "hex1": 64, "hex2": 125, "hex2L": 125}[name]
        d = np.abs(ctx.quadrature_points(cdfem.RULE_NONLINEAR) - F.xq).max()
        print(f"{name}: {d:.2e}")
        assert d <= 1e-14
        assert ctx.rule_size(cdfem.RULE_OPERATOR) == (m.order + (1 if m.dim == 2 else 2)) ** m.dim  # unchanged


@pytest.mark.parametrize("with_ess", [False, True], ids=["free", "ess"])
@pytest.mark.parametrize("set_name", ["A", "B"])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_residual(name, set_name, with_ess):
    m, F, prm, ed = problem(name, set_name, with_ess)
    u = smooth_u(m, prm)
    g = F.g.copy()
    try:
        with context(m, ed) as ctx:
            for with_g in (True, False):
                setup(ctx, F, prm, with_g)
                F.g = g if with_g else np.zeros(m.nl)
                R, Rr = ctx.nl_residual(u), F.residual(u)
                dR = rel_inf(R, Rr)
                print(f"{name} {set_name} ess={with_ess} g={with_g}: residual {dR:.2e}")
                assert dR <= 1e-13
                assert np.all(R[ed] == 0.0)
                assert np.array_equal(R, ctx.nl_residual(u))  # one fixed summation order
    finally:
        F.g = g


@pytest.mark.parametrize("with_ess", [False, True], ids=["free", "ess"])
@pytest.mark.parametrize("set_name", ["A", "B"])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_jacobian(name, set_name, with_ess):
    """after nl_gradient(u) the current operator is J(u), matrix-free: Mult unconstrained, constrained and
    rank-local, and the diagonal, against the restatement's CSR, 1e-13 of max |J| |v|_inf"""
    m, F, prm, ed = problem(name, set_name, with_ess)
    u = smooth_u(m, prm)
    J = F.jacobian(u, eliminated=False)
    Jc = F.eliminate(J)
    v = np.random.default_rng(5).uniform(-1.0, 1.0, m.nl)
    scale = np.abs(J.data).max() * np.abs(v).max()
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.mult(v)
        assert e.value.code == cdfem.ERR_STATE  # no operator yet
        ctx.nl_gradient(u)
        assert ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")
        y0, y2 = ctx.mult(v), ctx.mult(v, constrained=2)
        dm = np.abs(y0 - J @ v).max() / scale
        ve = v.copy()
        ve[ed] = 0.0
        yr = Jc @ ve
        yr[ed] = v[ed]
        yc = ctx.mult(v, constrained=True)
        dmc = np.abs(yc - yr).max() / scale
        dd = np.abs(ctx.diagonal() - J.diagonal()).max() / np.abs(J.data).max()
        print(f"{name} {set_name} ess={with_ess}: mult {dm:.2e} {dmc:.2e} diag {dd:.2e}")
        assert max(dm, dmc, dd) <= 1e-13
        assert np.array_equal(y0, y2) and np.array_equal(yc[ed], v[ed])
        assert np.array_equal(y0, ctx.mult(v))
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.fa_csr()
        assert e.value.code == cdfem.ERR_STATE
        # J reads the current u_old: another one changes the operator and drops the Jacobi scale
        if not with_ess and set_name == "A":
            X, info = ctx.solve(v, method="gmres", pc="jacobi", rel_tol=1e-13, max_iter=5000)
            assert info["converged"]
            F2 = copy.copy(F)
            F2.u_old = prm["u_old"] + 0.25
            ctx.nl_set_old(F2.u_old)
            J2 = F2.jacobian(u, eliminated=False)
            assert np.abs(ctx.mult(v) - J2 @ v).max() / scale <= 1e-13
            X2, info = ctx.solve(v, method="gmres", pc="jacobi", rel_tol=1e-13, max_iter=5000)
            assert info["converged"] and np.abs(J2 @ X2 - v).max() <= 1e-10 * np.abs(v).max()


def test_linear_limit_is_pa_setup():
    """a1 = m1 = 0 on an unperturbed (3, 2, 3) p = 2 box (both rules exact): the new kernel against the linear
    operator's, pa_setup(kappa = a0, mass = m0 / dt), Mult and diagonal to 1e-13"""
    m, F, prm, ed = problem("hex2", "A", True, 0.0)
    dt, a0, m0 = 0.1, 2.0, 3.0
    v = np.random.default_rng(9).uniform(-1.0, 1.0, m.nl)
    with context(m, ed) as ctx, context(m, ed) as lin:
        ctx.nl_pa_setup(dt=dt, a0=a0, a1=0.0, m0=m0, m1=0.0)
        ctx.nl_set_old(prm["u_old"])
        ctx.nl_gradient(smooth_u(m, prm))
        lin.pa_setup(kinds=cdfem.DIFFUSION | cdfem.MASS, kappa=a0, mass=m0 / dt)
        assert not lin.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")
        for con in (False, True):
            d = rel_inf(ctx.mult(v, constrained=con), lin.mult(v, constrained=con))
            print(f"constrained={con}: {d:.2e}")
            assert d <= 1e-13
        d = rel_inf(ctx.diagonal(), lin.diagonal())
        print(f"diagonal: {d:.2e}")
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
    assert du <= u_tol and dh <= T.HISTORY_TOL
    assert info["initial_residual"] == pytest.approx(r0, rel=1e-12)
    assert info["final_residual"] == hist["residual"][-1] and hist["update"][-1] == 0.0
    assert info["linear_iterations"] == int(hist["linear_iterations"].sum())
    ru = np.array(ref["update"])
    assert np.abs(hist["update"][:-1] - ru).max() <= 1e-8 * ru.max()


NEWTON_RUNS = [(mn, sn, "gmres") for mn, sn in T.NEWTON_CASES] + [("quad2", "A", "bicgstab")]


@pytest.mark.parametrize("mesh_name,set_name,method", NEWTON_RUNS)
def test_newton(mesh_name, set_name, method):
    """GMRES(30) / BiCGStab + Jacobi at 1e-13: the restatement's iteration count, u to 1e-10, the history"""
    m, F, prm, ed = problem(mesh_name, set_name, True)
    rel_tol = T.NEWTON_CASES[(mesh_name, set_name)]
    ref = ref_newton(mesh_name, set_name, rel_tol)
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        u, info, hist = ctx.newton_solve(prm["u_old"], abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol, **dict(LIN, method=method))
        print(mesh_name, set_name, method, end=" ")
        check_against(ref, u, info, hist, 1e-10)
        assert ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")
        assert np.array_equal(u[ed], prm["u_old"][ed])


def test_newton_cg():
    """the CG driver runs on J too (cdfem_solve accepts it; J is not symmetric, so only the residual is asked for)"""
    m, F, prm, ed = problem("hex2", "A", True)
    u = smooth_u(m, prm)
    b = np.random.default_rng(2).uniform(-1.0, 1.0, m.nl)
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        ctx.nl_gradient(u)
        for pc in ("jacobi", "none"):
            X, info = ctx.solve(b, method="cg", pc=pc, rel_tol=1e-6, max_iter=20)
            assert np.all(np.isfinite(X)) and info["iterations"] > 0
        assert ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")


def test_three_backward_euler_steps():
    """set A on quad2, u_old taken from the previous solution on the device: each step's iteration count equals
    the restatement's, the final state agrees to 1e-10"""
    m, F, prm, ed = problem("quad2", "A", True)
    ur = prm["u_old"].copy()
    try:
        with context(m, ed) as ctx:
            setup(ctx, F, prm)
            du = ctx.to_device(prm["u_old"])
            for step in range(3):
                F.u_old = ur.copy()
                r = F.newton(ur, abs_tol=T.NEWTON_ABS_TOL, rel_tol=T.THREE_STEP_REL_TOL)
                ur = r["u"]
                ctx.nl_set_old(du, where=cdfem.DEVICE)
                info, hist = ctx.newton_solve_device(du, abs_tol=T.NEWTON_ABS_TOL, rel_tol=T.THREE_STEP_REL_TOL, **LIN)
                print(step, info["iterations"], hist["residual"])
                assert info["converged"] and info["iterations"] == r["iterations"]
            u = ctx.from_device(du, m.nl)
            ctx.free(du)
    finally:
        F.u_old = prm["u_old"].copy()
    d = np.linalg.norm(u - ur) / np.linalg.norm(ur)
    print(f"final {d:.2e}")
    assert d <= 1e-10


def test_jacobian_rebuild_freq_2():
    """the Jacobian stays at the older iterate while the Newton loop updates u in place: iteration count and
    history equal the restatement's with the same setting (they differ if the linearisation state aliases u)"""
    m, F, prm, ed = problem("hex2", "A", True)
    ref = ref_newton("hex2", "A", T.FREQ2_REL_TOL, freq=2)
    fresh = ref_newton("hex2", "A", T.NEWTON_CASES[("hex2", "A")])
    assert ref["iterations"] > fresh["iterations"]
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        u, info, hist = ctx.newton_solve(prm["u_old"], rel_tol=T.FREQ2_REL_TOL, jacobian_rebuild_freq=2, **LIN)
        check_against(ref, u, info, hist, 1e-10)


def test_max_iter_1_linear_failure_and_bitwise_repeat():
    """max_iter = 1: CDFEM_ERR_NOT_CONVERGED with the result and the history filled; a linear solve capped at 3
    iterations ends the Newton solve with the iteration named and u unchanged; two identical Newton solves are
    bitwise equal"""
    m, F, prm, ed = problem("hex2", "A", True)
    kw = dict(LIN, rel_tol=T.NEWTON_CASES[("hex2", "A")])
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        u1, info, hist = ctx.newton_solve(prm["u_old"], max_iter=1, **kw)
        assert info["status"] == cdfem.ERR_NOT_CONVERGED and not info["converged"] and info["iterations"] == 1
        assert len(hist["residual"]) == 1 and hist["update"][0] > 0 and hist["linear_iterations"][0] > 0
        assert "Newton" in info["message"] and not np.array_equal(u1, prm["u_old"])
        u, info, hist = ctx.newton_solve(prm["u_old"], **dict(kw, lin_max_iter=3))
        assert info["status"] == cdfem.ERR_NOT_CONVERGED and not info["converged"] and info["iterations"] == 0
        assert "Newton iteration 0" in info["message"] and np.array_equal(u, prm["u_old"])
        ua, ia, ha = ctx.newton_solve(prm["u_old"], **kw)
        ub, ib, hb = ctx.newton_solve(prm["u_old"], **kw)
        assert ia["converged"] and np.array_equal(ua, ub)
        assert np.array_equal(ha["residual"], hb["residual"]) and np.array_equal(ha["update"], hb["update"])
        assert np.array_equal(ha["linear_iterations"], hb["linear_iterations"])


@pytest.mark.parametrize("perturb", [0.2, 0.0], ids=["perturbed", "box"])
def test_structured_context_takes_no_fast_path(perturb):
    """a context with set_structured (where the linear operator runs the brick kernels, the patch-buffer Krylov
    sources and the uniform-box tables): while J(u) is current none of them runs, so residual, Mult, diagonal, a
    linear solve per method and the Newton solve equal the unstructured context's bitwise; and the other way
    round, a pa_setup + solve after the Newton solve equals a fresh context's, as does nl_pa_setup + Newton after
    a pa_setup + solve"""
    m, F, prm, ed = problem("hex2", "A", True, perturb)
    u = smooth_u(m, prm)
    v = np.random.default_rng(11).uniform(-1.0, 1.0, m.nl)
    kw = dict(LIN, rel_tol=T.NEWTON_CASES[("hex2", "A")])

    def nonlinear(ctx):
        setup(ctx, F, prm)
        out = [ctx.nl_residual(u)]
        ctx.nl_gradient(u)
        out += [ctx.mult(v), ctx.mult(v, constrained=True), ctx.diagonal()]
        for method in ("gmres", "bicgstab", "cg"):
            out.append(ctx.solve(v, method=method, pc="jacobi", rel_tol=1e-10, max_iter=40)[0])
            assert ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")
        un, info, hist = ctx.newton_solve(prm["u_old"], **kw)
        assert info["converged"]
        return out + [un, hist["residual"], hist["update"]]

    def linear(ctx):
        ctx.pa_setup(kinds=cdfem.DIFFUSION | cdfem.MASS, kappa=0.1, mass=1.0)
        out = [ctx.mult(v, constrained=True), ctx.diagonal()]
        for method in ("cg", "gmres"):
            out.append(ctx.solve(v, method=method, pc="jacobi", rel_tol=1e-12, max_iter=2000)[0])
        assert not ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")
        return out

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

    with context(m, ed) as plain:
        ref_nl = nonlinear(plain)
    with context(m, ed, (3, 2, 3)) as ctx:
        ref_lin = linear(ctx)
    with context(m, ed, (3, 2, 3)) as ctx:
        assert same(nonlinear(ctx), ref_nl)          # structured, nonlinear first
        assert same(linear(ctx), ref_lin)            # back to the linear operator
        assert same(nonlinear(ctx), ref_nl)          # forward again, after a pa_setup + solve
    with context(m, ed) as plain:
        lin_plain = linear(plain)
        assert same(nonlinear(plain), ref_nl)
        assert same(linear(plain), lin_plain)


def test_status_codes():
    quad = cdfem.box_mesh(2, (3, 2), 2)
    co = dict(dt=0.1, a0=1.0, a1=0.5, m0=1.0, m1=0.5)
    with cdfem.Context(0).upload_mesh(cdfem.kuhn_mesh(2, 3, 2)) as ctx:
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_pa_setup(**co)
        assert e.value.code == cdfem.ERR_UNSUPPORTED
    for mesh in (cdfem.box_mesh(3, 2, 3), cdfem.box_mesh(2, 2, 4)):
        with cdfem.Context(0).upload_mesh(mesh) as ctx:
            with pytest.raises(cdfem.CdfemError) as e:
                ctx.nl_pa_setup(**co)
            assert e.value.code == cdfem.ERR_UNSUPPORTED
    u0 = np.ones(quad.nl)
    with cdfem.Context(0).upload_mesh(quad) as ctx:
        for call in (lambda: ctx.nl_residual(u0), lambda: ctx.nl_gradient(u0), lambda: ctx.newton_solve(u0),
                     lambda: ctx.nl_set_old(u0)):
            with pytest.raises(cdfem.CdfemError) as e:
                call()
            assert e.value.code == cdfem.ERR_STATE
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_pa_setup(**dict(co, dt=0.0))
        assert e.value.code == cdfem.ERR_ARG
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_setup(**co)
        assert e.value.code == cdfem.ERR_UNSUPPORTED  # the assembled form stays simplex-only
        ctx.nl_pa_setup(**co)
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.newton_solve(u0, pc="ilu", raise_on_fail=True)
        assert e.value.code == cdfem.ERR_UNSUPPORTED
        # a context with a two-rank host communicator is refused
        ctx.comm_init_host(0, 2, lambda a: None, lambda *a: None)
        for call in (lambda: ctx.nl_pa_setup(**co), lambda: ctx.newton_solve(u0, pc="jacobi")):
            with pytest.raises(cdfem.CdfemError) as e:
                call()
            assert e.value.code == cdfem.ERR_UNSUPPORTED
