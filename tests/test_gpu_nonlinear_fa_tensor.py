"""The nonlinear heat form on quads and hexes with an assembled Jacobian (cdfem_nl_fa_setup;
csrc/nl_fa_tensor.hip k_nl_tensor_point / k_nl_tensor_elem, then the full assembly's gather, elimination, SELL
fill, SpMV and ILU(0)) against the numpy restatement tests/nonlinear_tensor_ref.py and against the matrix-free
path of cdfem_nl_pa_setup.

Meshes, sets and tolerances are tests/test_gpu_nonlinear_pa.py's: nonlinear_tensor_ref.MESHES with perturb = 0.2
(at most 60 elements: one Ee block, its last lanes padding), sets A and B (B on the mesh scaled by 0.01, u ~ 300),
essential dofs none or the x = 1 face; 1e-13 of max |J| for CSR values and the diagonal, 1e-13 of max |J| |v|_inf
for Mult, 1e-10 relative L2 for two solves both taken to 1e-13, residual histories where the restatement's norm
exceeds 1e-6 r0 within nonlinear_tensor_ref.HISTORY_TOL.  GMRES + ILU(0) on J(u) is compared as
tests/test_gpu_fa_tensor.py compares it on the linear operator: 1e-11 after five fixed steps, converged solves
1e-8 with iteration counts within +-1.

Newton with jacobian_rebuild_freq = 2 runs at the rel_tol of nonlinear_tensor_ref.NEWTON_CASES too.  The
restatement's rn / r0 there (direct solves): quad2 A .. 8.0e-6, 1.6e-8 (1e-7); quad3 B .. 4.0e-7, 2.5e-10 (1e-8);
hex1 B .. 8.9e-4, 2.4e-5, 1.2e-10 (1e-4); hex2 A .. 5.0e-6, 1.0e-8 (1e-7); hex2 B .. 1.7e-5, 1.3e-10 (1e-6): no
iterate within a factor 4 of its threshold, and every absolute norm at the stop at least 17 times abs_tol."""
import copy
import functools

import numpy as np
import pytest

import cdfem
import nonlinear_tensor_ref as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ALL_MESHES = ["quad1", "quad2", "quad3", "hex1", "hex2", "hex2L"]
LIN = dict(method="gmres", lin_rel_tol=1e-13, lin_abs_tol=0.0, lin_max_iter=50000)


@functools.lru_cache(maxsize=None)
def problem(mesh_name, set_name, ess):
    """mesh on the set's domain, restatement form with u_old and the load, the set, the essential dofs"""
    return T.problem(mesh_name, set_name, ess=ess)


@functools.lru_cache(maxsize=None)
def ref_newton(mesh_name, set_name, rel_tol, freq=1):
    m, F, prm, ed = problem(mesh_name, set_name, True)
    F.u_old = prm["u_old"].copy()
    return F.newton(prm["u_old"].copy(), abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol, jacobian_rebuild_freq=freq)


@functools.lru_cache(maxsize=None)
def ref_jacobian(mesh_name, set_name, ess):
    """the restatement's J(u) at the smooth state, plain and eliminated, computed once"""
    m, F, prm, ed = problem(mesh_name, set_name, ess)
    F.u_old = prm["u_old"].copy()
    J = F.jacobian(smooth_u(m, prm), eliminated=False)
    return J, F.eliminate(J)


def smooth_u(m, prm):
    """a smooth non-polynomial state, different from u_old"""
    xyz = T.dof_coords(m) / prm["scale"]
    amp = 0.3 if prm["scale"] == 1.0 else 2.0
    return prm["u_old"] + amp * np.cos(2.0 * xyz[:, 0] + xyz[:, 1]) * np.exp(0.5 * xyz[:, -1])


def context(m, ess):
    mm = copy.copy(m)
    mm.ess = np.asarray(ess, dtype=np.int32)
    return cdfem.Context(0).upload_mesh(mm)


def setup(ctx, F, prm, assembled=True):
    (ctx.nl_fa_setup if assembled else ctx.nl_pa_setup)(**prm["coeffs"])
    ctx.nl_set_old(prm["u_old"])
    ctx.nl_set_rhs(F.g)


@pytest.mark.parametrize("with_ess", [False, True], ids=["free", "ess"])
@pytest.mark.parametrize("set_name", ["A", "B"])
@pytest.mark.parametrize("name", ALL_MESHES)
def test_csr_and_operator_parity(name, set_name, with_ess):
    """after nl_gradient(u): fa_csr() is the restatement's CSR in pattern and values, plain and eliminated; Mult
    (constrained 0 / 1 / 2) and the diagonal act on it; the SpMV is the apply; a second nl_gradient gives the
    same bits; the residual is still the matrix-free kernel's"""
    m, F, prm, ed = problem(name, set_name, with_ess)
    u = smooth_u(m, prm)
    J, Jc = ref_jacobian(name, set_name, with_ess)
    jmax = np.abs(J.data).max()
    v = np.random.default_rng(5).uniform(-1.0, 1.0, m.nl)
    scale = jmax * np.abs(v).max()
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.fa_csr()
        assert e.value.code == cdfem.ERR_STATE  # nothing assembled yet
        ctx.nl_gradient(u)
        rp, cols, vals = ctx.fa_csr()
        np.testing.assert_array_equal(rp, J.indptr)
        np.testing.assert_array_equal(cols, J.indices)
        dv = np.abs(vals - J.data).max() / jmax
        _, _, cvals = ctx.fa_csr(constrained=True)
        dc = np.abs(cvals - Jc.data).max() / jmax
        y0, y2, yc = ctx.mult(v), ctx.mult(v, constrained=2), ctx.mult(v, constrained=True)
        dm = np.abs(y0 - J @ v).max() / scale
        ve = v.copy()
        ve[ed] = 0.0
        yr = Jc @ ve
        yr[ed] = v[ed]
        dmc = np.abs(yc - yr).max() / scale
        dd = np.abs(ctx.diagonal() - J.diagonal()).max() / jmax
        print(f"{name} {set_name} ess={with_ess}: csr {dv:.2e} {dc:.2e} mult {dm:.2e} {dmc:.2e} diag {dd:.2e}")
        assert max(dv, dc, dm, dmc, dd) <= 1e-13
        assert np.array_equal(y0, y2) and np.array_equal(yc[ed], v[ed])
        assert not ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")  # the SpMV
        ctx.nl_gradient(u)
        np.testing.assert_array_equal(ctx.fa_csr()[2], vals)
        np.testing.assert_array_equal(ctx.fa_csr(constrained=True)[2], cvals)
        R = ctx.nl_residual(u)
        assert np.abs(R - F.residual(u)).max() <= 1e-13 * np.abs(F.residual(u)).max()


@pytest.mark.parametrize("name", ["quad2", "hex2"])
def test_snapshot_and_cross_check(name):
    """the assembled J keeps the u_old it was assembled with until the next nl_gradient, the matrix-free J reads
    the current one; at the same u, u_old and v the two Mults agree to 1e-13 of max |J| |v|_inf"""
    m, F, prm, ed = problem(name, "A", True)
    u = smooth_u(m, prm)
    J, _ = ref_jacobian(name, "A", True)
    F2 = copy.copy(F)
    F2.u_old = prm["u_old"] + 0.25
    J2 = F2.jacobian(u, eliminated=False)
    v = np.random.default_rng(6).uniform(-1.0, 1.0, m.nl)
    scale = np.abs(J.data).max() * np.abs(v).max()
    assert np.abs(J2 @ v - J @ v).max() > 1e-6 * scale  # the other u_old is another operator
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        ctx.nl_gradient(u)
        ya = ctx.mult(v)
        ctx.nl_set_old(F2.u_old)
        assert np.array_equal(ctx.mult(v), ya)
        x1, i1 = ctx.solve(v, method="gmres", pc="ilu", rel_tol=1e-12, max_iter=500)
        assert i1["converged"]
        ctx.nl_gradient(u)
        ya2 = ctx.mult(v)
        assert np.abs(ya2 - J2 @ v).max() <= 1e-13 * scale and not np.array_equal(ya2, ya)
        # the matrix-free path on the same context: the same sequence changes the operator
        setup(ctx, F, prm, assembled=False)
        ctx.nl_gradient(u)
        yf = ctx.mult(v)
        d = np.abs(yf - ya).max() / scale
        print(f"{name}: assembled against matrix-free {d:.2e}")
        assert d <= 1e-13
        ctx.nl_set_old(F2.u_old)
        yf2 = ctx.mult(v)
        assert not np.array_equal(yf2, yf) and np.abs(yf2 - ya2).max() <= 1e-13 * scale


@pytest.mark.parametrize("name,set_name", [("quad3", "B"), ("hex2L", "A")])
def test_gmres_ilu_parity(name, set_name):
    """GMRES + ILU(0) on J(u) against the oracle's ILU(0) of the restatement's eliminated CSR"""
    m, F, prm, ed = problem(name, set_name, True)
    u = smooth_u(m, prm)
    _, Jc = ref_jacobian(name, set_name, True)
    Ac = O.csr_from_scipy(Jc)
    Fo = O.ilu0(Ac)
    b = np.random.default_rng(11).uniform(-1.0, 1.0, m.nl)
    tol = dict(rel_tol=1e-10, abs_tol=1e-12, max_iter=2000)
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        ctx.nl_gradient(u)
        xo, io = O.gmres_ilu(Ac, b, Fo, restart=3, rtol=0.0, atol=0.0, max_it=5)
        xg, ig = ctx.solve(b, method="gmres", pc="ilu", restart=3, rel_tol=0.0, abs_tol=0.0, max_iter=5)
        assert io["iterations"] == ig["iterations"] == 5
        err = np.linalg.norm(xg - xo) / np.linalg.norm(xo)
        print(f"5 fixed steps {err:.3e}")
        assert err <= 1e-11
        xo, io = O.gmres_ilu(Ac, b, Fo, restart=30, rtol=1e-10, atol=1e-12, max_it=2000)
        xg, ig = ctx.solve(b, method="gmres", pc="ilu", restart=30, **tol)
        print(f"iterations ilu {ig['iterations']} (oracle {io['iterations']})")
        assert io["converged"] and ig["converged"] and abs(io["iterations"] - ig["iterations"]) <= 1
        assert np.linalg.norm(xg - xo) <= 1e-8 * np.linalg.norm(xo)
        _, ij = ctx.solve(b, method="gmres", pc="jacobi", restart=30, **tol)
        print(f"iterations jacobi {ij['iterations']}")
        assert ij["converged"] and ig["iterations"] < ij["iterations"]
        xg2, _ = ctx.solve(b, method="gmres", pc="ilu", restart=30, **tol)
        np.testing.assert_array_equal(xg, xg2)
        for method, pc in (("bicgstab", "ilu"), ("bicgstab", "none"), ("cg", "jacobi")):
            xb, ib = ctx.solve(b, method=method, pc=pc, rel_tol=1e-10, abs_tol=1e-12, max_iter=20 if method == "cg" else 2000)
            assert np.all(np.isfinite(xb)) and ib["iterations"] > 0      # CG runs (J is not symmetric: no more asked)
            if method != "cg":
                assert ib["converged"] and np.linalg.norm(xb - xo) <= 1e-8 * np.linalg.norm(xo)


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


@pytest.mark.parametrize("freq", [1, 2])
@pytest.mark.parametrize("pc", ["ilu", "jacobi"])
@pytest.mark.parametrize("mesh_name,set_name", list(T.NEWTON_CASES))
def test_newton_history(mesh_name, set_name, pc, freq):
    """GMRES(30) + ILU(0) / Jacobi at 1e-13, the Jacobian rebuilt every or every second iteration: the
    restatement's iteration count, u to 1e-10, the residual history"""
    m, F, prm, ed = problem(mesh_name, set_name, True)
    rel_tol = T.NEWTON_CASES[(mesh_name, set_name)]
    ref = ref_newton(mesh_name, set_name, rel_tol, freq)
    with context(m, ed) as ctx:
        setup(ctx, F, prm)
        u, info, hist = ctx.newton_solve(prm["u_old"], abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol,
                                         jacobian_rebuild_freq=freq, pc=pc, **LIN)
        print(mesh_name, set_name, pc, freq, end=" ")
        check_against(ref, u, info, hist, 1e-10)
        assert not ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")
        assert np.array_equal(u[ed], prm["u_old"][ed])


@pytest.mark.parametrize("mesh_name,set_name", list(T.NEWTON_CASES))
def test_newton_solution_against_matrix_free(mesh_name, set_name):
    """the assembled path with ILU(0) and with Jacobi against the matrix-free path, all at the same tolerances:
    the final u within 1e-10 relative L2; the linear iteration counts are printed, not asserted"""
    m, F, prm, ed = problem(mesh_name, set_name, True)
    kw = dict(abs_tol=T.NEWTON_ABS_TOL, rel_tol=T.NEWTON_CASES[(mesh_name, set_name)], **LIN)
    with context(m, ed) as ctx:
        setup(ctx, F, prm, assembled=False)
        uf, inf_, _ = ctx.newton_solve(prm["u_old"], pc="jacobi", **kw)
        setup(ctx, F, prm)
        ui, ini, _ = ctx.newton_solve(prm["u_old"], pc="ilu", **kw)
        uj, inj, _ = ctx.newton_solve(prm["u_old"], pc="jacobi", **kw)
    assert inf_["converged"] and ini["converged"] and inj["converged"]
    di, dj = (np.linalg.norm(x - uf) / np.linalg.norm(uf) for x in (ui, uj))
    print(f"{mesh_name} {set_name}: ilu {di:.2e} jacobi {dj:.2e}; linear iterations ilu {ini['linear_iterations']} "
          f"jacobi {inj['linear_iterations']} matrix-free jacobi {inf_['linear_iterations']}")
    assert ini["iterations"] == inj["iterations"] == inf_["iterations"]
    assert di <= 1e-10 and dj <= 1e-10


def test_switching_is_bitwise():
    """nl_fa_setup -> nl_pa_setup -> nl_fa_setup, and nl_fa_setup -> fa_setup -> a linear solve -> nl_fa_setup:
    every stage reproduces its first results bitwise; after nl_pa_setup the ILU preconditioner is refused again"""
    m, F, prm, ed = problem("hex2", "A", True)
    u = smooth_u(m, prm)
    v = np.random.default_rng(12).uniform(-1.0, 1.0, m.nl)
    kw = dict(abs_tol=T.NEWTON_ABS_TOL, rel_tol=T.NEWTON_CASES[("hex2", "A")], **LIN)

    def assembled(ctx):
        setup(ctx, F, prm)
        out = [ctx.nl_residual(u)]
        ctx.nl_gradient(u)
        out += [ctx.fa_csr()[2], ctx.fa_csr(constrained=True)[2], ctx.mult(v), ctx.mult(v, constrained=True), ctx.diagonal()]
        out.append(ctx.solve(v, method="gmres", pc="ilu", rel_tol=1e-10, max_iter=200)[0])
        un, info, hist = ctx.newton_solve(prm["u_old"], pc="ilu", **kw)
        assert info["converged"]
        return out + [un, hist["residual"], hist["update"]]

    def matrix_free(ctx):
        setup(ctx, F, prm, assembled=False)
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.fa_csr()
        assert e.value.code == cdfem.ERR_STATE  # the assembled Jacobian is dropped
        ctx.nl_gradient(u)
        assert ctx.kernel_name(cdfem.K_APPLY).startswith("k_nl_tensor")
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.solve(v, method="gmres", pc="ilu", rel_tol=1e-10, max_iter=200)
        assert e.value.code == cdfem.ERR_UNSUPPORTED
        un, info, hist = ctx.newton_solve(prm["u_old"], pc="jacobi", **kw)
        assert info["converged"]
        return [ctx.mult(v), ctx.diagonal(), un, hist["residual"]]

    def linear(ctx):
        ctx.fa_setup(kinds=cdfem.DIFFUSION | cdfem.CONVECTION | cdfem.MASS, kappa=0.1, conv=(1.0, -2.0, 0.5), mass=1.0)
        _, B = ctx.form_linear_system(np.zeros(m.nl), v)
        x, info = ctx.solve(B, method="gmres", pc="ilu", rel_tol=1e-10, abs_tol=1e-12, max_iter=500)
        assert info["converged"]
        return [ctx.fa_csr(True)[2], ctx.mult(v), x]

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))

    with context(m, ed) as ctx:
        a0 = assembled(ctx)
        f0 = matrix_free(ctx)
        assert same(assembled(ctx), a0)
        l0 = linear(ctx)
        assert same(assembled(ctx), a0)
        assert same(matrix_free(ctx), f0)
        assert same(linear(ctx), l0)
    with context(m, ed) as fresh:
        assert same(linear(fresh), l0)
        assert same(matrix_free(fresh), f0)


def test_status_codes():
    quad = cdfem.box_mesh(2, (3, 2), 2)
    co = dict(dt=0.1, a0=1.0, a1=0.5, m0=1.0, m1=0.5)
    with cdfem.Context(0).upload_mesh(cdfem.kuhn_mesh(2, 3, 2)) as ctx:
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_fa_setup(**co)
        assert e.value.code == cdfem.ERR_UNSUPPORTED
    for mesh in (cdfem.box_mesh(3, 2, 3), cdfem.box_mesh(2, 2, 4)):
        with cdfem.Context(0).upload_mesh(mesh) as ctx:
            with pytest.raises(cdfem.CdfemError) as e:
                ctx.nl_fa_setup(**co)
            assert e.value.code == cdfem.ERR_UNSUPPORTED
    u0 = np.ones(quad.nl)
    with cdfem.Context(0).upload_mesh(quad) as ctx:
        for call in (lambda: ctx.nl_gradient(u0), lambda: ctx.nl_residual(u0), lambda: ctx.newton_solve(u0)):
            with pytest.raises(cdfem.CdfemError) as e:
                call()
            assert e.value.code == cdfem.ERR_STATE
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_fa_setup(**dict(co, dt=0.0))
        assert e.value.code == cdfem.ERR_ARG
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.nl_gradient(u0)
        assert e.value.code == cdfem.ERR_STATE  # a refused setup sets nothing up
        ctx.nl_fa_setup(**co)
        assert ctx.rule_size(cdfem.RULE_NONLINEAR) == 16
        ctx.nl_gradient(u0)
        assert ctx.fa_csr()[0][-1] > 0
        # a context with a two-rank host communicator is refused
        ctx.comm_init_host(0, 2, lambda a: None, lambda *a: None)
        for call in (lambda: ctx.nl_fa_setup(**co), lambda: ctx.nl_gradient(u0)):
            with pytest.raises(cdfem.CdfemError) as e:
                call()
            assert e.value.code == cdfem.ERR_UNSUPPORTED
