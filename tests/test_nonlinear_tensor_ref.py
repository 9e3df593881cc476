"""Pins tests/nonlinear_tensor_ref.py, the numpy restatement of the nonlinear heat form on quads and hexes, before
tests/test_gpu_nonlinear_pa.py compares the matrix-free HIP path with it.  No GPU.  Every test prints the
figures it asserts."""
import numpy as np
import pytest

import cdfem
import nonlinear_tensor_ref as T
from oracle import oracle as O

SPACES = ["quad1", "quad2", "quad3", "hex1", "hex2"]
_PROBLEM = {}


def problem(mesh_name, set_name, ess):
    key = (mesh_name, set_name, ess)
    if key not in _PROBLEM:
        _PROBLEM[key] = T.problem(mesh_name, set_name, ess=ess)
    return _PROBLEM[key]


def smooth_u(m, prm):
    """a smooth non-polynomial state, different from u_old, on the set's domain"""
    xyz = T.dof_coords(m) / prm["scale"]
    amp = 0.3 if prm["scale"] == 1.0 else 2.0
    return prm["u_old"] + amp * np.cos(2.0 * xyz[:, 0] + xyz[:, 1]) * np.exp(0.5 * xyz[:, -1])


def test_rule_sizes_and_dof_coordinates():
    """p + 2 points per direction on quads, p + 3 on hexes; the restatement's GLL lattice, mapped, lands on the
    mesh generator's dof coordinates"""
    assert [T.points_1d(2, p) for p in (1, 2, 3)] == [3, 4, 5] and [T.points_1d(3, p) for p in (1, 2)] == [4, 5]
    for name in SPACES:
        m = T.build_mesh(name)
        assert np.abs(T.dof_coords(m) - m.dof_xyz).max() <= 4e-16, name
        assert O.rule_npts(0, m.dim, m.order) + 1 == T.points_1d(m.dim, m.order)  # one more than the operator rule


LINEAR_CASES = [(2, (5, 3), 2), (2, (3, 3), 3), (2, (3, 3), 1), (3, (2, 2, 2), 1), (3, (2, 2, 2), 2), (3, (3, 2, 3), 2)]


@pytest.mark.parametrize("dim,n,p", LINEAR_CASES)
def test_linear_limit(dim, n, p):
    """a1 = m1 = 0 against oracle.fa_assemble(kappa = a0, s = m0 / dt): on the unperturbed box the form's rule
    agrees to rounding (both rules are exact there); on the perturbed box only the oracle's operator count
    (p + 1 / p + 2 points) does, and the form's own rule differs at quadrature level, which shows the rule in use"""
    dt, a0, m0 = 0.1, 1.3, 0.7
    nop = O.rule_npts(0, dim, p)
    assert nop == (p + 1 if dim == 2 else p + 2)

    def diff(perturb, nq1):
        m = O.BoxMesh(dim, n, p, perturb=perturb)
        A = O.fa_assemble(m, kappa=a0, s=m0 / dt, kinds=O.DIFFUSION | O.MASS).to_scipy()
        F = T.TensorHeatForm(m, dt=dt, a0=a0, a1=0.0, m0=m0, m1=0.0, nq1=nq1)
        return np.abs(F.jacobian(np.zeros(m.nl), eliminated=False) - A).max() / np.abs(A).max()

    flat, bent_op, bent = diff(0.0, None), diff(0.2, nop), diff(0.2, None)
    print(f"dim {dim} n {n} p {p}: unperturbed {flat:.2e}, perturbed at the operator count {bent_op:.2e}, "
          f"at the form's {bent:.2e}")
    assert flat <= 1e-13 and bent_op <= 1e-13 and bent > 1e-8


@pytest.mark.parametrize("with_ess", [False, True], ids=["free", "ess"])
@pytest.mark.parametrize("set_name", ["A", "B"])
@pytest.mark.parametrize("name", SPACES)
def test_jacobian_identity(name, set_name, with_ess):
    """R is quadratic in u, so R(u + v / 2) - R(u - v / 2) = J(u) v to rounding: 1e-12 of max |J v|.  With
    essential dofs v vanishes there (R is zero on those rows, and J v would return v)."""
    m, F, prm, ed = problem(name, set_name, with_ess)
    u = smooth_u(m, prm)
    v = np.random.default_rng(3).uniform(-1.0, 1.0, m.nl)
    v[ed] = 0.0
    cd = F.residual(u + 0.5 * v) - F.residual(u - 0.5 * v)
    jv = F.jacobian(u) @ v
    err = np.abs(cd - jv).max() / np.abs(jv).max()
    print(f"{name} {set_name} ess={with_ess}: {err:.2e}")
    assert err <= 1e-12
    if with_ess:
        assert len(ed) > 0 and np.all(F.residual(u)[ed] == 0.0)
        Jc = F.jacobian(u).toarray()
        assert np.array_equal(Jc[ed][:, ed], np.eye(len(ed))) and not Jc[ed].sum() - len(ed) and not Jc[:, ed].sum() - len(ed)


@pytest.mark.parametrize("name", ["quad3", "hex2"])
def test_rounding_level(name):
    """the double-precision residual against the same formulas in long double on set B (u ~ 300 on a domain 0.01
    wide): at most 1e-13, so the GPU test's 1e-13 is 10 times the restatement's own rounding or more"""
    m, F, prm, _ = problem(name, "B", False)
    _, Fx, _, _ = T.problem(name, "B", ess=False, dtype=np.longdouble)
    u = smooth_u(m, prm)
    R, Rx = F.residual(u), Fx.residual(u)
    err = float(np.abs(R - Rx).max() / np.abs(Rx).max())
    print(f"{name}: {err:.2e}")
    assert err <= 1e-14 * 10


def assert_decisive(r, abs_tol, rel_tol):
    """no iterate's rn / r0 within a factor 3 of rel_tol, none within a factor 3 of abs_tol; only the last one
    converged"""
    for k, rn in enumerate(r["residual"]):
        rel = rn / r["r0"]
        assert not rel_tol / 3 <= rel <= 3 * rel_tol, (k, rel)
        assert not abs_tol / 3 <= rn <= 3 * abs_tol, (k, rn)
        assert (rn < abs_tol or rel < rel_tol) == (k == r["iterations"] and r["converged"])


@pytest.mark.parametrize("mesh_name,set_name", list(T.NEWTON_CASES))
def test_newton_cases(mesh_name, set_name):
    """every Newton case of the GPU test: converged, decisively at every iterate with the case's rel_tol; the
    restatement driven by the oracle's GMRES(30) + Jacobi at 1e-13 takes the same iterations, and its residual
    norms above 1e-6 r0 stay within the measured spread nonlinear_tensor_ref.HISTORY_SPREAD"""
    m, F, prm, ed = problem(mesh_name, set_name, True)
    rel_tol = T.NEWTON_CASES[(mesh_name, set_name)]
    r = F.newton(F.u_old.copy(), abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol)
    res, r0 = np.array(r["residual"]), r["r0"]
    print(mesh_name, set_name, r["iterations"], res / r0, res)
    assert r["converged"] and 3 <= r["iterations"] <= 5
    assert_decisive(r, T.NEWTON_ABS_TOL, rel_tol)
    g = F.newton(F.u_old.copy(), abs_tol=T.NEWTON_ABS_TOL, rel_tol=rel_tol, linear="gmres_jacobi", lin_max_it=50000)
    assert g["iterations"] == r["iterations"] and not g["linear_failed"]
    gr = np.array(g["residual"])
    sel = res > 1e-6 * r0
    spread = (np.abs(gr[sel] - res[sel]) / res[sel]).max()
    print(f"spread {spread:.2e}, linear iterations {g['linear_iterations']}")
    assert spread <= T.HISTORY_SPREAD
    assert np.linalg.norm(g["u"] - r["u"]) <= 1e-11 * np.linalg.norm(r["u"])


def test_newton_rebuild():
    """hex2, set A with the Jacobian kept for two iterations: more iterations than with a fresh one, decisive at
    every iterate"""
    m, F, prm, ed = problem("hex2", "A", True)
    r1 = F.newton(F.u_old.copy(), rel_tol=T.NEWTON_CASES[("hex2", "A")])
    r2 = F.newton(F.u_old.copy(), rel_tol=T.FREQ2_REL_TOL, jacobian_rebuild_freq=2)
    print(r2["iterations"], np.array(r2["residual"]) / r2["r0"])
    assert r2["converged"] and r2["iterations"] > r1["iterations"]
    assert_decisive(r2, T.NEWTON_ABS_TOL, T.FREQ2_REL_TOL)


def test_three_steps():
    """three backward-Euler steps of set A on quad2, each from the last solution: decisive at every iterate of
    every step with nonlinear_tensor_ref.THREE_STEP_REL_TOL"""
    m, F, prm, ed = T.problem("quad2", "A", ess=True)
    u = F.u_old.copy()
    its = []
    for step in range(3):
        F.u_old = u.copy()
        r = F.newton(u, abs_tol=T.NEWTON_ABS_TOL, rel_tol=T.THREE_STEP_REL_TOL)
        print(step, r["iterations"], np.array(r["residual"]) / r["r0"], r["residual"])
        assert r["converged"]
        assert_decisive(r, T.NEWTON_ABS_TOL, T.THREE_STEP_REL_TOL)
        u = r["u"]
        its.append(r["iterations"])
    assert its == [4, 3, 3]


def test_binding_surface():
    """the header declares the new entry point, the library exports it, the binding declares its signature"""
    assert "cdfem_nl_pa_setup" in cdfem.exported_symbols_from_header()
    f = cdfem.lib().cdfem_nl_pa_setup
    assert f.argtypes is not None and f.restype is not None
    assert callable(cdfem.Context.nl_pa_setup) and cdfem.lib().cdfem_abi_version() == 1
