"""Pins tests/nonlinear_ref.py, the numpy restatement of the nonlinear heat form, its boundary load and the
Newton loop, before tests/test_gpu_nonlinear.py compares the HIP path with it.  No GPU.

The last test lists the new C-ABI symbols and checks the header and the binding's declarations for them."""
import types

import numpy as np
import pytest

import cdfem
import nonlinear_ref as N
from oracle import oracle as O

SPACES = ["tri1", "tri2", "tri3", "tet1", "tet2"]
_MESH = {}


def mesh(name):
    if name not in _MESH:
        _MESH[name] = N.build_mesh(name)
    return _MESH[name]


def smooth_u(m, prm):
    """a smooth non-polynomial state, different from u_old"""
    xyz = N.dof_coords(m)
    return prm["u_old"] + 0.3 * np.cos(2.0 * xyz[:, 0] + xyz[:, 1]) * np.exp(0.5 * xyz[:, -1])


def oracle_mesh(m):
    return types.SimpleNamespace(dim=m.dim, p=m.order, ne=m.ne, verts=m.verts, dofmap=m.dofmap, nl=m.nl)


def test_nodes_are_the_spaces_nodes():
    """the restatement's node set, mapped to the mesh, lands on the mesh generator's dof coordinates"""
    for name in SPACES:
        m = mesh(name)
        assert np.abs(N.dof_coords(m) - m.dof_xyz).max() <= 4e-16


@pytest.mark.parametrize("name", SPACES)
def test_linear_limit(name):
    """a1 = m1 = 0: J = (m0 / dt) M + a0 K of the oracle's assembly (every rule involved is exact there), and
    R(u) = J (u - u_old) + a0 K u_old.  1e-12 of the largest entry."""
    m = mesh(name)
    dt, a0, m0 = 0.1, 2.0, 3.0
    F = N.HeatForm(m, dt=dt, a0=a0, a1=0.0, m0=m0, m1=0.0)
    F.u_old = N.set_a(m)["u_old"]
    u = smooth_u(m, N.set_a(m))
    om = oracle_mesh(m)
    A = O.fa_assemble_simplex(om, kappa=a0, s=m0 / dt, kinds=O.DIFFUSION | O.MASS).to_scipy()
    K = O.fa_assemble_simplex(om, kappa=1.0, kinds=O.DIFFUSION).to_scipy()
    J = F.jacobian(u, eliminated=False)
    dJ = np.abs((A - J)).max() / np.abs(J.data).max()
    R, Rl = F.residual(u), J @ (u - F.u_old) + a0 * (K @ F.u_old)
    dR = np.abs(R - Rl).max() / np.abs(R).max()
    print(f"{name}: dJ {dJ:.2e} dR {dR:.2e}")
    assert dJ <= 1e-12 and dR <= 1e-12


@pytest.mark.parametrize("with_ess", [False, True], ids=["free", "ess"])
@pytest.mark.parametrize("name", SPACES)
def test_central_difference(name, with_ess):
    """R is quadratic in u, so R(u + v / 2) - R(u - v / 2) = J(u) v to rounding: 1e-12 relative.  With
    essential dofs v vanishes there (R is zero on those rows, and J v would return v)."""
    m = mesh(name)
    prm = N.set_a(m)
    F = N.HeatForm(m, ess=m.ess if with_ess else (), **prm["coeffs"])
    F.u_old = prm["u_old"]
    u = smooth_u(m, prm)
    v = np.random.default_rng(3).uniform(-1.0, 1.0, m.nl)
    if with_ess:
        v[m.ess] = 0.0
    cd = F.residual(u + 0.5 * v) - F.residual(u - 0.5 * v)
    jv = F.jacobian(u) @ v
    err = np.abs(cd - jv).max() / np.abs(jv).max()
    print(f"{name} ess={with_ess}: {err:.2e}")
    assert err <= 1e-12
    if with_ess:
        assert np.all(F.residual(u)[m.ess] == 0.0)
        Jc = F.jacobian(u).toarray()
        e = np.asarray(m.ess)
        assert np.array_equal(Jc[e][:, e], np.eye(len(e))) and not Jc[e].sum() - len(e) and not Jc[:, e].sum() - len(e)


def _rule_diff(name, rule):
    m = mesh(name)
    prm = N.set_a(m)
    u = smooth_u(m, prm)
    out = []
    for r in (None, rule):
        F = N.HeatForm(m, rule=r, **prm["coeffs"])
        F.u_old = prm["u_old"]
        out.append((F.residual(u), F.jacobian(u, eliminated=False).data))
    (R1, J1), (R2, J2) = out
    return np.abs(R1 - R2).max() / np.abs(R1).max(), np.abs(J1 - J2).max() / np.abs(J1).max()


@pytest.mark.parametrize("name", ["tri1", "tri2", "tet1", "tet2"])
def test_rule_order_is_exact_up_to_p2(name):
    """The integrands have degree 3p (the mass term m(u) (u - u_old) phi_i, and its derivative) and 3p - 2 (the
    diffusion terms), so the rule of order 2p + 2 is exact for p <= 2: a collapsed-Gauss rule exact to degree
    2p + 5 gives the same R and J to 1e-12.
    The issue that introduced this form listed P2 tetrahedra among the spaces where the two rules must differ;
    there 3p = 6 = 2p + 2, the order-6 rule is exact, and the measured difference is 1.7e-15 (R), 1.3e-15 (J).
    test_rule_order_is_pinned checks against the next lower rule instead, which does pin order 6 on them."""
    m = mesh(name)
    dR, dJ = _rule_diff(name, O.simplex_rule(m.dim, m.order + 4))  # exact to degree 2 (p + 4) - dim >= 2p + 5
    print(f"{name}: dR {dR:.2e} dJ {dJ:.2e}")
    assert dR <= 1e-12 and dJ <= 1e-12


@pytest.mark.parametrize("name,other", [("tri3", "higher"), ("tri3", "lower"), ("tet2", "lower"), ("tri2", "lower")])
def test_rule_order_is_pinned(name, other):
    """P3 triangles: degree 9 against the rule's 8, so a rule two orders higher must change R and J (measured
    2.5e-8, 2.6e-7): a test on P3 triangles pins order 8, not "some exact rule".  And on P3 triangles, P2
    tetrahedra and P2 triangles the tabulated rule one order lower (2p + 1) must change them too.  1e-9."""
    m = mesh(name)
    p = m.order
    rule = O.simplex_rule(m.dim, p + 4) if other == "higher" else O.simplex_rule_order(m.dim, 2 * p + 1)
    dR, dJ = _rule_diff(name, rule)
    print(f"{name} {other}: dR {dR:.2e} dJ {dJ:.2e}")
    assert dR > 1e-9 and dJ > 1e-9


@pytest.mark.parametrize("name", SPACES)
def test_boundary_load_integrates(name):
    """sum_i b_i = int g over the selected facets for g = 1 and g linear (exact at order p + 1): 1e-13.  On
    the unit square / cube with the facets on x = 0: int 1 = 1, int (1 + 2 y [+ 3 z]) = 2 [3.5]."""
    m = mesh(name)
    e, f = cdfem.boundary_facets(m, lambda X: bool(np.all(np.abs(X[:, 0]) < 1e-12)))
    one = N.boundary_load(m, e, f, lambda X: np.ones(len(X))).sum()
    lin = N.boundary_load(m, e, f, lambda X: 1.0 + 2.0 * X[:, 1] + (3.0 * X[:, 2] if m.dim == 3 else 0.0)).sum()
    print(f"{name}: {one - 1.0:.2e} {lin - (2.0 if m.dim == 2 else 3.5):.2e}")
    assert abs(one - 1.0) <= 1e-13 and abs(lin - (2.0 if m.dim == 2 else 3.5)) <= 1e-13 * 3.5
    # the whole boundary: perimeter 4 / surface 6
    e, f = cdfem.boundary_facets(m)
    assert abs(N.boundary_load(m, e, f, lambda X: np.ones(len(X))).sum() - (4.0 if m.dim == 2 else 6.0)) <= 6e-13


def test_boundary_facets_by_predicate():
    """Kuhn square n = 6: 24 boundary edges, 6 on each side; Kuhn cube n = 3: 2 * 9 triangles per face"""
    m = mesh("tri2")
    e, f = cdfem.boundary_facets(m)
    assert len(e) == 24 and e.dtype == np.int32 and f.dtype == np.int32 and f.min() >= 0 and f.max() <= 2
    for axis, val in ((0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0)):
        es, fs = cdfem.boundary_facets(m, lambda X: bool(np.all(np.abs(X[:, axis] - val) < 1e-12)))
        assert len(es) == 6
        for a, b in zip(es, fs):  # the facet opposite local vertex b lies on the side
            assert np.all(np.abs(np.delete(m.verts[a], b, axis=0)[:, axis] - val) < 1e-12)
    m3 = mesh("tet1")
    assert len(cdfem.boundary_facets(m3)[0]) == 6 * 18
    assert len(cdfem.boundary_facets(m3, lambda X: bool(np.all(X[:, 0] > 1.0 - 1e-12)))[0]) == 18


NEWTON_CASES = [(mn, sn) for mn in ["tri1", "tri2", "tri3", "tet1", "tet2", "square3"] for sn in "AB"]


@pytest.mark.parametrize("mesh_name,set_name", NEWTON_CASES)
def test_newton_restatement(mesh_name, set_name):
    """Newton converges on both parameter sets; the last two order estimates
    log(r_k+1 / r_k) / log(r_k / r_k-1) show quadratic convergence (>= 1.7); and no iterate leaves the stopping
    decision to rounding: every iterate is either decisively converged (rn < abs_tol / 3 or rn / r0 < rel_tol / 3)
    or decisively not (rn > 3 abs_tol and rn / r0 > 3 rel_tol), with rel_tol per set from nonlinear_ref
    (NEWTON_REL_TOL: A 1e-7, B 1e-8), so two implementations that differ in rounding count alike.  The
    GMRES-driven restatement (1e-13) takes the same iterations and its residual norms above 1e-6 r0 stay
    within the tolerance tests/test_gpu_nonlinear.py allows the HIP path (nonlinear_ref.HISTORY_TOL, 100 times the
    largest spread measured between the two restatement runs)."""
    m, F, _, prm = N.newton_problem(mesh_name, set_name)
    rel_tol, abs_tol = N.NEWTON_REL_TOL[set_name], N.NEWTON_ABS_TOL
    r = F.newton(prm["u_old"].copy(), abs_tol=abs_tol, rel_tol=rel_tol)
    res, r0 = np.array(r["residual"]), r["r0"]
    print(mesh_name, set_name, r["iterations"], res)
    assert r["converged"] and r["iterations"] == (3 if set_name == "A" else 4)
    assert_decisive(r, abs_tol, rel_tol)
    q = [np.log(res[k + 1] / res[k]) / np.log(res[k] / res[k - 1]) for k in range(len(res) - 3, len(res) - 1)]
    print("order estimates", q)
    assert min(q) >= 1.7
    if set_name == "B":
        assert r0 == res[0] > 10.0  # r0 = ||R0|| >> 1 is exercised
    g = F.newton(prm["u_old"].copy(), abs_tol=abs_tol, rel_tol=rel_tol, linear="gmres_jacobi", lin_max_it=50000)
    assert g["iterations"] == r["iterations"] and not g["linear_failed"]
    gr = np.array(g["residual"])
    sel = res > 1e-6 * r0
    spread = (np.abs(gr[sel] - res[sel]) / res[sel]).max()
    print(f"spread {spread:.2e}")
    assert spread <= N.HISTORY_TOL
    assert np.linalg.norm(g["u"] - r["u"]) <= 1e-12 * np.linalg.norm(r["u"])


def assert_decisive(r, abs_tol, rel_tol):
    """no iterate's stopping decision is within a factor 3 of a threshold; only the last one converged"""
    for k, rn in enumerate(r["residual"]):
        yes = rn < abs_tol / 3 or rn / r["r0"] < rel_tol / 3
        no = rn > 3 * abs_tol and rn / r["r0"] > 3 * rel_tol
        assert yes or no, (k, rn, rn / r["r0"])
        assert yes == (k == r["iterations"] and r["converged"])


def test_newton_rebuild_and_max_iter():
    """a Jacobian kept for two iterations converges more slowly but converges, decisively at every iterate;
    max_iter = 1 stops unconverged after one update"""
    m, F, _, prm = N.newton_problem("tri2", "A")
    r1 = F.newton(prm["u_old"].copy(), rel_tol=N.NEWTON_REL_TOL["A"])
    r2 = F.newton(prm["u_old"].copy(), rel_tol=N.NEWTON_REL_TOL["A"], jacobian_rebuild_freq=2)
    print(r2["iterations"], r2["residual"])
    assert r2["converged"] and r2["iterations"] >= r1["iterations"]
    assert_decisive(r2, N.NEWTON_ABS_TOL, N.NEWTON_REL_TOL["A"])
    assert np.linalg.norm(r2["u"] - r1["u"]) <= 1e-6 * np.linalg.norm(r1["u"])
    r3 = F.newton(prm["u_old"].copy(), rel_tol=N.NEWTON_REL_TOL["A"], max_iter=1)
    assert not r3["converged"] and r3["iterations"] == 1 and len(r3["residual"]) == 1 and len(r3["update"]) == 1


def test_three_steps_restatement():
    """three backward-Euler steps of set A on P2 triangles, each from the last solution: rel_tol
    nonlinear_ref.THREE_STEP_REL_TOL = 1e-9 keeps every iterate of every step decisive (at 1e-7, step 2's second
    iterate sits at 2.8e-7; at 1e-8, step 0's third at 9.2e-9)"""
    m, F, _, prm = N.newton_problem("tri2", "A")
    u = prm["u_old"].copy()
    its = []
    for step in range(3):
        F.u_old = u.copy()
        r = F.newton(u, abs_tol=N.NEWTON_ABS_TOL, rel_tol=N.THREE_STEP_REL_TOL)
        print(step, r["iterations"], r["residual"])
        assert r["converged"]
        assert_decisive(r, N.NEWTON_ABS_TOL, N.THREE_STEP_REL_TOL)
        u = r["u"]
        its.append(r["iterations"])
    assert its == [4, 3, 3]


NEW_SYMBOLS = ["cdfem_nl_setup", "cdfem_nl_set_old", "cdfem_nl_set_rhs", "cdfem_nl_residual", "cdfem_nl_gradient",
               "cdfem_newton_solve", "cdfem_newton_history", "cdfem_bdr_set", "cdfem_bdr_rule_size",
               "cdfem_bdr_quadrature_points", "cdfem_bdr_lf_assemble"]


def test_binding_surface():
    """the header declares the new entry points, the library exports them, the binding declares their
    signatures, and Context has the methods"""
    declared = cdfem.exported_symbols_from_header()
    L = cdfem.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        f = getattr(L, s)
        assert f.argtypes is not None and f.restype is not None, s  # set by _declare
    for meth in ("nl_setup", "nl_set_old", "nl_set_rhs", "nl_residual", "nl_gradient", "newton_solve", "bdr_set",
                 "bdr_quadrature_points", "bdr_lf_assemble"):
        assert callable(getattr(cdfem.Context, meth)), meth
    assert cdfem.RULE_NONLINEAR == 6 and callable(cdfem.boundary_facets)
    assert L.cdfem_abi_version() == 1
