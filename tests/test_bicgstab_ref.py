"""The CPU restatement of BiCGStab (tests/bicgstab_ref.py) pinned independently, and the Python
binding's method names.  No GPU.

With Jacobi, left-preconditioned KSPBCGS is unpreconditioned BiCGStab on (D^-1 A_c, D^-1 B), which
scipy implements: 8 iterates agree to 1e-12 (measured <= 7.1e-15 with scipy 1.15.3).  Converged at
the reference's tolerances the solution is GMRES's to 1e-8 (measured <= 7.9e-10).
"""
import numpy as np
import pytest

import bicgstab_ref as R
from oracle import oracle as O

C3 = (1.0, -2.0, 0.5)
# (dim, shape, p, perturb): the GPU tests' small systems
SYSTEMS = [(3, (9, 6, 7), 2, 0.0), (3, (5, 6, 9), 2, 0.1), (3, (3, 2, 3), 4, 0.1), (2, (7, 5), 3, 0.15)]


def _system(dim, shape, p, pert, seed=17):
    om = O.BoxMesh(dim, shape, p, perturb=pert)
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3[:dim])
    rng = np.random.default_rng(seed)
    u = np.zeros(om.nl)
    u[om.ess] = rng.uniform(-1, 1, len(om.ess))
    b = rng.uniform(-1, 1, om.nl)
    return O.form_linear_system(A, om.bdr, u, b)


@pytest.fixture(scope="module", params=SYSTEMS, ids=lambda s: "x".join(map(str, s[1])) + f"-p{s[2]}")
def system(request):
    return _system(*request.param)


def test_restatement_matches_scipy_bicgstab(system):
    spla = pytest.importorskip("scipy.sparse.linalg")
    sp = pytest.importorskip("scipy.sparse")
    Ac, Bo = system
    dinv = 1.0 / Ac.diag()
    x, info = R.bcgs(Ac.mult, lambda y: dinv * y, Bo, 0.0, 0.0, 8)
    assert info["iterations"] == 8 and not info["converged"]
    DA = sp.diags(dinv) @ Ac.to_scipy()
    xs, _ = spla.bicgstab(DA, dinv * Bo, x0=np.zeros_like(Bo), rtol=0.0, atol=0.0, maxiter=8)
    rel = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"restatement against scipy bicgstab, 8 iterations: {rel:.2e}")
    assert rel <= 1e-12


def test_restatement_converged_matches_gmres(system):
    Ac, Bo = system
    dinv = 1.0 / Ac.diag()
    xg, ig = O.gmres(Ac, Bo, dinv=dinv, restart=30, rtol=1e-10, atol=1e-12, max_it=500)
    x, info = R.bcgs(Ac.mult, lambda y: dinv * y, Bo, 1e-10, 1e-12, 500)
    assert ig["converged"] and info["converged"]
    rel = np.linalg.norm(x - xg) / np.linalg.norm(xg)
    print(f"BiCGStab {info['iterations']} iterations, GMRES {ig['iterations']} steps, solutions {rel:.2e} apart")
    assert rel <= 1e-8


def test_restatement_second_pattern_agrees(system):
    """The two rounding patterns (Ac.mult + np.dot, scipy product + reversed-block dot) stay within 1e-13
    over 8 iterations: the bound the GPU tests' guard asserts."""
    Ac, Bo = system
    dinv = 1.0 / Ac.diag()
    (_, _, h1), (_, _, h2) = R.restatements(Ac, Bo, lambda y: dinv * y)
    assert len(h1) == len(h2) == 8
    assert R.drift(h1, h2) <= 1e-13


def test_restatement_edge_cases():
    Ac, Bo = _system(2, (4, 4), 1, 0.0)
    x, info = R.bcgs(Ac.mult, None, np.zeros_like(Bo), 1e-10, 0.0, 10)
    assert info["converged"] and info["iterations"] == 0 and not x.any()
    x, info = R.bcgs(Ac.mult, None, Bo, 1e-10, 0.0, 0)
    assert not info["converged"] and info["iterations"] == 0 and not x.any()
    # one p = 1 hex, every dof essential: A_c = I, so s = 0 and t = 0 (the d2 == 0 exit), x = u exactly
    om = O.BoxMesh(3, 1, 1)
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3)
    u = np.arange(1.0, om.nl + 1.0)
    Ac, Bo = O.form_linear_system(A, om.bdr, u, np.zeros(om.nl))
    x, info = R.bcgs(Ac.mult, None, Bo, 1e-12, 0.0, 10)
    assert info["converged"] and info["iterations"] == 1 and info["final_norm"] == 0.0
    np.testing.assert_array_equal(x, u)


def test_method_names():
    import cdfem
    assert [cdfem.METHODS[k] for k in ("cg", "gmres", "bicgstab", "bcgs")] == [0, 1, 2, 2]
    assert [cdfem.method_id(k) for k in ("cg", "gmres", "bicgstab", "bcgs")] == [0, 1, 2, 2]
    assert (cdfem.CG, cdfem.GMRES, cdfem.BICGSTAB) == (0, 1, 2)
    for bad in ("bicg", "GMRES", "", None):
        with pytest.raises(ValueError):
            cdfem.method_id(bad)
