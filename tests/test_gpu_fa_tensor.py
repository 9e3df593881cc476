"""GPU full assembly on quad and hex meshes (cdfem_fa_setup on tensor elements) against the oracle.

The element matrices come from k_tensor_elem (quads p = 1..4, hexes p = 1, 2, the OPERATOR rule); the gather,
the elimination, the SELL SpMV and ILU(0) are the simplex pipeline's.  Tolerances are tests/test_gpu_fa.py's:
1e-13 of the largest entry for CSR values, Mult, constrained Mult, diagonal and FormLinearSystem; 1e-11 for
fixed-step iterates; converged solves 1e-8 with iteration counts within +-1; FA against PA 1e-12 of max |y|.
The meshes put the element count below, just above and across the 64-element block of the Ee layout.
"""
import functools

import numpy as np
import pytest

import cdfem
from oracle import oracle as O

pytestmark = pytest.mark.gpu
C3 = (1.0, -2.0, 0.5)

# dim, n, p, perturb            ne   max nnz/row
MESHES = [(2, (9, 8), 1, 0.2),     # 72    9
          (2, (10, 7), 2, 0.15),   # 70   25
          (2, (4, 3), 3, 0.2),     # 12   49
          (2, (3, 2), 4, 0.2),     #  6   81
          (3, (5, 4, 4), 1, 0.2),  # 80   27
          (3, (5, 7, 2), 2, 0.15)]  # 70  125


def _kinds_o(k):
    return (O.DIFFUSION if k & 1 else 0) | (O.CONVECTION if k & 2 else 0) | (O.MASS if k & 4 else 0)


@functools.lru_cache(maxsize=None)
def _mesh(dim, n, p, pert):
    gm = cdfem.box_mesh(dim, n, p, perturb=pert)
    om = O.BoxMesh(dim, n, p)              # container for the same arrays
    om.verts, om.dofmap = gm.verts, gm.dofmap
    np.testing.assert_array_equal(om.ess, gm.ess)
    return gm, om


@functools.lru_cache(maxsize=None)
def _oracle(dim, n, p, pert, kinds=7):
    """The oracle's CSR and its FormLinearSystem matrix for a mesh and a kinds mask, computed once."""
    _, om = _mesh(dim, n, p, pert)
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3[:dim], kinds=_kinds_o(kinds))
    Ac, _ = O.form_linear_system(A, om.bdr, np.zeros(om.nl), np.zeros(om.nl))
    return A, Ac


def _fa(ctx, gm, kinds=7):
    ctx.fa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3[:gm.dim], mass=1.0)
    return ctx


def _system(om, A, seed=11):
    """Random essential values and right-hand side, as test_fa_gmres_ilu_parity draws them."""
    rng = np.random.default_rng(seed)
    u = np.zeros(om.nl)
    u[om.ess] = rng.uniform(-1, 1, len(om.ess))
    b = rng.uniform(-1, 1, om.nl)
    Ac, Bo = O.form_linear_system(A, om.bdr, u, b)
    return u, b, Ac, Bo


@pytest.mark.parametrize("dim,n,p,pert", MESHES)
@pytest.mark.parametrize("kinds", [7, 5, 2])
def test_fa_tensor_csr_parity(dim, n, p, pert, kinds):
    gm, om = _mesh(dim, n, p, pert)
    A, Ac = _oracle(dim, n, p, pert, kinds)
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        _fa(ctx, gm, kinds)
        rp, cols, vals = ctx.fa_csr()
        orp, ocol, oval = A.export()
        np.testing.assert_array_equal(rp, orp)
        np.testing.assert_array_equal(cols, ocol)
        err = np.abs(vals - oval).max() / np.abs(oval).max()
        print(f"csr values {err:.3e}")
        assert err <= 1e-13
        _, _, cvals = ctx.fa_csr(constrained=True)
        _, _, ocv = Ac.export()
        assert np.abs(cvals - ocv).max() <= 1e-13 * np.abs(ocv).max()
        _fa(ctx, gm, kinds)                 # assembling twice: identical bits
        np.testing.assert_array_equal(ctx.fa_csr()[2], vals)
        np.testing.assert_array_equal(ctx.fa_csr(constrained=True)[2], cvals)


@pytest.mark.parametrize("dim,n,p,pert", MESHES)
def test_fa_tensor_operator_parity(dim, n, p, pert):
    gm, om = _mesh(dim, n, p, pert)
    A, _ = _oracle(dim, n, p, pert)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, om.nl)
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        _fa(ctx, gm)
        yo = A.mult(x)
        y = ctx.mult(x)
        assert np.abs(y - yo).max() <= 1e-13 * np.abs(yo).max()
        xz = x.copy()
        xz[om.ess] = 0.0
        yc = A.mult(xz)
        yc[om.ess] = x[om.ess]
        assert np.abs(ctx.mult(x, constrained=True) - yc).max() <= 1e-13 * np.abs(yc).max()
        d = ctx.diagonal()
        assert np.abs(d - A.diag()).max() <= 1e-13 * np.abs(A.diag()).max()
        u = np.zeros(om.nl)
        u[om.ess] = rng.uniform(-1, 1, len(om.ess))
        b = rng.uniform(-1, 1, om.nl)
        _, Bo = O.form_linear_system(A, om.bdr, u, b)
        _, B = ctx.form_linear_system(u, b)
        assert np.abs(B - Bo).max() <= 1e-13 * np.abs(Bo).max()
    # the partial-assembly operator of a second context on the same mesh
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        ctx.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3[:dim], mass=1.0)
        ypa = ctx.mult(x)
    assert np.abs(y - ypa).max() <= 1e-12 * np.abs(ypa).max()


@pytest.mark.parametrize("dim,n,p,pert", [(3, (3, 2, 3), 2, 0.2), (2, (4, 3), 3, 0.2)])
def test_fa_tensor_point_coefficients(dim, n, p, pert):
    """kappa_q, kmat_q (K = kappa_q I + K_q), conv_q and mass_q sampled at the OPERATOR rule's points."""
    gm, om = _mesh(dim, n, p, pert)
    ns = dim * (dim + 1) // 2
    rng = np.random.default_rng(21)
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        nq = ctx.rule_size(cdfem.RULE_OPERATOR)
        assert nq == ((p + 2) ** 3 if dim == 3 else (p + 1) ** 2)
        assert ctx.quadrature_points(cdfem.RULE_OPERATOR).shape == (gm.ne, nq, dim)
        kq = rng.uniform(0.05, 0.2, (gm.ne, nq))
        cq = rng.uniform(-1, 1, (gm.ne, nq, dim))
        mq = rng.uniform(0.5, 1.5, (gm.ne, nq))
        kmq = rng.uniform(-0.02, 0.02, (gm.ne, nq, ns))   # small and symmetric by storage: K stays positive
        for kw_g, kw_o in ((dict(kappa_q=kq, conv_q=cq, mass_q=mq), dict(kappa_q=kq, c_q=cq, s_q=mq)),
                           (dict(kappa_q=kq, kmat_q=kmq, conv_q=cq, mass_q=mq),
                            dict(kappa_q=kq, kmat_q=kmq, c_q=cq, s_q=mq))):
            ctx.fa_setup(kinds=7, kappa=0.0, alpha=1.0, mass=0.0, **kw_g)
            A = O.fa_assemble_q(om, kappa=0.0, alpha=1.0, s=0.0, **kw_o)
            _, _, oval = A.export()
            vals = ctx.fa_csr()[2]
            assert np.abs(vals - oval).max() <= 1e-13 * np.abs(oval).max()
        # arrays that hold the constants give the constants' matrix
        ctx.fa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3[:dim], mass=1.0)
        v0 = ctx.fa_csr()[2]
        ctx.fa_setup(kinds=7, kappa=0.0, kappa_q=np.full((gm.ne, nq), 0.1), alpha=1.0,
                     conv_q=np.tile(np.array(C3[:dim]), gm.ne * nq), mass=0.0, mass_q=np.ones((gm.ne, nq)))
        assert np.abs(ctx.fa_csr()[2] - v0).max() <= 1e-14 * np.abs(v0).max()


@pytest.mark.parametrize("dim,n,p,pert", MESHES)
def test_fa_tensor_gmres_ilu_parity(dim, n, p, pert):
    gm, om = _mesh(dim, n, p, pert)
    A, _ = _oracle(dim, n, p, pert)
    u, b, Ac, Bo = _system(om, A)
    F = O.ilu0(Ac)
    tol = dict(rel_tol=1e-10, abs_tol=1e-12, max_iter=2000)
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        _fa(ctx, gm)
        _, B = ctx.form_linear_system(u, b)
        xo, io = O.gmres_ilu(Ac, Bo, F, restart=3, rtol=0.0, atol=0.0, max_it=5)
        xg, ig = ctx.solve(B, method="gmres", pc="ilu", restart=3, rel_tol=0.0, abs_tol=0.0, max_iter=5)
        assert io["iterations"] == ig["iterations"] == 5
        err = np.linalg.norm(xg - xo) / np.linalg.norm(xo)
        print(f"5 fixed steps {err:.3e}")
        assert err <= 1e-11
        xo, io = O.gmres_ilu(Ac, Bo, F, restart=30, rtol=1e-10, atol=1e-12, max_it=2000)
        xg, ig = ctx.solve(B, method="gmres", pc="ilu", restart=30, **tol)
        print(f"iterations ilu {ig['iterations']} (oracle {io['iterations']})")
        assert io["converged"] and ig["converged"] and abs(io["iterations"] - ig["iterations"]) <= 1
        assert np.linalg.norm(xg - xo) <= 1e-8 * np.linalg.norm(xo)
        _, ij = ctx.solve(B, method="gmres", pc="jacobi", restart=30, **tol)
        print(f"iterations jacobi {ij['iterations']}")
        assert ij["converged"] and ig["iterations"] < ij["iterations"]
        xg2, _ = ctx.solve(B, method="gmres", pc="ilu", restart=30, **tol)
        np.testing.assert_array_equal(xg, xg2)
        xb, ib = ctx.solve(B, method="bicgstab", pc="ilu", **tol)
        assert ib["converged"]
        assert np.linalg.norm(xb - xo) <= 1e-8 * np.linalg.norm(xo)


@pytest.mark.parametrize("dim,n,p,pert", [MESHES[1], MESHES[5]])
def test_fa_tensor_cg_and_jacobi_gmres_parity(dim, n, p, pert):
    gm, om = _mesh(dim, n, p, pert)
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        A, _ = _oracle(dim, n, p, pert, 5)          # kappa K + s M: SPD
        _fa(ctx, gm, 5)
        b = np.random.default_rng(4).uniform(-1, 1, om.nl)
        Ac, Bo = O.form_linear_system(A, om.bdr, np.zeros(om.nl), b)
        _, B = ctx.form_linear_system(np.zeros(om.nl), b)
        xo, io = O.cg(Ac, Bo, dinv=1.0 / Ac.diag(), rel_tol=0.0, abs_tol=0.0, max_iter=30)
        xg, ig = ctx.solve(B, method="cg", rel_tol=0.0, abs_tol=0.0, max_iter=30, check_every=9)
        assert io["iterations"] == ig["iterations"] == 30
        assert np.linalg.norm(xg - xo) <= 1e-11 * np.linalg.norm(xo)
        A, _ = _oracle(dim, n, p, pert, 7)
        _fa(ctx, gm, 7)
        u, b, Ac, Bo = _system(om, A, seed=8)
        _, B = ctx.form_linear_system(u, b)
        xo, io = O.gmres(Ac, Bo, dinv=1.0 / Ac.diag(), restart=7, rtol=0.0, atol=0.0, max_it=30)
        xg, ig = ctx.solve(B, method="gmres", restart=7, rel_tol=0.0, abs_tol=0.0, max_iter=30)
        assert io["iterations"] == ig["iterations"] == 30
        assert np.linalg.norm(xg - xo) <= 1e-11 * np.linalg.norm(xo)


@pytest.mark.parametrize("order", [1, 2, 3, 8])
def test_fa_tensor_spmv_orders(order):
    dim, n, p, pert = MESHES[5]
    gm, om = _mesh(dim, n, p, pert)
    A, _ = _oracle(dim, n, p, pert)
    x = np.random.default_rng(5).uniform(-1, 1, om.nl)
    yo = A.mult(x)
    with cdfem.Context(0) as ctx:
        try:
            ctx.set_option("sell_order", order)
            ctx.upload_mesh(gm)
            _fa(ctx, gm)
            assert np.abs(ctx.mult(x) - yo).max() <= 1e-13 * np.abs(yo).max()
        finally:
            ctx.set_option("sell_order", 8)


@pytest.mark.parametrize("n,p", [((4, 3, 3), 2), ((5, 4, 4), 1)])
@pytest.mark.parametrize("pert", [0.0, 0.2])
def test_fa_tensor_structured_context(n, p, pert):
    """A context declared structured runs the SpMV after fa_setup, not the brick kernels: the bits of a context
    that was not declared structured."""
    gm, om = _mesh(3, n, p, pert)
    rng = np.random.default_rng(6)
    x, b = rng.uniform(-1, 1, om.nl), rng.uniform(-1, 1, om.nl)

    def run(structured):
        with cdfem.Context(0).upload_mesh(gm) as ctx:
            if structured:
                ctx.set_structured(*n)
            _fa(ctx, gm, 7)
            out = [ctx.fa_csr()[2], ctx.mult(x), ctx.mult(x, constrained=True), ctx.kernel_name(cdfem.K_APPLY)]
            _, B = ctx.form_linear_system(np.zeros(om.nl), b)
            out.append(ctx.solve(B, method="gmres", restart=10, rel_tol=0.0, abs_tol=0.0, max_iter=15)[0])
            _fa(ctx, gm, 5)
            _, B = ctx.form_linear_system(np.zeros(om.nl), b)
            out.append(ctx.solve(B, method="cg", rel_tol=0.0, abs_tol=0.0, max_iter=15)[0])
            return out

    plain, st = run(False), run(True)
    for a, c in zip(plain, st):
        if isinstance(a, str):
            assert a == c
        else:
            np.testing.assert_array_equal(a, c)
    km = cdfem.kuhn_mesh(3, 3, 2, perturb=0.1)
    with cdfem.Context(0).upload_mesh(km) as ctx:
        ctx.fa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
        assert st[3] == ctx.kernel_name(cdfem.K_APPLY)


def test_fa_tensor_operator_switching():
    dim, n, p, pert = MESHES[1]
    gm, om = _mesh(dim, n, p, pert)
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, om.nl)
    co = dict(dt=0.1, a0=1.0, a1=0.5, m0=1.0, m1=0.5)
    pa = dict(kinds=7, kappa=0.1, alpha=1.0, conv=C3[:dim], mass=1.0)
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        yfa = (_fa(ctx, gm).mult(x), ctx.mult(x, constrained=True))
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        ctx.pa_setup(**pa)
        ypa = (ctx.mult(x), ctx.mult(x, constrained=True))
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        ctx.nl_pa_setup(**co)
        ctx.nl_set_old(0.5 * x)
        rnl = ctx.nl_residual(x)
    with cdfem.Context(0).upload_mesh(gm) as ctx:
        B = np.ones(om.nl)
        _fa(ctx, gm)
        for k in (0, 1):
            np.testing.assert_array_equal(ctx.mult(x, constrained=bool(k)), yfa[k])
        xi, info = ctx.solve(B, method="gmres", pc="ilu", restart=30, rel_tol=1e-10, abs_tol=1e-12, max_iter=200)
        assert info["converged"]
        ctx.pa_setup(**pa)
        for k in (0, 1):
            np.testing.assert_array_equal(ctx.mult(x, constrained=bool(k)), ypa[k])
        with pytest.raises(cdfem.CdfemError) as e:     # ILU is refused again on the PA operator
            ctx.solve(B, method="gmres", pc="ilu")
        assert e.value.code == cdfem.ERR_UNSUPPORTED
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.fa_csr()
        assert e.value.code == cdfem.ERR_STATE
        _fa(ctx, gm)                                   # the pattern is reused
        for k in (0, 1):
            np.testing.assert_array_equal(ctx.mult(x, constrained=bool(k)), yfa[k])
        xi2, _ = ctx.solve(B, method="gmres", pc="ilu", restart=30, rel_tol=1e-10, abs_tol=1e-12, max_iter=200)
        np.testing.assert_array_equal(xi, xi2)
        ctx.nl_pa_setup(**co)
        ctx.nl_set_old(0.5 * x)
        np.testing.assert_array_equal(ctx.nl_residual(x), rnl)
        with pytest.raises(cdfem.CdfemError) as e:     # the assembled operator went with nl_pa_setup
            ctx.fa_csr()
        assert e.value.code == cdfem.ERR_STATE


def test_fa_tensor_status_codes():
    for mesh in (cdfem.box_mesh(3, 2, 3), cdfem.box_mesh(3, 1, 4)):
        with cdfem.Context(0).upload_mesh(mesh) as ctx:
            with pytest.raises(cdfem.CdfemError, match="hexes p = 1, 2") as e:
                ctx.fa_setup(kinds=5, kappa=0.1, mass=1.0)
            assert e.value.code == cdfem.ERR_UNSUPPORTED
    quad = cdfem.box_mesh(2, (3, 2), 2)
    with cdfem.Context(0).upload_mesh(quad) as ctx:
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.fa_csr()
        assert e.value.code == cdfem.ERR_STATE
        # a context with a two-rank host communicator is refused
        ctx.comm_init_host(0, 2, lambda a: None, lambda *a: None)
        with pytest.raises(cdfem.CdfemError) as e:
            ctx.fa_setup(kinds=5, kappa=0.1, mass=1.0)
        assert e.value.code == cdfem.ERR_UNSUPPORTED
