"""Every term mask (kinds 1..7) through every launcher that turns it into a template argument, and the
GMRES passes at every entries-per-thread count.

The launchers (csrc/dispatch.hpp) pick a kernel instantiation from run-time state. The other GPU tests
reach every option and every order, but mostly at kinds 7, 5 and 3; a mask that reached the wrong
instantiation would compute another operator, which the oracle sees at once. Shapes are the smallest
that separate the launch branches: p <= 2 bricks on 4 x 4 x 4 elements (every brick full) and 5 x 4 x 6
(partial bricks), p = 3, 4 blocks on 2 x 2 x 2 and 3 x 2 x 5 with ho_block_z 2 and 4, the generic apply
on a perturbed 3 x 4 x 2 box. Tolerances are the ones of tests/test_gpu_parity.py and
tests/test_gpu_high_order.py for the same quantities: Mult to 1e-13 of the oracle's, fixed Jacobi-CG
iterates to 1e-11 (fewer iterates here than there).

Convection alone (kinds 2) is skew-symmetric: d . A d = 0 and its diagonal is zero, so Jacobi-CG has no
iterate to compare; its CG instantiations run in test_gpu_brick_cg.py::test_beta_fold_breakdown_paths,
and here its Mult is checked.
"""
import functools

import numpy as np
import pytest

import cdfem
from oracle import oracle as O

pytestmark = pytest.mark.gpu
C3 = (1.0, -2.0, 0.5)
ITERS = 8  # below the 10 distinct eigenvalues of the smallest case (4 x 4 x 4 at p = 1: 3^3 interior dofs)
ALL_KINDS = [1, 2, 3, 4, 5, 6, 7]


def _kinds_o(k):
    return (O.DIFFUSION if k & 1 else 0) | (O.CONVECTION if k & 2 else 0) | (O.MASS if k & 4 else 0)


@functools.lru_cache(maxsize=None)
def _reference(dim, shape, p, pert, kinds):
    """The oracle's operator, a system with non-zero essential values and ITERS Jacobi-CG iterates."""
    om = O.BoxMesh(dim, shape, p, perturb=pert)
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3[:dim], kinds=_kinds_o(kinds))
    rng = np.random.default_rng(97)
    x = rng.uniform(-1, 1, om.nl)
    u = np.zeros(om.nl)
    u[om.ess] = rng.uniform(-1, 1, len(om.ess))
    b = rng.uniform(-1, 1, om.nl)
    xo = None
    if kinds != 2:
        Ac, Bo = O.form_linear_system(A, om.bdr, u, b)
        xo, _ = O.cg(Ac, Bo, dinv=1.0 / Ac.diag(), rel_tol=0.0, abs_tol=0.0, max_iter=ITERS)
    y = A.mult(x)
    xz = x.copy()
    xz[om.ess] = 0.0
    yc = A.mult(xz)
    yc[om.ess] = x[om.ess]
    for a in (x, u, b, y, yc) + (() if xo is None else (xo,)):
        a.setflags(write=False)
    return om, x, y, yc, u, b, xo


def _check_mult(gpu_ctx, x, y, yc):
    assert np.abs(gpu_ctx.mult(x) - y).max() <= 1e-13 * np.abs(y).max()
    assert np.abs(gpu_ctx.mult(x, constrained=True) - yc).max() <= 1e-13 * np.abs(yc).max()


def _check_cg(gpu_ctx, u, b, xo):
    _, B = gpu_ctx.form_linear_system(u, b)
    xg, info = gpu_ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=ITERS, check_every=5)
    assert info["iterations"] == ITERS
    assert np.linalg.norm(xg - xo) <= 1e-11 * np.linalg.norm(xo)


@pytest.mark.parametrize("kinds", ALL_KINDS)
@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 4, 6)])
@pytest.mark.parametrize("p", [1, 2])
def test_brick_every_kinds(gpu_ctx, p, shape, kinds):
    """p <= 2 on a structured box: the brick Mult (k_brick3d) and the brick CG (k_brick_cg and the update;
    at p = 2, kinds 7 and 5 the uniform box's element-matrix kernel) for every mask."""
    om, x, y, yc, u, b, xo = _reference(3, shape, p, 0.0, kinds)
    gpu_ctx.upload_mesh(cdfem.Mesh(3, p, om.verts, om.dofmap, om.nl, om.ess)).set_structured(*shape)
    gpu_ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    assert gpu_ctx.kernel_name(cdfem.K_APPLY) == "k_brick_cg"
    _check_mult(gpu_ctx, x, y, yc)
    if xo is not None:
        _check_cg(gpu_ctx, u, b, xo)
        if p == 2 and kinds in (5, 7):  # the Kronecker form's instantiation of the same mask
            try:
                gpu_ctx.set_option("pa_uniform", 0)
                _check_cg(gpu_ctx, u, b, xo)
            finally:
                gpu_ctx.set_option("pa_uniform", 1)


@pytest.mark.parametrize("kinds", ALL_KINDS)
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 5)])
@pytest.mark.parametrize("p", [3, 4])
def test_ho_every_kinds(gpu_ctx, p, shape, kinds):
    """p = 3, 4 on a structured box: the tile apply's Mult and the block CG on 2 x 2 x 2 and 2 x 2 x 4
    blocks (k_hobrick_cg; on 2 x 2 x 4 blocks at kinds 7 and 5 the element-matrix kernel) for every mask."""
    om, x, y, yc, u, b, xo = _reference(3, shape, p, 0.0, kinds)
    gm = cdfem.Mesh(3, p, om.verts, om.dofmap, om.nl, om.ess)
    try:
        for bz in (2, 4):
            gpu_ctx.set_option("ho_block_z", bz)
            gpu_ctx.upload_mesh(gm).set_structured(*shape)
            gpu_ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
            assert gpu_ctx.kernel_name(cdfem.K_APPLY) in ("k_hobrick_cg", "k_hobrick_um")
            if bz == 2:
                _check_mult(gpu_ctx, x, y, yc)
            if xo is not None:
                _check_cg(gpu_ctx, u, b, xo)
    finally:
        gpu_ctx.set_option("ho_block_z", 2)


@pytest.mark.parametrize("kinds", ALL_KINDS)
@pytest.mark.parametrize("dim,shape,p", [(3, (3, 4, 2), 1), (3, (3, 4, 2), 2), (2, (3, 4), 3)])
def test_generic_apply_every_kinds(gpu_ctx, dim, shape, p, kinds):
    """The generic apply (k_apply3d / k_apply2d, per-point data) on a perturbed box for every mask, plain
    and constrained (the box has too few interior dofs for CG iterates to mean anything)."""
    om, x, y, yc, u, b, xo = _reference(dim, shape, p, 0.2, kinds)
    gpu_ctx.upload_mesh(cdfem.Mesh(dim, p, om.verts, om.dofmap, om.nl, om.ess))
    gpu_ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3[:dim], mass=1.0)
    _check_mult(gpu_ctx, x, y, yc)


@pytest.mark.parametrize("structured", [False, True])
def test_gmres_entries_per_thread(gpu_ctx, structured):
    """gm_ept 4, 5, 6, 8: the two orthogonalisation passes with that many entries per thread (the partial
    sums split differently, so not bitwise) against the oracle's GMRES, tolerances of
    test_gpu_gmres.py::test_gmres_fixed_steps_parity; 13^3 and 17^3 dofs: several blocks at every count,
    the last one partial. The structured box reads w from the brick patch in the first pass."""
    n, p = (8, 2) if structured else (6, 2)
    om = O.BoxMesh(3, n, p, perturb=0.1)
    gpu_ctx.upload_mesh(cdfem.Mesh(3, p, om.verts, om.dofmap, om.nl, om.ess))
    if structured:
        gpu_ctx.set_structured(n, n, n)
    gpu_ctx.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3, kinds=_kinds_o(7))
    rng = np.random.default_rng(5)
    u = np.zeros(om.nl)
    u[om.ess] = rng.uniform(-1, 1, len(om.ess))
    b = rng.uniform(-1, 1, om.nl)
    Ac, Bo = O.form_linear_system(A, om.bdr, u, b)
    _, B = gpu_ctx.form_linear_system(u, b)
    xo, io = O.gmres(Ac, Bo, dinv=1.0 / Ac.diag(), restart=7, rtol=0.0, atol=0.0, max_it=17)
    try:
        for ept in (4, 5, 6, 8):
            gpu_ctx.set_option("gm_ept", ept)
            xg, ig = gpu_ctx.solve(B, method="gmres", pc="jacobi", restart=7, rel_tol=0.0, abs_tol=0.0, max_iter=17)
            assert ig["iterations"] == io["iterations"] == 17, ept
            assert np.linalg.norm(xg - xo) <= 1e-11 * np.linalg.norm(xo), ept
            assert abs(ig["final_norm"] - io["final_norm"]) <= 1e-9 * io["final_norm"], ept
    finally:
        gpu_ctx.set_option("gm_ept", 0)
