"""ho_uniform: the p = 3, 4 block CG apply on a uniformly refined box as one dense GEMM on the matrix cores.

With set_option("ho_uniform", 1) cdfem_pa_setup checks that every element's affine factors equal element
0's (each component within 1e-14 of its own magnitude) and forms the one N x N element matrix (N = 64 at
p = 3, 125 at p = 4; column j = the Kronecker core on e_j).  The CG apply on 2 x 2 x 4 blocks
(ho_block_z 4) is then k_hobrick_um: a persistent kernel whose waves hold one 16-row tile of the matrix
each and form Y (N x 16) = A X for the block's 16 elements on v_mfma_f64_16x16x4_f64; the patch gather,
the in-block E->L sum and the update kernel are the Kronecker form's.  The operator is the Kronecker
form's to rounding, so the iterates are checked against the oracle (Jacobi-CG on the assembled
constrained matrix, mesh_recession_handler.cpp:270-276 semantics, 1e-11), against ho_uniform 0 on the
same blocks, for bitwise repeatability and for independence of the grid (ho_uniform_grid); every case
the option does not cover must keep the Kronecker form."""
import numpy as np
import pytest

import cdfem
from oracle import oracle as O

pytestmark = pytest.mark.gpu
C3 = (1.0, -2.0, 0.5)
UM, KRON = "k_hobrick_um", "k_hobrick_cg"
# ho_uniform 1 against ho_uniform 0 on the same blocks: the sibling tests' bound (test_ho_block_z4_parity,
# test_uniform_matrix_parity).  Measured on the MI355X over every case below: at most 4.0e-15.
TOL_KRON = 1e-12


def _kinds_o(kinds):
    return (O.DIFFUSION if kinds & 1 else 0) | (O.CONVECTION if kinds & 2 else 0) | (O.MASS if kinds & 4 else 0)


def _problem(om, kinds, seed, bdr=None):
    """The oracle's constrained system with non-zero essential values (bdr: the essential marker)."""
    bdr = om.bdr if bdr is None else bdr
    ess = np.nonzero(bdr)[0].astype(np.int32)
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3, kinds=_kinds_o(kinds))
    rng = np.random.default_rng(seed)
    u = np.zeros(om.nl)
    u[ess] = rng.uniform(-1, 1, len(ess))
    b = rng.uniform(-1, 1, om.nl)
    Ac, Bo = O.form_linear_system(A, bdr, u, b)
    return Ac, Bo, u, b, ess


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _restore(ctx):
    ctx.set_option("ho_uniform", 0)
    ctx.set_option("ho_uniform_grid", 0)
    ctx.set_option("ho_block_z", 2)


def _setup(ctx, om, shape, p, kinds, ess, bz=4, uni=1):
    ctx.set_option("ho_block_z", bz)
    ctx.set_option("ho_uniform", uni)
    ctx.upload_mesh(cdfem.Mesh(3, p, om.verts, om.dofmap, om.nl, ess)).set_structured(*shape)
    ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)


def _fixed(ctx, B, n, **kw):
    return ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=n, **kw)


def _both_forms(ctx, om, shape, p, kinds, seed, bdr=None, iters=40):
    """iters fixed Jacobi-CG iterates with ho_uniform 1 and 0 on 2 x 2 x 4 blocks, against the oracle's."""
    Ac, Bo, u, b, ess = _problem(om, kinds, seed, bdr)
    xo, _ = O.cg(Ac, Bo, dinv=1.0 / Ac.diag(), rel_tol=0.0, abs_tol=0.0, max_iter=iters)
    out, name, nbytes = {}, {}, {}
    try:
        _setup(ctx, om, shape, p, kinds, ess)
        _, B = ctx.form_linear_system(u, b)
        for uni in (1, 0):  # (0 after the setup switches back without a new setup)
            ctx.set_option("ho_uniform", uni)
            name[uni] = ctx.kernel_name(cdfem.K_APPLY)
            nbytes[uni] = ctx.kernel_bytes(cdfem.K_APPLY)
            out[uni] = _fixed(ctx, B, iters, check_every=7)
        ctx.set_option("ho_uniform", 1)
        again = _fixed(ctx, B, iters)
        flops = ctx.kernel_flops(cdfem.K_APPLY)
    finally:
        _restore(ctx)
    assert name == {1: UM, 0: KRON}
    nd, ne = (p + 1) ** 3, shape[0] * shape[1] * shape[2]
    assert flops == 2.0 * nd * nd * ne
    ncomp = {7: 10, 5: 7}[kinds]
    assert nbytes[0] - nbytes[1] == 8.0 * ncomp * ne - 8.0 * (16 * ((nd + 15) // 16)) * (4 * ((nd + 3) // 4))
    np.testing.assert_array_equal(again[0], out[1][0])
    e_or = {uni: _rel(out[uni][0], xo) for uni in (1, 0)}
    e_kr = _rel(out[1][0], out[0][0])
    print(f"ho_uniform {shape} p={p} kinds={kinds}: vs oracle {e_or[1]:.3e} (Kronecker form {e_or[0]:.3e}), "
          f"vs Kronecker form {e_kr:.3e}")
    for uni in (1, 0):
        assert out[uni][1]["iterations"] == iters
    return e_or, e_kr


@pytest.mark.parametrize("shape,p,kinds", [((2, 2, 4), 4, 7), ((3, 3, 5), 4, 7), ((4, 4, 8), 4, 7), ((3, 5, 6), 4, 5),
                                           ((5, 3, 7), 3, 7), ((4, 2, 9), 3, 5)])
def test_ho_uniform_parity(gpu_ctx, shape, p, kinds):
    """One full block, partial blocks on every axis, several blocks; kinds 7 and 5; non-zero essential
    values: 40 fixed Jacobi-CG iterates of the dense matrix-core apply against the oracle (1e-11) and
    against the Kronecker form on the same blocks (1e-12), bitwise repeatable; the kernel's name, its
    2 nd^2 ne flops and the bytes without the factor stream.  Unknown key on the code before ho_uniform."""
    e_or, e_kr = _both_forms(gpu_ctx, O.BoxMesh(3, shape, p), shape, p, kinds, 41)
    assert e_or[1] <= 1e-11
    assert e_kr <= TOL_KRON


@pytest.mark.parametrize("shape,p", [((3, 3, 5), 4), ((5, 3, 7), 3)])
def test_ho_uniform_natural_faces_partial_blocks(gpu_ctx, shape, p):
    """Natural boundary on the x = 1, y = 1 and z = 1 faces of a box with partial blocks there: the dofs
    on those faces are free, so an element slot outside the box that was not masked would add its
    (non-zero) product into them and into den."""
    om = O.BoxMesh(3, shape, p)
    xyz = om.dof_coords()
    bdr = om.bdr.copy()
    bdr[np.any(np.abs(xyz - 1.0) < 1e-12, axis=1)] = 0
    assert 0 < np.count_nonzero(bdr) < np.count_nonzero(om.bdr)
    e_or, e_kr = _both_forms(gpu_ctx, om, shape, p, 7, 43, bdr=bdr)
    assert e_or[1] <= 1e-11
    assert e_kr <= TOL_KRON
    assert e_or[0] <= 1e-11  # (the Kronecker form on the same problem)


def test_ho_uniform_grid_independence(gpu_ctx):
    """12 blocks walked by 5 workgroups (an uneven remainder), by 1 and by the automatic grid: bitwise
    equal iterates.  A negative grid is refused."""
    shape, p, kinds = (4, 4, 12), 4, 7
    om = O.BoxMesh(3, shape, p)
    rng = np.random.default_rng(47)
    u = np.zeros(om.nl)
    u[om.ess] = rng.uniform(-1, 1, len(om.ess))
    b = rng.uniform(-1, 1, om.nl)
    out = {}
    try:
        _setup(gpu_ctx, om, shape, p, kinds, om.ess)
        assert gpu_ctx.kernel_name(cdfem.K_APPLY) == UM
        _, B = gpu_ctx.form_linear_system(u, b)
        for grid in (5, 1, 0):
            gpu_ctx.set_option("ho_uniform_grid", grid)
            out[grid] = _fixed(gpu_ctx, B, 25)
        with pytest.raises(cdfem.CdfemError):
            gpu_ctx.set_option("ho_uniform_grid", -1)
    finally:
        _restore(gpu_ctx)
    assert np.all(np.isfinite(out[0][0])) and np.linalg.norm(out[0][0]) > 0
    np.testing.assert_array_equal(out[5][0], out[0][0])
    np.testing.assert_array_equal(out[1][0], out[0][0])


@pytest.mark.parametrize("case", ["graded", "block_z2"])
def test_ho_uniform_fallbacks(gpu_ctx, case):
    """A box graded along x and y (affine, element sizes differ) and a uniform box on 2^3 blocks keep the
    Kronecker form with ho_uniform 1: its kernel name, its bytes, and 30 iterates on the oracle's (1e-11)."""
    shape, p, kinds = (4, 3, 5), 4, 7
    om = O.BoxMesh(3, shape, p)
    if case == "graded":
        v = om.verts.copy()
        v[..., 0] = v[..., 0] ** 1.5
        v[..., 1] = 0.5 * (v[..., 1] + v[..., 1] ** 2)
        om.verts = np.ascontiguousarray(v)
    bz = 2 if case == "block_z2" else 4
    Ac, Bo, u, b, ess = _problem(om, kinds, 11)
    xo, _ = O.cg(Ac, Bo, dinv=1.0 / Ac.diag(), rel_tol=0.0, abs_tol=0.0, max_iter=30)
    nbytes = {}
    try:
        for uni in (1, 0):
            _setup(gpu_ctx, om, shape, p, kinds, ess, bz=bz, uni=uni)
            assert gpu_ctx.kernel_name(cdfem.K_APPLY) == KRON
            nbytes[uni] = gpu_ctx.kernel_bytes(cdfem.K_APPLY)
            _, B = gpu_ctx.form_linear_system(u, b)
            xg, ig = _fixed(gpu_ctx, B, 30)
            assert ig["iterations"] == 30
            assert _rel(xg, xo) <= 1e-11, uni
    finally:
        _restore(gpu_ctx)
    assert nbytes[1] == nbytes[0]


def test_ho_uniform_ignored_at_p2(gpu_ctx):
    """A p = 2 box ignores the option: the same kernel name and bytes as without it."""
    shape, p = (4, 4, 4), 2
    om = O.BoxMesh(3, shape, p)
    seen = {}
    try:
        for uni in (1, 0):
            _setup(gpu_ctx, om, shape, p, 7, om.ess, uni=uni)
            seen[uni] = (gpu_ctx.kernel_name(cdfem.K_APPLY), gpu_ctx.kernel_bytes(cdfem.K_APPLY))
    finally:
        _restore(gpu_ctx)
    assert seen[1] == seen[0] and seen[0][0] == "k_brick_cg"


def test_ho_uniform_converging_spd(gpu_ctx):
    """kK + sM (kinds 5, SPD): a converging Jacobi-CG solve (rel_tol 1e-10) stops on the Kronecker form's
    iteration, within one of the oracle's, and matches the oracle's solution (1e-9)."""
    shape, p, kinds = (4, 4, 8), 4, 5
    om = O.BoxMesh(3, shape, p)
    Ac, Bo, u, b, ess = _problem(om, kinds, 5)
    xo, io = O.cg(Ac, Bo, dinv=1.0 / Ac.diag(), rel_tol=1e-10, max_iter=2000)
    out = {}
    try:
        _setup(gpu_ctx, om, shape, p, kinds, ess)
        _, B = gpu_ctx.form_linear_system(u, b)
        for uni in (1, 0):
            gpu_ctx.set_option("ho_uniform", uni)
            assert gpu_ctx.kernel_name(cdfem.K_APPLY) == (UM if uni else KRON)
            out[uni] = gpu_ctx.solve(B, method="cg", pc="jacobi", rel_tol=1e-10, max_iter=2000, check_every=7)
    finally:
        _restore(gpu_ctx)
    assert out[1][1]["converged"] and out[1][1]["iterations"] == out[0][1]["iterations"]
    assert abs(out[1][1]["iterations"] - io["iterations"]) <= 1
    assert _rel(out[1][0], xo) <= 1e-9


def test_ho_uniform_mid_size_host_pa(gpu_ctx):
    """16^3 elements at p = 4 (256 blocks, the interior ones on the no-essential-dof shortcut), kinds 7, zero
    essential values: 20 fixed Jacobi-CG iterates against the oracle's host partial assembly (1e-11)."""
    n, p = 16, 4
    om = O.BoxMesh(3, n, p)
    pa = O.PA(om, kappa=0.1, alpha=1.0, s=1.0, c=C3, kinds=7)
    ess = om.bdr != 0
    dinv = np.where(ess, 1.0, 1.0 / np.where(ess, 1.0, pa.diag()))
    b = np.random.default_rng(20261015).uniform(-1, 1, om.nl)
    u = np.zeros(om.nl)
    Bo = pa.form_linear_system(u, b)
    xo, io = pa.cg(Bo, dinv=dinv, rel_tol=0.0, abs_tol=0.0, max_iter=20)
    try:
        _setup(gpu_ctx, om, (n, n, n), p, 7, om.ess)
        assert gpu_ctx.kernel_name(cdfem.K_APPLY) == UM
        xg, ig = _fixed(gpu_ctx, Bo, 20)
    finally:
        _restore(gpu_ctx)
    assert io["iterations"] == ig["iterations"] == 20
    print(f"ho_uniform 16^3 p=4 vs host PA: {_rel(xg, xo):.3e}")
    assert _rel(xg, xo) <= 1e-11
