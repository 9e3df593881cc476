"""Geometric factors formed inside the high-order tile apply (set_option "ho_geom").

The p = 3, 4 sibling of `pa_geom` (tests/test_gpu_geom_fly.py): with constant coefficients on a hex mesh
the affine forms do not take, `ho_geom` 1 keeps 24 doubles per element (the coefficients a1..a7 of the
trilinear map, element-major) and k_apply3d_tile (mode bit 32) forms J, adj J, det J and the point
operator per quadrature plane in registers instead of streaming 8 * nc * Q1^3 bytes per element.
Checked on perturbed boxes (no element a parallelepiped) whose element counts give several elements per
wave and a partial last block (p = 4: 24 elements = 3 blocks of 7 + 3 and the idle threads 252-255;
p = 3: 36 elements = 3 blocks of 10 + 6), against the oracle's assembled matrix and against the stream
(ho_geom 0): Mult at the parity ladder's 1e-13, fixed Krylov iterates at 1e-11 (oracle) and 1e-12 (between
two forms of the operator).  The oracle bound is asserted on the ho_geom 0 leg too, so a miss by the stream
itself shows as such.  The cases the option must leave alone keep their byte counts.
"""
import os

import numpy as np
import pytest

import cdfem
from oracle import oracle as O

pytestmark = pytest.mark.gpu
C3 = (1.0, -2.0, 0.5)
MULT_TOL = 1e-13   # test_gpu_parity.py's Mult bound
ORACLE_TOL = 1e-11  # fixed Krylov iterates against the oracle
FORM_TOL = 1e-12    # ... between two forms of the operator
KAPPA = 0.1
PERT = 0.1
SHAPES = {4: (3, 4, 2), 3: (4, 3, 3)}
ORDERS = [4, 3]


def _kinds_o(k):
    return (O.DIFFUSION if k & 1 else 0) | (O.CONVECTION if k & 2 else 0) | (O.MASS if k & 4 else 0)


def _relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _relnorm(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


_MESHES = {}


def _mesh(shape, p, perturb=PERT, dim=3):
    key = (shape, p, perturb, dim)
    if key not in _MESHES:
        _MESHES[key] = O.BoxMesh(dim, shape, p, perturb=perturb)
    return _MESHES[key]


class _Problem:
    """One operator on one mesh: the oracle's matrix, inputs and references, computed once."""

    def __init__(self, om, kinds, ess=None, seed=3):
        self.om, self.kinds = om, kinds
        self.ess = om.ess if ess is None else np.asarray(ess, dtype=np.int32)
        self.bdr = np.zeros(om.nl, dtype=np.int32)
        self.bdr[self.ess] = 1
        self.A = O.fa_assemble(om, kappa=KAPPA, alpha=1.0, s=1.0, c=C3[:om.dim], kinds=_kinds_o(kinds))
        rng = np.random.default_rng(seed + 10 * kinds + om.p)
        self.x = rng.uniform(-1, 1, om.nl)
        self.u = np.zeros(om.nl)
        self.u[self.ess] = rng.uniform(-1, 1, len(self.ess))
        self.b = rng.uniform(-1, 1, om.nl)
        self.y = self.A.mult(self.x)
        xz = self.x.copy()
        xz[self.ess] = 0.0
        self.yc = self.A.mult(xz)
        self.yc[self.ess] = self.x[self.ess]
        self._sys = None
        self._ref = {}

    def system(self):
        if self._sys is None:
            Ac, B = O.form_linear_system(self.A, self.bdr, self.u, self.b)
            self._sys = (Ac, B, 1.0 / Ac.diag())
        return self._sys

    def cg(self, iters):
        if ("cg", iters) not in self._ref:
            Ac, B, dinv = self.system()
            self._ref["cg", iters] = O.cg(Ac, B, dinv=dinv, rel_tol=0.0, abs_tol=0.0, max_iter=iters)[0]
        return self._ref["cg", iters]

    def gmres(self, iters):
        if ("gmres", iters) not in self._ref:
            Ac, B, dinv = self.system()
            self._ref["gmres", iters] = O.gmres(Ac, B, dinv=dinv, restart=30, rtol=0.0, atol=0.0, max_it=iters)[0]
        return self._ref["gmres", iters]


_PROBLEMS = {}


def _problem(p, kinds):
    key = (p, kinds)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _Problem(_mesh(SHAPES[p], p), kinds)
    return _PROBLEMS[key]


def _setup(ctx, pr, shape, structured, geom, **kw):
    """Upload + PA setup with ho_geom = geom (the caller restores 0)."""
    om = pr.om
    ctx.set_option("ho_geom", geom)
    ctx.upload_mesh(cdfem.Mesh(om.dim, om.p, om.verts, om.dofmap, om.nl, pr.ess))
    if structured:
        ctx.set_structured(*shape)
    ctx.pa_setup(kinds=pr.kinds, kappa=KAPPA, alpha=1.0, conv=C3[:om.dim], mass=1.0, **kw)
    return ctx


def _check_mult(ctx, pr, shape, structured):
    """Mult and constrained Mult with ho_geom 1 against the oracle and against ho_geom 0; accounting."""
    out = {}
    try:
        for geom in (1, 0):
            _setup(ctx, pr, shape, structured, geom)
            o = dict(bytes=ctx.kernel_bytes(cdfem.K_APPLY), flops=ctx.kernel_flops(cdfem.K_APPLY),
                     name=ctx.kernel_name(cdfem.K_APPLY))
            o["y"] = ctx.mult(pr.x)
            o["yc"] = ctx.mult(pr.x, constrained=True)
            out[geom] = o
    finally:
        ctx.set_option("ho_geom", 0)
    for geom in (1, 0):
        ey, eyc = _relmax(out[geom]["y"], pr.y), _relmax(out[geom]["yc"], pr.yc)
        print(f"ho_geom {geom}: mult vs oracle {ey:.3e}, constrained {eyc:.3e}")
        assert np.isfinite(out[geom]["y"]).all() and np.isfinite(out[geom]["yc"]).all()
        assert ey <= MULT_TOL, geom
        assert eyc <= MULT_TOL, geom
    d, dc = _relmax(out[1]["y"], out[0]["y"]), _relmax(out[1]["yc"], out[0]["yc"])
    print(f"ho_geom 1 vs 0: mult {d:.3e}, constrained {dc:.3e}; bytes {out[1]['bytes']:.0f} / {out[0]['bytes']:.0f}, "
          f"flops {out[1]['flops']:.0f} / {out[0]['flops']:.0f}")
    assert d <= MULT_TOL and dc <= MULT_TOL
    assert out[1]["bytes"] < out[0]["bytes"]
    assert out[1]["flops"] > out[0]["flops"]
    assert out[1]["name"] == out[0]["name"] == "k_apply3d_tile"
    # the qdata term alone: 8 * 24 B per element against the stream's 8 nc Q1^3
    om = pr.om
    nc = (6 if pr.kinds & 1 else 0) + (3 if pr.kinds & 2 else 0) + (1 if pr.kinds & 4 else 0)
    assert out[0]["bytes"] - out[1]["bytes"] == 8.0 * om.ne * (nc * (om.p + 2) ** 3 - 24)


def _solve(ctx, pr, method, iters):
    _, B = ctx.form_linear_system(pr.u, pr.b)
    if method == "cg":
        x, info = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=iters)
    else:
        x, info = ctx.solve(B, method="gmres", pc="jacobi", restart=30, rel_tol=0.0, abs_tol=0.0, max_iter=iters)
    assert info["iterations"] == iters
    return x


def _check_krylov(ctx, pr, shape, method, iters):
    """Fixed iterates with ho_geom 1 (twice) and 0: against the oracle (both legs) and against each other."""
    xo = pr.cg(iters) if method == "cg" else pr.gmres(iters)
    try:
        _setup(ctx, pr, shape, True, 1)
        # the geometry form is on: all the apply's bytes are fewer than the stream's qdata alone (kinds 7: nc 10)
        assert pr.kinds == 7 and ctx.kernel_bytes(cdfem.K_APPLY) < 8.0 * 10 * pr.om.ne * (pr.om.p + 2) ** 3
        x1 = _solve(ctx, pr, method, iters)
        x1b = _solve(ctx, pr, method, iters)
        _setup(ctx, pr, shape, True, 0)
        x0 = _solve(ctx, pr, method, iters)
    finally:
        ctx.set_option("ho_geom", 0)
    e1, e0, es = _relnorm(x1, xo), _relnorm(x0, xo), _relnorm(x1, x0)
    print(f"{iters} {method} iterates: ho_geom 1 vs oracle {e1:.3e}, ho_geom 0 vs oracle {e0:.3e}, 1 vs 0 {es:.3e}")
    assert np.isfinite(x1).all()
    assert e0 <= ORACLE_TOL, "the stream (ho_geom 0) misses the oracle"
    assert e1 <= ORACLE_TOL
    assert es <= FORM_TOL
    assert np.array_equal(x1, x1b)


# ---------------------------------------------------------------------------------------------
# 1. Mult parity, structured (lattice gather, pencil E-vector)
@pytest.mark.parametrize("kinds", [7, 5, 2, 1])
@pytest.mark.parametrize("p", ORDERS)
def test_mult_structured(gpu_ctx, p, kinds):
    _check_mult(gpu_ctx, _problem(p, kinds), SHAPES[p], structured=True)


# ---------------------------------------------------------------------------------------------
# 2. generic path: no set_structured, the element map gather and the element-major E-vector
@pytest.mark.parametrize("p", ORDERS)
def test_mult_generic(gpu_ctx, p):
    _check_mult(gpu_ctx, _problem(p, 7), SHAPES[p], structured=False)


# ---------------------------------------------------------------------------------------------
# 3. CG, one rank, structured: the fused apply with den partials
@pytest.mark.parametrize("p", ORDERS)
def test_cg_structured(gpu_ctx, p):
    _check_krylov(gpu_ctx, _problem(p, 7), SHAPES[p], "cg", 40)


def test_cg_one_essential_face(gpu_ctx):
    """Only the x = 0 face is essential: the den ownership term sees non-zero inputs on the max faces."""
    p = 4
    om = _mesh(SHAPES[p], p)
    ess = np.nonzero(np.abs(om.dof_coords()[:, 0]) < 1e-12)[0].astype(np.int32)
    assert 0 < len(ess) < len(om.ess)
    pr = _Problem(om, 7, ess=ess, seed=5)
    _check_mult(gpu_ctx, pr, SHAPES[p], structured=True)
    _check_krylov(gpu_ctx, pr, SHAPES[p], "cg", 40)


# ---------------------------------------------------------------------------------------------
# 4. GMRES(30): the structured Mult
def test_gmres_structured(gpu_ctx):
    _check_krylov(gpu_ctx, _problem(4, 7), SHAPES[4], "gmres", 40)


# ---------------------------------------------------------------------------------------------
# 5. fallbacks keep their form
def _bytes(ctx, pr, shape, structured, geom, **kw):
    _setup(ctx, pr, shape, structured, geom, **kw)
    return ctx.kernel_bytes(cdfem.K_APPLY)


def test_fallback_affine_keeps_kronecker(gpu_ctx):
    """An unperturbed box: under the default pa_affine 2 the Kronecker form stays; under pa_affine 0
    the new form is taken and its CG iterates match the Kronecker-form run."""
    p = 4
    shape = SHAPES[p]
    pr = _Problem(_mesh(shape, p, perturb=0.0), 7)
    try:
        b0 = _bytes(gpu_ctx, pr, shape, True, 0)
        b1 = _bytes(gpu_ctx, pr, shape, True, 1)
        assert b1 == b0
        assert _relmax(gpu_ctx.mult(pr.x), pr.y) <= MULT_TOL
        xk = _solve(gpu_ctx, pr, "cg", 30)
        gpu_ctx.set_option("pa_affine", 0)
        bs = _bytes(gpu_ctx, pr, shape, True, 0)
        bg = _bytes(gpu_ctx, pr, shape, True, 1)
        yg = gpu_ctx.mult(pr.x)
        xg = _solve(gpu_ctx, pr, "cg", 30)
    finally:
        gpu_ctx.set_option("pa_affine", 2)
        gpu_ctx.set_option("ho_geom", 0)
    assert b0 < bs and bg < bs
    assert _relmax(yg, pr.y) <= MULT_TOL
    e = _relnorm(xg, xk)
    print(f"30 CG iterates, ho_geom form vs Kronecker form {e:.3e}")
    assert e <= FORM_TOL


def test_fallback_point_coefficient_keeps_stream(gpu_ctx):
    p = 3
    shape = SHAPES[p]
    om = _mesh(shape, p)
    pr = _problem(p, 7)
    try:
        _setup(gpu_ctx, pr, shape, True, 0)
        nq = gpu_ctx.rule_size(cdfem.RULE_OPERATOR)
        kq = np.random.default_rng(9).uniform(0.05, 0.2, om.ne * nq)
        b0 = _bytes(gpu_ctx, pr, shape, True, 0, kappa_q=kq)
        b1 = _bytes(gpu_ctx, pr, shape, True, 1, kappa_q=kq)
        y = gpu_ctx.mult(pr.x)
    finally:
        gpu_ctx.set_option("ho_geom", 0)
    assert b1 == b0
    # (kappa_q replaces the constant: the library takes kappa_q where given)
    A = O.fa_assemble_q(om, kappa=KAPPA, kappa_q=kq, alpha=1.0, c=C3, s=1.0, kinds=_kinds_o(7))
    e = _relmax(y, A.mult(pr.x))
    print(f"kappa_q mult vs oracle {e:.3e}")
    assert e <= MULT_TOL


@pytest.mark.parametrize("dim,shape,p", [(3, (3, 4, 2), 2), (2, (5, 4), 3)])
def test_fallback_other_kernels_keep_stream(gpu_ctx, dim, shape, p):
    """The 3D p = 2 apply and the 2D p = 3 apply keep the stream."""
    pr = _Problem(_mesh(shape, p, dim=dim), 7)
    try:
        b0 = _bytes(gpu_ctx, pr, shape, False, 0)
        b1 = _bytes(gpu_ctx, pr, shape, False, 1)
        y = gpu_ctx.mult(pr.x)
    finally:
        gpu_ctx.set_option("ho_geom", 0)
    assert b1 == b0
    assert _relmax(y, pr.y) <= MULT_TOL


def test_fallback_mfma_keeps_stream(gpu_ctx):
    """The matrix-core stage variants (ho_mfma 1) keep the stream."""
    p = 4
    shape = SHAPES[p]
    pr = _problem(p, 7)
    try:
        gpu_ctx.set_option("ho_mfma", 1)
        b0 = _bytes(gpu_ctx, pr, shape, True, 0)
        b1 = _bytes(gpu_ctx, pr, shape, True, 1)
        y = gpu_ctx.mult(pr.x)
        gpu_ctx.set_option("ho_mfma", 0)
        bg = gpu_ctx.kernel_bytes(cdfem.K_APPLY)  # ho_mfma is read by the apply: the geometry form is back
    finally:
        gpu_ctx.set_option("ho_mfma", 0)
        gpu_ctx.set_option("ho_geom", 0)
    assert b1 == b0
    assert bg < b0
    assert _relmax(y, pr.y) <= MULT_TOL


# ---------------------------------------------------------------------------------------------
# 6. switch back without a setup; invalid values
def test_switch_back_without_setup(gpu_ctx):
    """ho_geom 0 after a setup returns to the stream at once (bytes and values of the stream run)."""
    p = 4
    shape = SHAPES[p]
    pr = _problem(p, 5)
    try:
        _setup(gpu_ctx, pr, shape, True, 0)
        bs, ys = gpu_ctx.kernel_bytes(cdfem.K_APPLY), gpu_ctx.mult(pr.x)
        _setup(gpu_ctx, pr, shape, True, 1)
        bg, yg = gpu_ctx.kernel_bytes(cdfem.K_APPLY), gpu_ctx.mult(pr.x)
        gpu_ctx.set_option("ho_geom", 0)
        assert gpu_ctx.kernel_bytes(cdfem.K_APPLY) == bs and bg < bs
        assert np.array_equal(gpu_ctx.mult(pr.x), ys)
        assert _relmax(yg, ys) <= MULT_TOL
        with pytest.raises(Exception):
            gpu_ctx.set_option("ho_geom", 2)
        with pytest.raises(Exception):
            gpu_ctx.set_option("ho_geom", -1)
        assert gpu_ctx.kernel_bytes(cdfem.K_APPLY) == bs  # a refused value changes nothing
    finally:
        gpu_ctx.set_option("ho_geom", 0)


# ---------------------------------------------------------------------------------------------
# 7. z slabs: two ranks on one GPU through the host-callback communicator (gloo)
SLAB_SHAPE, SLAB_P, SLAB_SPLIT, SLAB_ITERS = (4, 3, 6), 3, 3, 30


def _slab_worker(rank, world, rdv, out_dir):
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "continuum-mechanics-mfem_amd", "python"))
    import cdfem as cd
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{rdv}", rank=rank, world_size=world)
    nx, ny, nz = SLAB_SHAPE
    z0, z1 = (0, SLAB_SPLIT) if rank == 0 else (SLAB_SPLIT, nz)
    m = cd.box_mesh(3, SLAB_SHAPE, SLAB_P, z_range=(z0, z1), perturb=PERT)
    ctx = cd.Context(0)
    try:
        ctx.set_option("ho_geom", 1)
        ctx.upload_mesh(m).set_structured(nx, ny, z1 - z0)
        ctx.comm_init_torch()
        ctx.set_slab(rank > 0, rank < world - 1)
        ctx.pa_setup(kinds=cd.DIFFUSION | cd.MASS, kappa=KAPPA, mass=1.0)
        stream = 8.0 * 7 * (SLAB_P + 2) ** 3 * m.ne
        took = ctx.kernel_bytes(cd.K_APPLY) < stream
        b = np.random.default_rng(100 + rank).uniform(-1, 1, m.nl)
        _, B = ctx.form_linear_system(np.zeros(m.nl), b)
        X, info = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=SLAB_ITERS)
        np.save(os.path.join(out_dir, f"b{rank}.npy"), b)
        np.save(os.path.join(out_dir, f"x{rank}.npy"), X)
        np.save(os.path.join(out_dir, f"info{rank}.npy"), np.array([info["iterations"], int(took)]))
    finally:
        ctx.close()
        dist.destroy_process_group()


def test_slab_two_ranks_one_device(tmp_path):
    import tempfile

    import torch.multiprocessing as mp
    fd, rdv = tempfile.mkstemp(prefix="cdfem_rdv_")
    os.close(fd)
    os.unlink(rdv)  # the file store creates it
    mp.start_processes(_slab_worker, args=(2, rdv, str(tmp_path)), nprocs=2, start_method="spawn", join=True)
    nx, ny, nz = SLAB_SHAPE
    plane = (SLAB_P * nx + 1) * (SLAB_P * ny + 1)
    b0, b1 = np.load(tmp_path / "b0.npy"), np.load(tmp_path / "b1.npy")
    x0, x1 = np.load(tmp_path / "x0.npy"), np.load(tmp_path / "x1.npy")
    for r in range(2):
        its, took = np.load(tmp_path / f"info{r}.npy")
        assert its == SLAB_ITERS and took == 1
    # the single-domain right-hand side = the sum of the rank-local (partial) L-vectors
    bfull = np.concatenate([b0, np.zeros(len(b1) - plane)])
    bfull[len(b0) - plane:] += b1
    xg = np.concatenate([x0, x1[plane:]])
    m = cdfem.box_mesh(3, SLAB_SHAPE, SLAB_P, perturb=PERT)
    assert len(xg) == m.nl
    # one rank, ho_geom 1
    with cdfem.Context(0) as ctx:
        ctx.set_option("ho_geom", 1)
        ctx.upload_mesh(m).set_structured(nx, ny, nz)
        ctx.pa_setup(kinds=cdfem.DIFFUSION | cdfem.MASS, kappa=KAPPA, mass=1.0)
        assert ctx.kernel_bytes(cdfem.K_APPLY) < 8.0 * 7 * (SLAB_P + 2) ** 3 * m.ne
        _, B = ctx.form_linear_system(np.zeros(m.nl), bfull)
        xs, info = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=SLAB_ITERS)
    assert info["iterations"] == SLAB_ITERS
    # the oracle on the same (library-generated) mesh
    om = O.BoxMesh(3, 1, SLAB_P)
    om.verts, om.dofmap, om.ne, om.nl = m.verts, m.dofmap, m.ne, m.nl
    bdr = np.zeros(m.nl, dtype=np.int32)
    bdr[m.ess] = 1
    A = O.fa_assemble(om, kappa=KAPPA, s=1.0, kinds=O.DIFFUSION | O.MASS)
    Ac, Bo = O.form_linear_system(A, bdr, np.zeros(m.nl), bfull)
    xo, _ = O.cg(Ac, Bo, dinv=1.0 / Ac.diag(), rel_tol=0.0, abs_tol=0.0, max_iter=SLAB_ITERS)
    e1, eo = _relnorm(xg, xs), _relnorm(xg, xo)
    print(f"two ranks: vs one rank {e1:.3e}, vs oracle {eo:.3e}; interface copies "
          f"{np.abs(x1[:plane] - x0[-plane:]).max():.3e}")
    assert e1 <= FORM_TOL
    assert eo <= ORACLE_TOL
