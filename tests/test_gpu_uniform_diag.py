"""pa_uniform_diag: the Jacobi scale of the uniform p = 2 brick CG from a 64-entry lattice-class table.

On a uniformly refined box the assembled diagonal depends only on each lattice coordinate's class per axis
(element-interior, shared by two elements, first plane, last plane) and on whether the dof is essential, so
k_brick_cg<XF, BF, FULL, UD> (brick_um.hip) and k_cg_update_faces<..., UD> (brick_kernels.hip) take M^-1
from 64 values in LDS instead of streaming the vector.  Checked as tests/test_gpu_brick_um.py checks the
apply: 40 fixed Jacobi-CG iterates with non-zero essential values and x0 = 0 (r is non-zero on essential
rows from the start, so the 1 there matters) against the oracle (1e-11) and against the streamed vector
(pa_uniform_diag 0, 1e-12: two forms of one operator; the oracle's own sensitivity to replacing every entry
by its class's first is below 1e-15), a second solve bitwise equal to the first, and the update's byte count
telling that the table was taken.  Shapes: one full brick with every boundary class; partial bricks on
anisotropic boxes; essential dofs on x = 0 only (boundary classes whose scale is not 1); the boundary plus
5 % of the interior dofs essential (the essential select in both kernels).  pc = none, a graded box and a
two-rank slab close the set."""
import functools
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import cdfem
from oracle import oracle as O

gpu = pytest.mark.gpu
C3 = (1.0, -2.0, 0.5)
P = 2
ITERS = 40


def _okinds(kinds):
    return ((O.DIFFUSION if kinds & 1 else 0) | (O.CONVECTION if kinds & 2 else 0) | (O.MASS if kinds & 4 else 0))


def _marker(om, ess):
    """bdr: the whole boundary; x0: the x = 0 face only; rand: the boundary plus a seeded 5 % of the interior."""
    if ess == "bdr":
        return np.array(om.bdr, dtype=np.int32)
    if ess == "x0":
        return (np.abs(om.dof_coords()[:, 0]) < 1e-12).astype(np.int32)
    m = np.array(om.bdr, dtype=np.int32)
    inner = np.nonzero(m == 0)[0]
    pick = np.random.default_rng(41).choice(inner, size=max(1, len(inner) // 20), replace=False)
    m[pick] = 1
    return m


@functools.lru_cache(maxsize=None)
def _case(shape, kinds, ess):
    """Mesh, essential marker and the oracle's ITERS fixed Jacobi-CG iterates (computed once per case)."""
    om = O.BoxMesh(3, shape, P)
    marker = _marker(om, ess)
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3, kinds=_okinds(kinds))
    rng = np.random.default_rng(29)
    idx = np.nonzero(marker)[0]
    u = np.zeros(om.nl)
    u[idx] = rng.uniform(-1, 1, len(idx))
    b = rng.uniform(-1, 1, om.nl)
    Ac, Bo = O.form_linear_system(A, marker, u, b)
    xo, _ = O.cg(Ac, Bo, dinv=1.0 / Ac.diag(), rel_tol=0.0, abs_tol=0.0, max_iter=ITERS)
    for a in (xo, u, b, marker):
        a.setflags(write=False)
    return om, marker, xo, u, b


CASES = [((4, 4, 4), 7, "bdr"), ((9, 6, 7), 7, "bdr"), ((5, 9, 10), 5, "bdr"), ((6, 5, 7), 7, "x0"),
         ((6, 5, 7), 5, "x0"), ((5, 4, 6), 7, "rand"), ((5, 4, 6), 5, "rand")]


@pytest.fixture(scope="module")
def ctx():
    """A context of the module's own: the option under test is switched on it, whatever its default."""
    with cdfem.Context(0) as c:
        yield c


def _setup(ctx, om, shape, marker, kinds, verts=None):
    idx = np.nonzero(marker)[0].astype(np.int32)
    ctx.upload_mesh(cdfem.Mesh(3, P, om.verts if verts is None else verts, om.dofmap, om.nl, idx)).set_structured(*shape)
    ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)


def _solves(ctx, B, pc):
    """Solves with the table on and off, and again on; the apply's and update's byte counts after each."""
    out, nbytes = {}, {}
    for ud in (1, 0, 2):
        ctx.set_option("pa_uniform_diag", 1 if ud else 0)
        out[ud] = ctx.solve(B, method="cg", pc=pc, rel_tol=0.0, abs_tol=0.0, max_iter=ITERS, check_every=7)
        nbytes[ud] = (ctx.kernel_bytes(cdfem.K_APPLY), ctx.kernel_bytes(cdfem.K_UPDATE))
        assert out[ud][1]["iterations"] == ITERS
    return out, nbytes


@pytest.mark.parametrize("kinds", [7, 5])
def test_random_essential_oracle_finite(kinds):
    """The oracle's 40 iterates with 5 % of the interior dofs essential are finite and of moderate size (no
    breakdown of the fixed iteration on the non-symmetric kinds 7 either): the reference means something."""
    om, marker, xo, _, _ = _case((5, 4, 6), kinds, "rand")
    assert marker.sum() > np.asarray(om.bdr).sum()
    nx = np.linalg.norm(xo)
    print(f"kinds {kinds}: |x| = {nx:.3e}")
    assert np.all(np.isfinite(xo)) and 0 < nx < 1e6


@gpu
@pytest.mark.parametrize("shape,kinds,ess", CASES)
def test_uniform_diag_iterates(ctx, shape, kinds, ess):
    om, marker, xo, u, b = _case(shape, kinds, ess)
    _setup(ctx, om, shape, marker, kinds)
    _, B = ctx.form_linear_system(u, b)
    out, nbytes = _solves(ctx, B, "jacobi")
    no = np.linalg.norm(xo)
    eo = {ud: np.linalg.norm(out[ud][0] - xo) / no for ud in (1, 0)}
    et = np.linalg.norm(out[1][0] - out[0][0]) / np.linalg.norm(out[0][0])
    print(f"shape {shape} kinds {kinds} ess {ess}: vs oracle table {eo[1]:.3e} vector {eo[0]:.3e}; "
          f"table vs vector {et:.3e}; update bytes {nbytes[1][1]:.0f} / {nbytes[0][1]:.0f}")
    assert nbytes[1][1] != nbytes[0][1]  # the table was taken
    assert nbytes[1][0] != nbytes[0][0]
    np.testing.assert_array_equal(out[2][0], out[1][0])
    assert eo[1] <= 1e-11 and eo[0] <= 1e-11
    assert et <= 1e-12


@gpu
def test_uniform_diag_pc_none():
    """Unpreconditioned CG keeps the ones vector and the present kernels: the option changes neither the
    iterates (bitwise) nor the byte counts."""
    shape = (9, 6, 7)
    om, marker, _, u, b = _case(shape, 7, "bdr")
    with cdfem.Context(0) as c:
        _setup(c, om, shape, marker, 7)
        _, B = c.form_linear_system(u, b)
        out, nbytes = _solves(c, B, "none")
    np.testing.assert_array_equal(out[1][0], out[0][0])
    assert nbytes[1] == nbytes[0]


@gpu
def test_uniform_diag_graded_box(ctx):
    """A graded box (x -> x^2: every element still a box, no two columns alike) has no common element matrix
    and no class table: the option changes neither the byte counts nor the iterates."""
    shape = (5, 4, 6)
    om = O.BoxMesh(3, shape, P)
    verts = np.array(om.verts, dtype=np.float64, copy=True)
    verts[..., 0] = verts[..., 0] ** 2
    _setup(ctx, om, shape, np.asarray(om.bdr), 7, verts=verts)
    b = np.random.default_rng(3).uniform(-1, 1, om.nl)
    _, B = ctx.form_linear_system(np.zeros(om.nl), b)
    out, nbytes = _solves(ctx, B, "jacobi")
    assert nbytes[1] == nbytes[0]
    np.testing.assert_array_equal(out[1][0], out[0][0])


# one two-rank slab (two processes on one device, the host communicator over gloo, as
# tests/test_gpu_brick_um.py): local depths 6 and 5 elements, partial bricks in x and y too, the table on
SL_XY, SL_PER, SL_ITERS = (6, 5), (6, 5), 15


def _slab_worker(rank, world, port, out_dir):
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "continuum-mechanics-mfem_amd", "python"))
    import cdfem
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{port}", rank=rank, world_size=world)
    z0 = sum(SL_PER[:rank])
    m = cdfem.box_mesh(3, (*SL_XY, sum(SL_PER)), P, z_range=(z0, z0 + SL_PER[rank]), with_coords=False)
    ctx = cdfem.Context(0)
    ctx.upload_mesh(m).set_structured(*SL_XY, SL_PER[rank])
    ctx.comm_init_torch()
    ctx.set_slab(rank > 0, rank < world - 1)
    ctx.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    b = np.random.default_rng(700 + rank).uniform(-1, 1, m.nl)
    np.save(os.path.join(out_dir, f"b{rank}.npy"), b)
    _, B = ctx.form_linear_system(np.zeros(m.nl), b)
    ctx.set_option("pa_uniform_diag", 1)
    X, info = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=SL_ITERS, check_every=5)
    assert info["iterations"] == SL_ITERS
    on = ctx.kernel_bytes(cdfem.K_UPDATE)
    ctx.set_option("pa_uniform_diag", 0)
    assert ctx.kernel_bytes(cdfem.K_UPDATE) != on  # the table was taken on this rank
    np.save(os.path.join(out_dir, f"x{rank}.npy"), X)
    ctx.close()
    dist.destroy_process_group()


@gpu
def test_uniform_diag_two_rank_slab(tmp_path):
    """Slabs of 6 and 5 element layers with the table on: both ranks hold the shared plane of x bitwise equal
    (each takes a class's entry at the same (x, y) of the plane), and the gathered iterate equals one
    context's on the union with the streamed vector (1e-12)."""
    import tempfile
    world = 2
    fd, port = tempfile.mkstemp(prefix="cdfem_rdv_")
    os.close(fd)
    os.unlink(port)  # the file store creates it
    mp.start_processes(_slab_worker, args=(world, port, str(tmp_path)), nprocs=world, start_method="spawn", join=True)
    plane = (P * SL_XY[0] + 1) * (P * SL_XY[1] + 1)
    bs = [np.load(tmp_path / f"b{r}.npy") for r in range(world)]
    bfull = np.concatenate([bs[0], bs[1][plane:]])
    bfull[len(bs[0]) - plane:len(bs[0])] += bs[1][:plane]
    shape = (*SL_XY, sum(SL_PER))
    m = cdfem.box_mesh(3, shape, P, with_coords=False)
    with cdfem.Context(0) as c:
        c.upload_mesh(m).set_structured(*shape)
        c.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
        c.set_option("pa_uniform_diag", 0)
        _, B = c.form_linear_system(np.zeros(m.nl), bfull)
        xs, info = c.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=SL_ITERS)
    x0, x1 = np.load(tmp_path / "x0.npy"), np.load(tmp_path / "x1.npy")
    np.testing.assert_array_equal(x1[:plane], x0[-plane:])
    xg = np.concatenate([x0, x1[plane:]])
    err = np.linalg.norm(xg - xs) / np.linalg.norm(xs)
    print(f"two-rank slab, table on: gathered against the union {err:.3e}")
    assert err <= 1e-12
