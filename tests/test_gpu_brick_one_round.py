"""The uniform p = 2 brick CG apply with all 16 bricks of a CU resident at once (brick_um.hip, brick_kernels.hip).

Three changes carry it, each checked here on p = 2 boxes with pa_uniform 1:

- cg_beta_sum (off by default: measured slower): the update's last-arriving workgroup sums the betanom partials
  once, in the order every apply workgroup sums them, and the apply loads that one double.  The iterates are bitwise those of
  cg_beta_sum 0 on an update grid above 64 workgroups that is no multiple of 64 (107) and on one below 64 (20),
  for fixed iteration counts and for a converging solve; the arrival counter is back at 0 after every kind
  of solve end (fixed count, convergence, max_iter 0, 1, 2).
- den from the assembled patch, one LDS patch: 1, 2 and 40 fixed Jacobi-CG iterates against the oracle (1e-11)
  and against the Kronecker form (pa_uniform 0, 1e-12), the bars of tests/test_gpu_brick_um.py and
  tests/test_gpu_uniform_diag.py, on one full-brick box with the whole boundary essential (the bench's
  instantiation), on partial bricks with essential dofs on x = 0 only, and on (9, 6, 7) with kinds 5 and 7; a
  second solve is bitwise equal to the first.
- the two-rank slab of tests/test_gpu_uniform_diag.py (local depths 6 and 5) once more with the defaults: the
  shared plane bitwise equal across the ranks.

Observed on MI355X (relative l2, maxima over 1, 2 and 40 iterates): at most 2.8e-15 to the oracle and 1.7e-15 to
the Kronecker form; profiles/r14/ab_c2_one_round/README.md."""
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
UPD_THREADS = 256  # dofs per update workgroup (one partial each)


def _okinds(kinds):
    return ((O.DIFFUSION if kinds & 1 else 0) | (O.CONVECTION if kinds & 2 else 0) | (O.MASS if kinds & 4 else 0))


@pytest.fixture(scope="module")
def ctx():
    with cdfem.Context(0) as c:
        yield c


def _box(ctx, shape, kinds):
    """The library's own box (whole boundary essential) with a seeded right-hand side."""
    m = cdfem.box_mesh(3, shape, P, with_coords=False)
    ctx.upload_mesh(m).set_structured(*shape)
    ctx.set_option("pa_uniform", 1)
    ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    b = np.random.default_rng(17).uniform(-1, 1, m.nl)
    _, B = ctx.form_linear_system(np.zeros(m.nl), b)
    return m, B


# ---- the betanom sum taken once ---------------------------------------------------------------------
SUM_SHAPES = [((16, 16, 12), 27225, 107), ((8, 8, 8), 4913, 20)]


@gpu
@pytest.mark.parametrize("shape,nl,nwg", SUM_SHAPES)
def test_beta_sum_bitwise(ctx, shape, nl, nwg):
    """cg_beta_sum 1 against 0: x after 30 fixed iterations bit for bit, and a converging SPD solve (kinds 5,
    rel_tol 1e-10) that stops at the same iteration with the same x."""
    m, B = _box(ctx, shape, 7)
    assert m.nl == nl and -(-m.nl // UPD_THREADS) == nwg
    try:
        out = {}
        for bs in (1, 0):
            ctx.set_option("cg_beta_sum", bs)
            out[bs] = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=30, check_every=7)
            assert out[bs][1]["iterations"] == 30
        np.testing.assert_array_equal(out[1][0], out[0][0])
        assert np.all(np.isfinite(out[1][0])) and np.linalg.norm(out[1][0]) > 0
        m, B = _box(ctx, shape, 5)
        for bs in (1, 0):
            ctx.set_option("cg_beta_sum", bs)
            out[bs] = ctx.solve(B, method="cg", pc="jacobi", rel_tol=1e-10, max_iter=500)
            assert out[bs][1]["converged"]
        print(f"shape {shape}: converged after {out[1][1]['iterations']} iterations")
        assert out[1][1]["iterations"] == out[0][1]["iterations"] < 500
        np.testing.assert_array_equal(out[1][0], out[0][0])
    finally:
        ctx.set_option("cg_beta_sum", 0)


@gpu
def test_beta_sum_counter_hygiene(ctx):
    """One context, in turn: a fixed-iteration solve, a solve that stops early by convergence, solves with
    max_iter 0, 1 and 2, then the first solve again: bitwise the first (the arrival counter is 0 after each,
    and a stale sum is never read)."""
    _, B = _box(ctx, (16, 16, 12), 5)
    fixed = dict(method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=30, check_every=7)
    ctx.set_option("cg_beta_sum", 1)
    try:
        x0, i0 = ctx.solve(B, **fixed)
        assert i0["iterations"] == 30
        xc, ic = ctx.solve(B, method="cg", pc="jacobi", rel_tol=1e-6, max_iter=500)
        assert ic["converged"] and ic["iterations"] < 500
        for k in (0, 1, 2):
            xk, ik = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=k)
            assert ik["iterations"] == k and np.all(np.isfinite(xk))
        x1, i1 = ctx.solve(B, **fixed)
        assert i1["iterations"] == 30
        np.testing.assert_array_equal(x1, x0)
    finally:
        ctx.set_option("cg_beta_sum", 0)


# ---- den from the assembled patch, one LDS patch ----------------------------------------------------
ITERS = (1, 2, 40)
DEN_CASES = [((8, 8, 8), 7, "bdr"), ((6, 5, 7), 7, "x0"), ((9, 6, 7), 5, "bdr"), ((9, 6, 7), 7, "bdr")]


@functools.lru_cache(maxsize=None)
def _case(shape, kinds, ess):
    """Mesh, essential marker, data and the oracle's fixed Jacobi-CG iterates (computed once per case)."""
    om = O.BoxMesh(3, shape, P)
    marker = (np.array(om.bdr, dtype=np.int32) if ess == "bdr"
              else (np.abs(om.dof_coords()[:, 0]) < 1e-12).astype(np.int32))
    A = O.fa_assemble(om, kappa=0.1, alpha=1.0, s=1.0, c=C3, kinds=_okinds(kinds))
    rng = np.random.default_rng(29)
    idx = np.nonzero(marker)[0]
    u = np.zeros(om.nl)
    u[idx] = rng.uniform(-1, 1, len(idx))
    b = rng.uniform(-1, 1, om.nl)
    Ac, Bo = O.form_linear_system(A, marker, u, b)
    dinv = 1.0 / Ac.diag()
    xo = {n: O.cg(Ac, Bo, dinv=dinv, rel_tol=0.0, abs_tol=0.0, max_iter=n)[0] for n in ITERS}
    for a in (*xo.values(), u, b, marker):
        a.setflags(write=False)
    return om, marker, xo, u, b


@gpu
@pytest.mark.parametrize("shape,kinds,ess", DEN_CASES)
def test_den_from_patch_iterates(ctx, shape, kinds, ess):
    om, marker, xo, u, b = _case(shape, kinds, ess)
    idx = np.nonzero(marker)[0].astype(np.int32)
    ctx.upload_mesh(cdfem.Mesh(3, P, om.verts, om.dofmap, om.nl, idx)).set_structured(*shape)
    ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    _, B = ctx.form_linear_system(u, b)
    try:
        worst_o = worst_k = 0.0
        for n in ITERS:
            out = {}
            for uni in (1, 0, 2):
                ctx.set_option("pa_uniform", 1 if uni else 0)
                out[uni], info = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=n,
                                           check_every=7)
                assert info["iterations"] == n
            eo = np.linalg.norm(out[1] - xo[n]) / np.linalg.norm(xo[n])
            ek = np.linalg.norm(out[1] - out[0]) / np.linalg.norm(out[0])
            print(f"shape {shape} kinds {kinds} ess {ess}, {n} iterations: vs oracle {eo:.3e}, vs Kronecker form {ek:.3e}")
            worst_o, worst_k = max(worst_o, eo), max(worst_k, ek)
            np.testing.assert_array_equal(out[2], out[1])
            assert eo <= 1e-11
            assert ek <= 1e-12
        print(f"shape {shape} kinds {kinds} ess {ess}: maxima vs oracle {worst_o:.3e}, vs Kronecker form {worst_k:.3e}")
    finally:
        ctx.set_option("pa_uniform", 1)


# ---- the two-rank slab with the defaults ------------------------------------------------------------
# (two processes on one device, the host communicator over gloo, as tests/test_gpu_uniform_diag.py: local
# depths 6 and 5 elements, partial bricks in x and y too)
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
    X, info = ctx.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=SL_ITERS, check_every=5)
    assert info["iterations"] == SL_ITERS
    np.save(os.path.join(out_dir, f"x{rank}.npy"), X)
    ctx.close()
    dist.destroy_process_group()


@gpu
def test_two_rank_slab_defaults(tmp_path):
    """Slabs of 6 and 5 element layers, every option at its default (several ranks keep the partial vector):
    both ranks hold the shared plane of x bitwise equal, and the gathered iterate equals one context's on the
    union (1e-12)."""
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
        _, B = c.form_linear_system(np.zeros(m.nl), bfull)
        xs, info = c.solve(B, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=SL_ITERS)
    x0, x1 = np.load(tmp_path / "x0.npy"), np.load(tmp_path / "x1.npy")
    np.testing.assert_array_equal(x1[:plane], x0[-plane:])
    xg = np.concatenate([x0, x1[plane:]])
    err = np.linalg.norm(xg - xs) / np.linalg.norm(xs)
    print(f"two-rank slab, defaults: gathered against the union {err:.3e}")
    assert err <= 1e-12
