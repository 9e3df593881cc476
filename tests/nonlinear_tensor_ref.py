"""numpy / scipy restatement of the nonlinear heat form on quads and hexes (the matrix-free path of
cdfem_nl_pa_setup).  Test code only: what tests/test_gpu_nonlinear_pa.py compares the HIP path with, pinned on
its own by tests/test_nonlinear_tensor_ref.py.  The form, the elimination and the Newton loop are
tests/nonlinear_ref.py's (HeatForm); what differs is the element:

    the basis    tensor products of the 1D Lagrange basis on the Gauss-Lobatto nodes (oracle.gll_nodes), from the
                 product formula, local dof i = dx + (p + 1) dy (+ (p + 1)^2 dz);
    the rule     tensor Gauss-Legendre on [0, 1] with p + 2 (quads) / p + 3 (hexes) points per direction, point
                 q = qx + n qy (+ n^2 qz): IntRules.Get(geom, 2p + OrderW + 2) with OrderW = p_geom dim - 1 of the
                 multilinear geometry, so order 2p + 3 / 2p + 4, and (order | 1) // 2 + 1 points per direction;
    the map      the multilinear map of the 2^dim vertices (vertex v = bits (x, y, z), x fastest), J, det J and
                 the physical gradients at every point.

Everything is dense per-element einsums over all elements at once.  dtype=np.longdouble runs the same formulas
in extended precision (the tables are formed there and rounded only to dtype)."""
import numpy as np
import scipy.sparse as sp

import nonlinear_ref as NR
from oracle import oracle as O


def points_1d(dim, p):
    """Points per direction of the nonlinear form's rule."""
    order = 2 * p + (dim - 1) + 2            # 2p + OrderW + 2, OrderW = 1 * dim - 1
    return (order | 1) // 2 + 1


def gauss_01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def lagrange_1d(p, x):
    """B[q, d] = phi_d(x_q), G[q, d] = phi_d'(x_q) of the Lagrange basis on the GLL nodes of order p: the product
    formula, in long double."""
    nodes = O.gll_nodes(p).astype(np.longdouble)
    x = np.asarray(x, dtype=np.longdouble)
    B = np.ones((len(x), p + 1), dtype=np.longdouble)
    G = np.zeros((len(x), p + 1), dtype=np.longdouble)
    for d in range(p + 1):
        for m in range(p + 1):
            if m != d:
                B[:, d] *= (x - nodes[m]) / (nodes[d] - nodes[m])
        for k in range(p + 1):
            if k == d:
                continue
            t = np.ones(len(x), dtype=np.longdouble) / (nodes[d] - nodes[k])
            for m in range(p + 1):
                if m != d and m != k:
                    t *= (x - nodes[m]) / (nodes[d] - nodes[m])
            G[:, d] += t
    return B, G


def _tensor(dim, fx, fy, fz=None):
    """f[q, i] = fx[qx, dx] fy[qy, dy] (fz[qz, dz]), q and i lexicographic with x fastest."""
    if dim == 2:
        return np.einsum("ya,xb->yxab", fy, fx).reshape(fy.shape[0] * fx.shape[0], -1)
    return np.einsum("zc,ya,xb->zyxcab", fz, fy, fx).reshape(fz.shape[0] * fy.shape[0] * fx.shape[0], -1)


def tables(dim, p, n):
    """xi (nq, dim), w (nq), phi (nq, nd), dphi (nq, nd, dim) in long double."""
    x, w = gauss_01(n)
    B, G = lagrange_1d(p, x)
    xl, wl = x.astype(np.longdouble), w.astype(np.longdouble)
    one = np.ones((n, 1), dtype=np.longdouble)
    if dim == 2:
        xi = np.stack([_tensor(2, xl[:, None], one)[:, 0], _tensor(2, one, xl[:, None])[:, 0]], axis=1)
        wq = _tensor(2, wl[:, None], wl[:, None])[:, 0]
        phi = _tensor(2, B, B)
        dphi = np.stack([_tensor(2, G, B), _tensor(2, B, G)], axis=2)
    else:
        xi = np.stack([_tensor(3, xl[:, None], one, one)[:, 0], _tensor(3, one, xl[:, None], one)[:, 0],
                       _tensor(3, one, one, xl[:, None])[:, 0]], axis=1)
        wq = _tensor(3, wl[:, None], wl[:, None], wl[:, None])[:, 0]
        phi = _tensor(3, B, B, B)
        dphi = np.stack([_tensor(3, G, B, B), _tensor(3, B, G, B), _tensor(3, B, B, G)], axis=2)
    return xi, wq, phi, dphi


def shape_q1(dim, xi):
    """N (npts, 2^dim) and dN (npts, 2^dim, dim) of the multilinear vertex functions at xi (npts, dim)."""
    nv = 1 << dim
    N = np.ones((len(xi), nv), dtype=xi.dtype)
    dN = np.ones((len(xi), nv, dim), dtype=xi.dtype)
    for v in range(nv):
        for k in range(dim):
            bit = (v >> k) & 1
            f = xi[:, k] if bit else 1 - xi[:, k]
            df = 1.0 if bit else -1.0
            N[:, v] *= f
            for m in range(dim):
                dN[:, v, m] *= df if m == k else f
    return N, dN


def _adjugate(J):
    """adj(J) and det J of (..., dim, dim) matrices: inv(J) = adj / det."""
    dim = J.shape[-1]
    A = np.empty_like(J)
    if dim == 2:
        A[..., 0, 0], A[..., 0, 1] = J[..., 1, 1], -J[..., 0, 1]
        A[..., 1, 0], A[..., 1, 1] = -J[..., 1, 0], J[..., 0, 0]
        return A, J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    for a in range(3):
        for b in range(3):
            r = [k for k in range(3) if k != b]
            c = [k for k in range(3) if k != a]
            A[..., a, b] = (-1) ** (a + b) * (J[..., r[0], c[0]] * J[..., r[1], c[1]] - J[..., r[0], c[1]] * J[..., r[1], c[0]])
    return A, J[..., 0, 0] * A[..., 0, 0] + J[..., 0, 1] * A[..., 1, 0] + J[..., 0, 2] * A[..., 2, 0]


class TensorHeatForm(NR.HeatForm):
    """nonlinear_ref.HeatForm on a quad / hex mesh (its eliminate, linear_solve and newton are used as they
    are).  nq1: points per direction instead of the rule's."""

    def __init__(self, mesh, dt, a0, a1, m0, m1, u_ref=0.0, ess=(), nq1=None, dtype=np.float64):
        self.dim, self.p, verts, self.dofmap, self.nl = NR._space(mesh)
        self.dt, self.a0, self.a1, self.m0, self.m1, self.u_ref = dt, a0, a1, m0, m1, u_ref
        self.dtype = dtype
        self.ess = np.zeros(self.nl, dtype=bool)
        self.ess[np.asarray(ess, dtype=np.int64)] = True
        self.nq1 = points_1d(self.dim, self.p) if nq1 is None else nq1
        xi, w, phi, dphi = tables(self.dim, self.p, self.nq1)
        _, dN = shape_q1(self.dim, xi)
        V = np.asarray(verts).astype(np.longdouble)
        J = np.einsum("evk,qvm->eqkm", V, dN)               # J[k, m] = d x_k / d xi_m
        A, det = _adjugate(J)                               # d xi_a / d x_k = A[a, k] / det
        self.xi = xi.astype(np.float64)
        self.phi = phi.astype(dtype)
        self.W = (w * det).astype(dtype)                    # (ne, nq)
        self.gphi = (np.einsum("qia,eqak->eqik", dphi, A) / det[..., None, None]).astype(dtype)
        self.xq = np.einsum("evk,qv->eqk", V, shape_q1(self.dim, xi)[0]).astype(np.float64)
        self.u_old = np.zeros(self.nl)
        self.g = np.zeros(self.nl)
        nd = self.dofmap.shape[1]
        self._rows = np.repeat(self.dofmap, nd, axis=1).ravel()
        self._cols = np.tile(self.dofmap, (1, nd)).ravel()

    def _state(self, u):
        """u, u - u_old and grad u at the points, (ne, nq[, dim]); the two accuracy measures of HeatForm._element:
        the difference per dof before the interpolation, the gradient of u - u(local dof 0)."""
        ue = np.asarray(u, dtype=self.dtype)[self.dofmap]
        de = ue - np.asarray(self.u_old, dtype=self.dtype)[self.dofmap]
        return (ue @ self.phi.T, de @ self.phi.T, np.einsum("eqik,ei->eqk", self.gphi, ue - ue[:, :1]))

    def residual(self, u):
        uq, du, gu = self._state(u)
        mu = self.m0 + self.m1 * (uq - self.u_ref)
        au = self.a0 + self.a1 * (uq - self.u_ref)
        r = (self.W * mu * du / self.dt) @ self.phi + np.einsum("eq,eqik,eqk->ei", self.W * au, self.gphi, gu)
        R = np.zeros(self.nl, dtype=self.dtype)
        np.add.at(R, self.dofmap.ravel(), r.ravel())
        R -= np.asarray(self.g, dtype=self.dtype)
        R[self.ess] = 0.0
        return R

    def jacobian(self, u, eliminated=True):
        uq, du, gu = self._state(u)
        mu = self.m0 + self.m1 * (uq - self.u_ref)
        au = self.a0 + self.a1 * (uq - self.u_ref)
        vals = (np.einsum("eq,qi,qj->eij", self.W * (mu / self.dt + self.m1 * du / self.dt), self.phi, self.phi)
                + np.einsum("eq,eqik,eqjk->eij", self.W * au, self.gphi, self.gphi)
                + np.einsum("eq,qj,eqik,eqk->eij", self.W * self.a1, self.phi, self.gphi, gu))
        A = sp.coo_matrix((vals.astype(np.float64).ravel(), (self._rows, self._cols)), shape=(self.nl, self.nl)).tocsr()
        A.sum_duplicates()
        A.sort_indices()
        return self.eliminate(A) if eliminated else A


def dof_coords(mesh):
    """Physical coordinates of the dofs (nl, dim): the multilinear map at the GLL lattice of each element."""
    dim, p, verts, dofmap, nl = NR._space(mesh)
    g = O.gll_nodes(p)[:, None]
    one = np.ones((p + 1, 1))
    if dim == 2:
        X = np.stack([_tensor(2, g, one)[:, 0], _tensor(2, one, g)[:, 0]], axis=1)
    else:
        X = np.stack([_tensor(3, g, one, one)[:, 0], _tensor(3, one, g, one)[:, 0], _tensor(3, one, one, g)[:, 0]], axis=1)
    N, _ = shape_q1(dim, X)
    xyz = np.zeros((nl, dim))
    xyz[np.asarray(dofmap).ravel()] = np.einsum("lv,evk->elk", N, np.asarray(verts)).reshape(-1, dim)
    return xyz


# ---- the meshes and parameter sets of the two test files ----------------------------------------------------
MESHES = {"quad1": (2, (5, 3), 1), "quad2": (2, (5, 3), 2), "quad3": (2, (4, 3), 3),
          "hex1": (3, (3, 2, 3), 1), "hex2": (3, (3, 2, 3), 2), "hex2L": (3, (5, 4, 3), 2)}


def build_mesh(name, perturb=0.2):
    """cdfem.box_mesh of the unit box (a host-side generator of the binding: an input, not code under test)."""
    import cdfem
    dim, n, p = MESHES[name]
    return cdfem.box_mesh(dim, n, p, perturb=perturb)


def set_a(mesh, xyz):
    """nonlinear_ref.set_a on the unit box: u_old from the dofs' coordinates."""
    u_old = 1.0 + 0.5 * np.sin(np.pi * xyz[:, 0]) * np.cos(np.pi * xyz[:, 1])
    return dict(coeffs=dict(dt=0.1, a0=1.0, a1=0.5, m0=1.0, m1=0.5, u_ref=0.0), scale=1.0, u_old=u_old, flux=0.25)


def set_b(mesh, xyz):
    """nonlinear_ref.set_b: the reference's input, on the unit box scaled to [0, 0.01]^dim."""
    prm = NR.set_b(mesh)
    return dict(coeffs=prm["coeffs"], scale=prm["scale"], u_old=prm["u_old"], flux=prm["flux"])


SETS = {"A": set_a, "B": set_b}


def x1_dofs(mesh):
    """The dofs of the x = 1 face of a unit box (the perturbation leaves the boundary in place)."""
    return np.nonzero(dof_coords(mesh)[:, 0] > 1.0 - 1e-9)[0].astype(np.int32)


def problem(mesh_name, set_name, ess=False, load=True, perturb=0.2, **kw):
    """(mesh on the set's domain, TensorHeatForm with u_old and the load, the set, essential dofs).  Sets A and B
    are nonlinear_ref's (coefficients, u_old, the flux, the scale of the domain); the load is the flux times the
    area of the x = 0 face, spread evenly over that face's dofs (g is any L-vector here: no boundary form on
    tensor faces)."""
    m0 = build_mesh(mesh_name, perturb)
    xyz = dof_coords(m0)
    prm = SETS[set_name](m0, xyz)
    m = NR.scaled(m0, prm["scale"])
    ed = x1_dofs(m0) if ess else np.zeros(0, dtype=np.int32)
    F = TensorHeatForm(m, ess=ed, **prm["coeffs"], **kw)
    F.u_old = np.array(prm["u_old"], dtype=np.float64)
    if load:
        on0 = np.nonzero(xyz[:, 0] < 1e-9)[0]
        F.g = np.zeros(m.nl)
        F.g[on0] = prm["flux"] * prm["scale"] ** (m.dim - 1) / len(on0)
    return m, F, prm, ed


# Newton cases of tests/test_gpu_nonlinear_pa.py: (mesh, set) -> rel_tol, chosen so that no iterate of the
# restatement sits within a factor 3 of a stopping threshold (test_nonlinear_tensor_ref.py checks every case, and
# prints the iterates).  Essential dofs on x = 1, the load on x = 0, u0 = u_old.
# Measured rn / r0 of the iterates (direct solves):
#   quad2 A  1, 6.2e-2, 2.9e-4, 1.0e-8                 1e-7
#   quad3 B  1, 3.3e-1, 1.6e-2, 5.7e-5, 8.2e-10        the reference's 1e-8
#   hex1  B  1, 1.8e-1, 4.2e-3, 3.3e-6, 2.3e-12        1e-4: at 1e-8 the fifth norm, 4.9e-11, is within a factor 3
#                                                       of abs_tol = 1e-10
#   hex2  A  7.3e-1, 3.9e-2, 1.8e-4, 6.2e-9            1e-7
#   hex2  B  1, 4.0e-1, 3.0e-2, 3.2e-4, 4.6e-8         1e-6: the fifth is only a factor 4.6 above 1e-8
NEWTON_CASES = {("quad2", "A"): 1e-7, ("quad3", "B"): 1e-8, ("hex1", "B"): 1e-4, ("hex2", "A"): 1e-7,
                ("hex2", "B"): 1e-6}
NEWTON_ABS_TOL = NR.NEWTON_ABS_TOL
# three backward-Euler steps of quad2, set A: the steps' iterates are at 2.9e-4, 1.0e-8 | 5.3e-6, 2.9e-12 | 2.1e-7,
# 7.1e-15, so 1e-7 and 1e-8 each have an iterate within a factor 3; 1e-9 is decisive (4, 3, 3 iterations)
THREE_STEP_REL_TOL = 1e-9
# hex2, set A with jacobian_rebuild_freq = 2: 7.3e-1, 3.9e-2, 5.2e-3, 5.0e-6, 1.0e-8
FREQ2_REL_TOL = 1e-7
# Residual histories are compared where the restatement's norm exceeds 1e-6 r0.  Measured on the five cases above,
# restatement with a direct solve against restatement with the oracle's GMRES(30) + Jacobi at 1e-13 (25 to 79
# iterations per linear solve): the largest relative spread of those norms is 1.1e-10 (hex1, set B; the others
# 3.8e-14 .. 5.0e-12).  The HIP path differs in summation order as well as in the linear solve: 100 times that
# spread, the margin and the reasoning of nonlinear_ref.HISTORY_TOL.
HISTORY_SPREAD = 1.1e-10
HISTORY_TOL = 100.0 * HISTORY_SPREAD
