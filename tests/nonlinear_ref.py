"""numpy / scipy restatement of the nonlinear heat form, its boundary load and the Newton loop
(the reference's nonlinear_convection_diffusion_1D.cpp:418-669 and newton_petsc_solver.hpp:180-259).
Test code only: what tests/test_gpu_nonlinear.py compares the HIP path with, pinned on its own by
tests/test_nonlinear_ref.py.

    a(u) = a0 + a1 (u - u_ref),  m(u) = m0 + m1 (u - u_ref),  W = w_q det J, rule of order 2p + 2
    R_i  = sum_e sum_q W [ m(u) (u - u_old) / dt phi_i + a(u) grad u . grad phi_i ] - g_i
    J_ij = sum_e sum_q W [ (m(u) / dt + m1 (u - u_old) / dt) phi_i phi_j + a(u) grad phi_i . grad phi_j
                           + a1 phi_j (grad phi_i . grad u) ]

It loops over the elements and has a Lagrange basis of its own: the nodal basis of the simplex's node set of
order p, from the inverse of the monomial Vandermonde matrix at the nodes (the product's P1 / P2 basis is
written in barycentric coordinates, and it is never called here).  The nodes are the space's: the lattice
points of order p, in the product's local order (vertices, then edge nodes along a -> b for the edges (0,1),
(0,2),(0,3),(1,2),(1,3),(2,3) [2D: (0,1),(0,2),(1,2)], then the P3 centroid), with the two P3 edge nodes at the
Gauss-Lobatto positions t = (1 -+ 1/sqrt 5) / 2, MFEM's H1_FECollection default and what a P3 dof vector of
this project means.  Rules come from oracle.simplex_rule_order (MFEM's tabulated rules)."""
import itertools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import oracle as O

EDGES = {2: [(0, 1), (0, 2), (1, 2)], 3: [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]}


def nodes(dim, p):
    """Reference coordinates of the nodes, local dof order."""
    V = np.vstack([np.zeros(dim), np.eye(dim)])
    X = [V[a] for a in range(dim + 1)]
    if p == 2:
        X += [0.5 * (V[a] + V[b]) for a, b in EDGES[dim]]
    elif p == 3:
        if dim != 2:
            raise ValueError("P3 is a triangle space here")
        ts = [0.5 * (1.0 - 1.0 / np.sqrt(5.0)), 0.5 * (1.0 + 1.0 / np.sqrt(5.0))]
        X += [V[a] + t * (V[b] - V[a]) for a, b in EDGES[2] for t in ts]
        X.append(V.mean(axis=0))
    elif p != 1:
        raise ValueError("order 1..3")
    return np.array(X)


def _exponents(dim, p):
    return [e for e in itertools.product(range(p + 1), repeat=dim) if sum(e) <= p]


def _monomials(dim, p, x):
    """values (npts, nm) and gradients (npts, nm, dim) of the monomials of total degree <= p at x (npts, dim)"""
    ex = _exponents(dim, p)
    val = np.ones((len(x), len(ex)), dtype=x.dtype)
    grad = np.zeros((len(x), len(ex), dim), dtype=x.dtype)
    for c, e in enumerate(ex):
        for k in range(dim):
            val[:, c] *= x[:, k] ** e[k]
        for k in range(dim):
            if e[k] == 0:
                continue
            g = e[k] * x[:, k] ** (e[k] - 1)
            for m in range(dim):
                if m != k:
                    g = g * x[:, m] ** e[m]
            grad[:, c, k] = g
    return val, grad


_COEF = {}


def _coefficients(dim, p):
    """C with phi_i = sum_c m_c C[c, i], in extended precision: the double inverse of the Vandermonde matrix,
    refined by Newton-Schulz steps in long double (the P3 nodes are irrational, so they are formed there too)."""
    if (dim, p) not in _COEF:
        X = nodes(dim, p).astype(np.longdouble)
        if p == 3:
            s5 = np.sqrt(np.longdouble(5))
            V = np.vstack([np.zeros(2), np.eye(2)]).astype(np.longdouble)
            ts = [(1 - 1 / s5) / 2, (1 + 1 / s5) / 2]
            X[3:9] = [V[a] + t * (V[b] - V[a]) for a, b in EDGES[2] for t in ts]
            X[9] = V.sum(axis=0) / 3
        Vm, _ = _monomials(dim, p, X)
        Cm = np.linalg.inv(Vm.astype(np.float64)).astype(np.longdouble)
        eye = np.eye(len(Vm), dtype=np.longdouble)
        for _ in range(3):
            Cm = Cm + Cm @ (eye - Vm @ Cm)
        _COEF[(dim, p)] = Cm
    return _COEF[(dim, p)]


def basis(dim, p, xi):
    """phi (npts, nd) and reference gradients dphi (npts, nd, dim) of the nodal basis at xi (npts, dim): formed
    in long double, rounded to double once.  R interpolates u and grad u from nodal values, and grad u =
    sum_i u_i grad phi_i cancels u's constant part: a table error d costs d |u| / (h |grad u|) of grad u."""
    xi = np.atleast_2d(np.asarray(xi, dtype=np.float64)).astype(np.longdouble)
    Cm = _coefficients(dim, p)
    val, grad = _monomials(dim, p, xi)
    return (val @ Cm).astype(np.float64), np.einsum("qck,ci->qik", grad, Cm).astype(np.float64)


def _space(mesh):
    p = getattr(mesh, "p", None)
    if p is None:
        p = mesh.order
    return mesh.dim, int(p), np.asarray(mesh.verts, dtype=np.float64), np.asarray(mesh.dofmap), int(mesh.nl)


class HeatForm:
    """The form on one mesh: residual, jacobian, newton.  ess: essential dofs (MFEM's NonlinearForm: R zero
    there, J's rows and columns eliminated with a unit diagonal).  rule: (points, weights) instead of the
    tabulated rule of order 2p + 2."""

    def __init__(self, mesh, dt, a0, a1, m0, m1, u_ref=0.0, ess=(), rule=None):
        self.dim, self.p, self.verts, self.dofmap, self.nl = _space(mesh)
        self.dt, self.a0, self.a1, self.m0, self.m1, self.u_ref = dt, a0, a1, m0, m1, u_ref
        self.ess = np.zeros(self.nl, dtype=bool)
        self.ess[np.asarray(ess, dtype=np.int64)] = True
        self.xi, self.w = O.simplex_rule_order(self.dim, 2 * self.p + 2) if rule is None else rule
        self.phi, self.dphi = basis(self.dim, self.p, self.xi)
        self.u_old = np.zeros(self.nl)
        self.g = np.zeros(self.nl)
        nd = self.dofmap.shape[1]
        self._rows = np.repeat(self.dofmap, nd, axis=1).ravel()
        self._cols = np.tile(self.dofmap, (1, nd)).ravel()

    def _element(self, e, u):
        """W (nq), physical gradients gphi (nq, nd, dim), and u, u - u_old, grad u at the points of element e."""
        V = self.verts[e]
        Jm = (V[1:] - V[0]).T                      # J[k, m] = d x_k / d xi_m
        det = np.linalg.det(Jm)
        gphi = self.dphi @ np.linalg.inv(Jm)       # d phi / d x_k = sum_a d phi / d xi_a  d xi_a / d x_k
        d = self.dofmap[e]
        ue = u[d]
        # grad u is taken of u - u(vertex 0) (the basis gradients sum to zero: the same gradient, without the
        # cancellation of u's constant part against the tables' rounding), and
        # u - u_old is interpolated from the dofs' differences: the same function, without the cancellation
        # of two interpolated values (at u ~ 300 that would cost three digits of the mass term)
        return self.w * det, gphi, self.phi @ ue, self.phi @ (ue - self.u_old[d]), np.einsum("qik,i->qk", gphi, ue - ue[0])

    def residual(self, u):
        R = np.zeros(self.nl)
        for e in range(len(self.dofmap)):
            W, gphi, uq, du, gu = self._element(e, u)
            mu = self.m0 + self.m1 * (uq - self.u_ref)
            au = self.a0 + self.a1 * (uq - self.u_ref)
            r = self.phi.T @ (W * mu * du / self.dt) + np.einsum("q,qik,qk->i", W * au, gphi, gu)
            np.add.at(R, self.dofmap[e], r)
        R -= self.g
        R[self.ess] = 0.0
        return R

    def jacobian(self, u, eliminated=True):
        """scipy CSR (sorted columns, the full element pattern with its explicit zeros)."""
        nd = self.dofmap.shape[1]
        vals = np.zeros((len(self.dofmap), nd, nd))
        for e in range(len(self.dofmap)):
            W, gphi, uq, du, gu = self._element(e, u)
            mu = self.m0 + self.m1 * (uq - self.u_ref)
            au = self.a0 + self.a1 * (uq - self.u_ref)
            vals[e] = (np.einsum("q,qi,qj->ij", W * (mu / self.dt + self.m1 * du / self.dt), self.phi, self.phi)
                       + np.einsum("q,qik,qjk->ij", W * au, gphi, gphi)
                       + np.einsum("q,qj,qik,qk->ij", W * self.a1, self.phi, gphi, gu))
        A = sp.coo_matrix((vals.ravel(), (self._rows, self._cols)), shape=(self.nl, self.nl)).tocsr()
        A.sum_duplicates()
        A.sort_indices()
        return self.eliminate(A) if eliminated else A

    def eliminate(self, A):
        A = A.copy()
        rows = np.repeat(np.arange(self.nl), np.diff(A.indptr))
        hit = self.ess[rows] | self.ess[A.indices]
        A.data[hit] = (rows[hit] == A.indices[hit]).astype(np.float64)
        return A

    def linear_solve(self, Jc, b, linear, lin_rtol, lin_atol, lin_max_it):
        """dx of J dx = b: ("direct") sparse LU, or the oracle's PETSc-like GMRES(30) from a zero guess with
        left Jacobi ("gmres_jacobi") or ILU(0) ("gmres_ilu").  Returns (dx, iterations, converged)."""
        if linear == "direct":
            return spla.splu(Jc.tocsc()).solve(b), 0, True
        A = O.csr_from_scipy(Jc)
        if linear == "gmres_ilu":
            x, info = O.gmres_ilu(A, b, O.ilu0(A), rtol=lin_rtol, atol=lin_atol, max_it=lin_max_it)
        else:
            x, info = O.gmres(A, b, dinv=1.0 / Jc.diagonal(), rtol=lin_rtol, atol=lin_atol, max_it=lin_max_it)
        return x, int(info["iterations"]), bool(info["converged"])

    def newton(self, u0, abs_tol=1e-10, rel_tol=1e-8, max_iter=20, jacobian_rebuild_freq=1, linear="direct",
               lin_rtol=1e-13, lin_atol=0.0, lin_max_it=2000):
        """newton_petsc_solver.hpp:180-259.  Returns a dict: u, converged, iterations, the residual norms of
        every iteration (the converged check included), the update norms, r0, du0, linear iterations."""
        u = np.array(u0, dtype=np.float64)
        out = dict(converged=False, iterations=max_iter, residual=[], update=[], linear_iterations=[], r0=1.0, du0=1.0,
                   linear_failed=False)
        Jc = None
        for it in range(max_iter):
            R = self.residual(u)
            rn = np.linalg.norm(R)
            if it == 0:
                out["r0"] = max(1.0, rn)
            out["residual"].append(rn)
            if rn < abs_tol or rn / out["r0"] < rel_tol:
                out["converged"], out["iterations"] = True, it
                break
            if it % max(1, jacobian_rebuild_freq) == 0 or Jc is None:
                Jc = self.jacobian(u, eliminated=True)
            dx, its, ok = self.linear_solve(Jc, -R, linear, lin_rtol, lin_atol, lin_max_it)
            out["linear_iterations"].append(its)
            if not ok:
                out["linear_failed"], out["iterations"] = True, it
                break
            un = np.linalg.norm(dx)
            if it == 0:
                out["du0"] = max(1.0, un)
            out["update"].append(un)
            u += dx
        out["u"] = u
        return out


# ---- boundary load ------------------------------------------------------------------------------------
def facet_rule(dim, p):
    """BoundaryLFIntegrator's default rule, order p + 1 on the facet: segments Gauss-Legendre with
    (p + 1) // 2 + 1 points on [0, 1]; triangles MFEM's tabulated rule of order p + 1.  (points (nq, dim - 1), w)"""
    if dim == 2:
        x, w = np.polynomial.legendre.leggauss((p + 1) // 2 + 1)
        return (0.5 * (x + 1.0))[:, None], 0.5 * w
    return O.simplex_rule_order(2, p + 1)


def boundary_load(mesh, elem, local_face, g):
    """b_i = sum_facets sum_q w_q (edge length | |t1 x t2|) g(x_q) phi_i(x_q); facet f of an element is the one
    opposite local vertex f, g maps points (n, dim) to values (n).  The element's whole basis is evaluated at
    the facet's points (the functions of the other nodes vanish there), so no facet dof table is needed."""
    dim, p, verts, dofmap, nl = _space(mesh)
    s, w = facet_rule(dim, p)
    Vref = np.vstack([np.zeros(dim), np.eye(dim)])
    b = np.zeros(nl)
    for e, f in zip(elem, local_face):
        v = [a for a in range(dim + 1) if a != f]
        xr = Vref[v[0]] + s @ (Vref[v[1:]] - Vref[v[0]])
        Vp = verts[e][v]
        xp = Vp[0] + s @ (Vp[1:] - Vp[0])
        t = Vp[1:] - Vp[0]
        meas = np.linalg.norm(t[0]) if dim == 2 else np.linalg.norm(np.cross(t[0], t[1]))
        phi, _ = basis(dim, p, xr)
        np.add.at(b, dofmap[e], phi.T @ (w * meas * g(xp)))
    return b


def dof_coords(mesh):
    """Physical coordinates of the dofs (nl, dim), from the node set."""
    dim, p, verts, dofmap, nl = _space(mesh)
    X = nodes(dim, p)
    lam = np.hstack([1.0 - X.sum(axis=1, keepdims=True), X])  # barycentric coordinates of the nodes
    xyz = np.zeros((nl, dim))
    xyz[dofmap.ravel()] = np.einsum("la,eak->elk", lam, verts).reshape(-1, dim)
    return xyz


# ---- the two parameter sets ---------------------------------------------------------------------------------
def set_a(mesh):
    """Set A on [0, 1]^dim: coefficients, u_old, the flux on x = 0 and its facet predicate."""
    xyz = dof_coords(mesh)
    u_old = 1.0 + 0.5 * np.sin(np.pi * xyz[:, 0]) * np.cos(np.pi * xyz[:, 1])
    return dict(coeffs=dict(dt=0.1, a0=1.0, a1=0.5, m0=1.0, m1=0.5, u_ref=0.0), scale=1.0, u_old=u_old, flux=0.25,
                on_x0=lambda X: bool(np.all(np.abs(X[:, 0]) < 1e-12)))


def set_b(mesh):
    """Set B (Input/input_nonlinear_1d.yaml) on the unit mesh scaled to [0, 0.01]^dim."""
    return dict(coeffs=dict(dt=0.1, a0=10.0, a1=0.09, m0=4.0e6, m1=3.6e4, u_ref=300.0), scale=0.01,
                u_old=np.full(int(mesh.nl), 300.0), flux=7.5e5, on_x0=lambda X: bool(np.all(np.abs(X[:, 0]) < 1e-12)))


# ---- the meshes of the two test files (host-side generators of the binding; inputs, not code under test) ----
def _p3_space(vxyz, elem_v, mesh_p1):
    import cdfem
    e, f = cdfem.boundary_facets(mesh_p1)
    bv = np.array([np.delete(elem_v[a], b) for a, b in zip(e, f)], dtype=np.int32)
    return cdfem.simplex_space(vxyz, elem_v, bv, np.ones(len(bv), dtype=np.int32), 3)


def build_mesh(name):
    """tri1 / tri2: perturbed Kuhn triangles n = 6 (72 elements); tri3: P3 on the Kuhn n = 4 topology;
    tet1 / tet2: perturbed Kuhn tetrahedra n = 3 (162 elements); square3: P3 on the reference's unit square
    (tests/golden/reference_meshes.npz: 938 triangles, 4,295 dofs)."""
    import cdfem
    if name in ("tri1", "tri2"):
        return cdfem.kuhn_mesh(2, 6, int(name[-1]), perturb=0.2)
    if name in ("tet1", "tet2"):
        return cdfem.kuhn_mesh(3, 3, int(name[-1]), perturb=0.2)
    if name == "tri3":
        m = cdfem.kuhn_mesh(2, 4, 1, perturb=0.2)
        return _p3_space(m.dof_xyz, m.dofmap, m)
    if name == "square3":
        import reference_meshes as RM
        d = RM.load("square")
        ids = d["node_id"]
        lut = np.full(int(ids.max()) + 1, -1, dtype=np.int64)
        lut[np.sort(ids)] = np.arange(len(ids))            # vertices in increasing gmsh node id
        xyz = d["node_xyz"][np.argsort(ids)][:, :2]
        tri = d["elem_type"] == 2
        ev = lut[d["elem_nodes"][tri][:, :3]].astype(np.int32)
        v = xyz[ev]
        det = (v[:, 1, 0] - v[:, 0, 0]) * (v[:, 2, 1] - v[:, 0, 1]) - (v[:, 2, 0] - v[:, 0, 0]) * (v[:, 1, 1] - v[:, 0, 1])
        ev[det < 0] = ev[det < 0][:, [0, 2, 1]]
        m1 = cdfem.Mesh(2, 1, np.ascontiguousarray(xyz[ev]), ev, len(xyz), np.zeros(0, dtype=np.int32), xyz, simplex=True)
        return _p3_space(np.ascontiguousarray(xyz), ev, m1)
    raise ValueError(name)


def scaled(mesh, s):
    """The same space on the mesh scaled by s about the origin."""
    import copy
    m = copy.copy(mesh)
    m.verts = np.asarray(mesh.verts) * s
    if getattr(mesh, "dof_xyz", None) is not None:
        m.dof_xyz = mesh.dof_xyz * s
    return m


# Newton cases of both test files: (mesh, set) -> rel_tol, chosen so that no iterate of the restatement sits
# within a factor 3 of a stopping threshold without the decision being clear (test_nonlinear_ref.py checks it).
# Set A: iterate 3 has rn / r0 between 1.0e-9 and 9.2e-9 on these meshes, against the default 1e-8; 1e-7 is
# decisive (iterate 2 is at 1e-4).  Set B: iterate 3 is at 1e-7 .. 5e-6 and iterate 4 below 2e-12: the
# reference's 1e-8 is decisive.  abs_tol stays at the reference's 1e-10.
NEWTON_REL_TOL = {"A": 1e-7, "B": 1e-8}
NEWTON_ABS_TOL = 1e-10
THREE_STEP_REL_TOL = 1e-9  # three backward-Euler steps of set A (test_three_steps_restatement says why)
# Residual histories are compared where the restatement's norm exceeds 1e-6 r0.  Measured on the six cases of
# test_gpu_nonlinear.py's Newton test (P2 triangles, P3 unit square, P2 tetrahedra, sets A and B), restatement
# with a direct solve against restatement with the oracle's GMRES(30) at 1e-13 under Jacobi and under ILU(0):
# the largest relative spread of those norms is 5.5e-10 (P3 square, set B, ILU(0); the others 3e-13 .. 2.9e-10).
# The HIP path differs in summation order as well as in the linear solve: 100 times that spread.
HISTORY_SPREAD = 5.5e-10
HISTORY_TOL = 100.0 * HISTORY_SPREAD
SETS = {"A": set_a, "B": set_b}


def newton_problem(mesh_name, set_name, ess=()):
    """(mesh on the set's domain, HeatForm with u_old and the Neumann load, facets (elem, face), u0)."""
    import cdfem
    m0 = build_mesh(mesh_name)
    prm = SETS[set_name](m0)
    m = scaled(m0, prm["scale"])
    F = HeatForm(m, ess=ess, **prm["coeffs"])
    F.u_old = prm["u_old"].copy()
    e, f = cdfem.boundary_facets(m0, prm["on_x0"])
    flux = prm["flux"]
    F.g = boundary_load(m, e, f, lambda X: np.full(len(X), flux))
    return m, F, (e, f), prm
