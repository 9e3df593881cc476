"""numpy restatement of the boundary linear form on quad / hex faces (cdfem_bdr_* on tensor meshes).  Test code
only: what tests/test_gpu_bdr_tensor.py compares the HIP path with, pinned on its own by
tests/test_nonlinear_tensor_bdr_ref.py.  Written from the formula

    b_i = sum_facets sum_q w_q sigma_q g(x_q) phi_i(xi_q)

    the facet    local facet f = 2 axis + side of an element, side 0 at xi_axis = 0 and side 1 at xi_axis = 1, in
                 the lexicographic vertex / dof convention of nonlinear_tensor_ref (x fastest);
    its dofs     the element's local dofs whose axis index is 0 or p, the lower remaining axis fastest;
    the rule     BoundaryLFIntegrator's default order p + 1: numpy's Gauss-Legendre with n = (p + 1) // 2 + 1 points
                 on [0, 1] per remaining direction, the lower remaining axis fastest;
    sigma        |dx/ds| on an edge, |dx/ds x dx/dt| on a face, from the element's multilinear map at the point
                 (a perturbed hex face is bilinear: sigma varies over it).

The element's whole basis is not used: only the facet's dofs carry a function that does not vanish on the facet,
and tests/test_nonlinear_tensor_bdr_ref.py checks that list against the dofs' coordinates."""
import numpy as np

import nonlinear_ref as NR
import nonlinear_tensor_ref as T


def rule_points_1d(p):
    return (p + 1) // 2 + 1


def remaining(dim, axis):
    """the axes of the facet, ascending"""
    return [k for k in range(dim) if k != axis]


def facet_rule(dim, p, n=None):
    """(s (nq, dim - 1) on the reference facet, w (nq)): tensor Gauss-Legendre, first facet coordinate fastest"""
    n = rule_points_1d(p) if n is None else n
    x, w = T.gauss_01(n)
    if dim == 2:
        return x[:, None], w
    return np.stack([np.tile(x, n), np.repeat(x, n)], axis=1), np.outer(w, w).ravel()


def rule_size(dim, p):
    return rule_points_1d(p) ** (dim - 1)


def facet_dofs(dim, p, f):
    """local dofs of facet f = 2 axis + side, the lower remaining axis fastest"""
    axis, side = f // 2, f % 2
    d1 = p + 1
    out = []
    for l in range(d1 ** (dim - 1)):
        idx = [0] * dim
        idx[axis] = side * p
        for m, k in enumerate(remaining(dim, axis)):
            idx[k] = (l // d1 ** m) % d1
        out.append(sum(i * d1 ** k for k, i in enumerate(idx)))
    return np.array(out, dtype=np.int64)


def facet_reference_points(dim, f, s):
    """the facet points s (nq, dim - 1) in the element's reference coordinates (nq, dim)"""
    axis, side = f // 2, f % 2
    xi = np.zeros((len(s), dim))
    xi[:, axis] = float(side)
    for m, k in enumerate(remaining(dim, axis)):
        xi[:, k] = s[:, m]
    return xi


def facet_geometry(V, dim, f, s):
    """physical points (nq, dim) and sigma (nq) of facet f of the element with vertices V (2^dim, dim)"""
    xi = facet_reference_points(dim, f, s)
    N, dN = T.shape_q1(dim, xi)
    x = N @ V
    Jm = np.einsum("vk,qvm->qkm", V, dN)                      # J[k, m] = d x_k / d xi_m
    r = remaining(dim, f // 2)
    if dim == 2:
        return x, np.linalg.norm(Jm[:, :, r[0]], axis=1)
    return x, np.linalg.norm(np.cross(Jm[:, :, r[0]], Jm[:, :, r[1]]), axis=1)


def facet_basis(dim, p, s):
    """phi (nq, (p + 1)^(dim - 1)) of the facet's dofs at the facet points, the lower remaining axis fastest"""
    B0, _ = T.lagrange_1d(p, s[:, 0])
    if dim == 2:
        return B0.astype(np.float64)
    B1, _ = T.lagrange_1d(p, s[:, 1])
    return np.einsum("qb,qa->qba", B1, B0).reshape(len(s), -1).astype(np.float64)


def quadrature_points(mesh, elem, local_face):
    """(nbf, nq, dim) physical coordinates of the rule's points, facet-major"""
    dim, p, verts, _, _ = NR._space(mesh)
    s, _ = facet_rule(dim, p)
    return np.array([facet_geometry(verts[e], dim, f, s)[0] for e, f in zip(elem, local_face)]).reshape(len(elem), len(s), dim)


def boundary_load(mesh, elem, local_face, g, n=None):
    """b (nl) for g mapping points (nq, dim) to values (nq); n: points per direction instead of the rule's"""
    dim, p, verts, dofmap, nl = NR._space(mesh)
    s, w = facet_rule(dim, p, n)
    phi = facet_basis(dim, p, s)
    b = np.zeros(nl)
    for e, f in zip(elem, local_face):
        x, sigma = facet_geometry(verts[e], dim, f, s)
        np.add.at(b, dofmap[e][facet_dofs(dim, p, f)], phi.T @ (w * sigma * g(x)))
    return b


def plane_facets(mesh, axis, value, tol=1e-12):
    """(elem, local_face) int32 arrays of the facets whose vertices all have coordinate `axis` equal to value,
    in ascending (element, f) order (the perturbation of a box mesh leaves its boundary planes in place)"""
    dim, _, verts, _, _ = NR._space(mesh)
    elem, face = [], []
    for e in range(len(verts)):
        for f in range(2 * dim):
            vs = [v for v in range(1 << dim) if ((v >> (f // 2)) & 1) == f % 2]
            if np.all(np.abs(verts[e][vs, axis] - value) <= tol):
                elem.append(e)
                face.append(f)
    return np.array(elem, dtype=np.int32), np.array(face, dtype=np.int32)
