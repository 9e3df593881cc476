"""Pins tests/nonlinear_tensor_bdr_ref.py, the numpy restatement of the boundary linear form on quad / hex
faces, before tests/test_gpu_bdr_tensor.py compares the HIP path with it.  No GPU.  Every test prints the figures
it asserts.

Tolerances: 1e-14 relative for the sums that are exact up to rounding (a facet sum has at most 9 points and 9
dofs, a boundary at most 20 facets: a few hundred roundings of 1.1e-16 with random signs stay below 1e-14)."""
import numpy as np
import pytest

import cdfem
import nonlinear_tensor_bdr_ref as B
import nonlinear_tensor_ref as T

QUADS = ["quad1", "quad2", "quad3"]
HEXES = ["hex1", "hex2", "hex2L"]


def all_boundary(mesh):
    """every facet of the unit box's boundary, plane by plane"""
    e, f = zip(*[B.plane_facets(mesh, axis, value) for axis in range(mesh.dim) for value in (0.0, 1.0)])
    return np.concatenate(e), np.concatenate(f)


def test_rule_sizes():
    """n = (p + 1) // 2 + 1 per direction: 2, 2, 3 for p = 1, 2, 3; weights sum to 1 on the reference facet"""
    assert [B.rule_points_1d(p) for p in (1, 2, 3)] == [2, 2, 3]
    assert [B.rule_size(2, p) for p in (1, 2, 3)] == [2, 2, 3] and [B.rule_size(3, p) for p in (1, 2)] == [4, 4]
    for dim, p in [(2, 1), (2, 3), (3, 1), (3, 2)]:
        s, w = B.facet_rule(dim, p)
        assert s.shape == (B.rule_size(dim, p), dim - 1) and abs(w.sum() - 1.0) <= 1e-15
    s, _ = B.facet_rule(3, 2)
    assert s[0, 0] < s[1, 0] and s[0, 1] == s[1, 1]  # the first facet coordinate is the fastest


@pytest.mark.parametrize("name", QUADS + HEXES)
def test_measure_of_the_boundary(name):
    """g = 1: sum_i b_i is the boundary's measure, 4 for the square (any quad mesh: its edges are straight, the
    perturbed ones included) and 6 for the unperturbed cube; one plane alone gives 1"""
    perturb = 0.2 if name in QUADS else 0.0
    m = T.build_mesh(name, perturb)
    e, f = all_boundary(m)
    one = lambda x: np.ones(len(x))
    total = B.boundary_load(m, e, f, one).sum()
    e0, f0 = B.plane_facets(m, 0, 0.0)
    assert len(e0) > 0 and np.all(f0 == 0)
    side = B.boundary_load(m, e0, f0, one).sum()
    print(f"{name}: boundary {total:.17g}, x = 0 {side:.17g}")
    assert abs(total - 2.0 * m.dim) <= 1e-14 * 2.0 * m.dim and abs(side - 1.0) <= 1e-14
    if name in HEXES:  # on the perturbed cube the boundary planes stay in place: still 6
        mp = T.build_mesh(name, 0.2)
        ep, fp = all_boundary(mp)
        assert abs(B.boundary_load(mp, ep, fp, one).sum() - 6.0) <= 1e-13


@pytest.mark.parametrize("name", QUADS + HEXES)
def test_rule_is_exact_for_linear_data(name):
    """constant and linear g on the unperturbed box: phi_i g has degree <= p + 1 <= 2n - 1 per direction, so the
    rule and the one with twice the points per direction are both exact and agree to rounding"""
    m = T.build_mesh(name, 0.0)
    e, f = all_boundary(m)
    n = B.rule_points_1d(m.order)
    for label, g in (("constant", lambda x: np.full(len(x), 0.25)), ("linear", lambda x: 1.0 + 2.0 * x[:, 1] - 0.5 * x[:, -1])):
        b, b2 = B.boundary_load(m, e, f, g), B.boundary_load(m, e, f, g, n=2 * n)
        d = np.abs(b - b2).max() / np.abs(b2).max()
        print(f"{name} {label}: {d:.2e}")
        assert d <= 1e-14
    # and a rule with one point fewer is not exact where p + 1 > 2 (n - 1) - 1: the count is the one in use
    if m.order + 1 > 2 * (n - 1) - 1:
        g = lambda x: 1.0 + 2.0 * x[:, 1] - 0.5 * x[:, -1]
        assert np.abs(B.boundary_load(m, e, f, g, n=n - 1) - B.boundary_load(m, e, f, g)).max() > 1e-6


@pytest.mark.parametrize("name", QUADS + HEXES)
def test_facet_dofs_lie_on_the_face(name):
    """facet f = 2 axis + side: its dof list is exactly the element's dofs whose coordinate lies on the face, the
    lower remaining axis fastest; checked on the reference lattice for all 2 dim facets and in physical
    coordinates on the planes of the box"""
    m = T.build_mesh(name, 0.2)
    dim, p = m.dim, m.order
    g = np.asarray(T.O.gll_nodes(p), dtype=np.float64)
    d1 = p + 1
    lat = np.array([[g[(l // d1 ** k) % d1] for k in range(dim)] for l in range(d1 ** dim)])  # local dof -> xi
    for f in range(2 * dim):
        axis, side = f // 2, f % 2
        fd = B.facet_dofs(dim, p, f)
        assert len(fd) == d1 ** (dim - 1)
        assert sorted(fd) == [l for l in range(d1 ** dim) if lat[l, axis] == float(side)]
        r = B.remaining(dim, axis)
        key = [tuple(lat[l, k] for k in reversed(r)) for l in fd]
        assert key == sorted(key)  # ascending with the lower remaining axis fastest
    xyz = T.dof_coords(m)
    for axis in range(dim):
        for value in (0.0, 1.0):
            e, f = B.plane_facets(m, axis, value)
            assert len(e) > 0 and np.all(f == 2 * axis + int(value))
            on = set(np.nonzero(np.abs(xyz[:, axis] - value) <= 1e-12)[0])
            hit = set()
            for ee, ff in zip(e, f):
                d = m.dofmap[ee][B.facet_dofs(dim, p, ff)]
                assert set(d) == on & set(m.dofmap[ee])
                hit |= set(d)
            assert hit == on


def test_points_and_sigma_on_a_bilinear_face():
    """a hex with one lifted vertex: the points lie on the mapped face, and sigma integrates to the face's area
    computed by a fine rule; on the unperturbed face sigma is the constant area"""
    V = np.array([[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)], dtype=np.float64)
    s, w = B.facet_rule(3, 2)
    x, sigma = B.facet_geometry(V, 3, 5, s)                     # z = 1
    assert np.abs(x[:, 2] - 1.0).max() == 0.0 and np.abs(sigma - 1.0).max() <= 1e-15
    assert np.abs(x[:, :2] - s).max() <= 1e-16                  # s -> x, t -> y: the lower remaining axis fastest
    V2 = V.copy()
    V2[7, 2] = 1.5                                              # the face z = 1 becomes bilinear
    _, sig = B.facet_geometry(V2, 3, 5, s)
    sf, wf = B.facet_rule(3, 2, n=12)
    area = wf @ B.facet_geometry(V2, 3, 5, sf)[1]
    exact = wf @ np.sqrt(1.0 + 0.25 * sf[:, 0] ** 2 + 0.25 * sf[:, 1] ** 2)   # z = 1 + s t / 2
    print(f"area {area:.15f} (closed form under the same rule {exact:.15f}), 2 x 2 rule {w @ sig:.15f}")
    assert abs(area - exact) <= 1e-15 and sig.max() - sig.min() > 1e-2 and abs(w @ sig - area) <= 1e-3
    assert cdfem.box_mesh(3, 1, 1).verts.shape == (1, 8, 3)     # the vertex convention above is box_mesh's
    assert np.array_equal(cdfem.box_mesh(3, 1, 1).verts[0], V)
