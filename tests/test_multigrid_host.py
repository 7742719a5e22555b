"""meshgen.refine_uniform and the CPU model of the multigrid cycle (tests/multigrid_reference.py),
on a machine without a GPU: the invariants of the red refinement, the prolongation that its parent
table gives, the symmetry of the model's cycle and the iteration counts that pin the model."""

import numpy as np
import pytest

from conftest import load_golden, mesh_from_golden

import multigrid_reference as mgref


def _flipped():
    from pytorch_fem_solver_amd import meshgen

    mesh = meshgen.unit_square(6, 0.25, 4)
    tri = mesh["triangles"].copy()
    flip = np.random.default_rng(5).random(tri.shape[0]) < 0.4
    tri[flip] = tri[flip][:, [0, 2, 1]]
    nb = mesh["neighbors"].copy()
    nb[flip] = nb[flip][:, [0, 2, 1]]
    mesh["triangles"], mesh["neighbors"] = tri, nb
    return mesh


def _mesh(name):
    from pytorch_fem_solver_amd import meshgen

    if name == "structured":
        return meshgen.unit_square(4, 0.25, 1)
    if name == "clockwise":
        return mesh_from_golden(load_golden("p1_square_n5_clockwise.npz"))
    if name == "flipped":
        return _flipped()
    if name == "delaunay":
        return meshgen.delaunay_square(60, 7)
    raise KeyError(name)


MESHES = ["structured", "clockwise", "flipped", "delaunay"]


def _det(mesh):
    p = np.asarray(mesh["vertices"], dtype=np.float64)[np.asarray(mesh["triangles"]).astype(np.int64)]
    return (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])


def _edge_keys(pairs, n):
    pairs = np.asarray(pairs).astype(np.int64)
    return pairs.min(axis=1) * n + pairs.max(axis=1)


@pytest.mark.parametrize("name", MESHES)
def test_refine_uniform_invariants(name):
    from pytorch_fem_solver_amd import meshgen

    coarse = _mesh(name)
    fine, parents = meshgen.refine_uniform(coarse)
    V, E, T = coarse["vertices"].shape[0], coarse["edges"].shape[0], coarse["triangles"].shape[0]
    Vf = fine["vertices"].shape[0]
    assert Vf == V + E
    assert fine["triangles"].shape == (4 * T, 3) and fine["triangles"].dtype == np.int32
    assert fine["edges"].shape == (2 * E + 3 * T, 2) and fine["edge_markers"].shape == (2 * E + 3 * T, 1)
    assert fine["vertex_markers"].shape == (Vf, 1) and fine["neighbors"].shape == (4 * T, 3)
    assert parents.shape == (Vf, 2) and parents.dtype == np.int32
    assert parents.min() >= 0 and parents.max() < V

    # the area, and the orientation of every child
    det_c, det_f = _det(coarse), _det(fine)
    assert abs(np.abs(det_f).sum() - np.abs(det_c).sum()) <= 1e-14 * np.abs(det_c).sum()
    assert (np.sign(det_f.reshape(T, 4)) == np.sign(det_c)[:, None]).all()
    assert np.abs(det_f.reshape(T, 4) - det_c[:, None] / 4).max() <= 1e-14 * np.abs(det_c).max()

    # the numbering is the Morton order of the fine vertices
    assert (meshgen.morton_order(fine["vertices"]) == np.arange(Vf)).all()

    # vertices: a kept vertex sits where its parent sits with its marker, a midpoint between the
    # endpoints of its edge with the edge's marker
    xc, xf = np.asarray(coarse["vertices"]), np.asarray(fine["vertices"])
    kept = parents[:, 0] == parents[:, 1]
    assert kept.sum() == V and sorted(parents[kept, 0]) == list(range(V))
    assert (xf[kept] == xc[parents[kept, 0]]).all()
    assert (xf[~kept] == 0.5 * (xc[parents[~kept, 0]] + xc[parents[~kept, 1]])).all()
    assert (fine["vertex_markers"][kept, 0] == np.asarray(coarse["vertex_markers"]).reshape(-1)[parents[kept, 0]]).all()
    coarse_keys = _edge_keys(coarse["edges"], V)
    order = np.argsort(coarse_keys)
    pos = order[np.searchsorted(coarse_keys[order], _edge_keys(parents[~kept], V))]
    assert (coarse_keys[pos] == _edge_keys(parents[~kept], V)).all(), "a midpoint's parents are a coarse edge"
    assert sorted(pos) == list(range(E)), "one midpoint per coarse edge"
    assert (fine["vertex_markers"][~kept, 0] == np.asarray(coarse["edge_markers"]).reshape(-1)[pos]).all()

    # edges: exactly the sides of the fine triangles, each once; the halves of a coarse edge carry
    # its marker, the edges inside a coarse triangle 0
    fine_keys = _edge_keys(fine["edges"], Vf)
    tri = np.asarray(fine["triangles"]).astype(np.int64)
    sides = np.concatenate([tri[:, [1, 2]], tri[:, [2, 0]], tri[:, [0, 1]]])
    assert len(set(fine_keys)) == fine_keys.size
    assert set(fine_keys) == set(_edge_keys(sides, Vf))
    midpoint_edge = np.full(Vf, -1)
    midpoint_edge[~kept] = pos
    a, b = fine["edges"][:, 0], fine["edges"][:, 1]
    half = kept[a] != kept[b]  # a kept vertex and a midpoint: half of a coarse edge
    assert half.sum() == 2 * E and (~kept[a] & ~kept[b]).sum() == 3 * T
    mid = np.where(kept[a], b, a)
    want = np.where(half, np.asarray(coarse["edge_markers"]).reshape(-1)[midpoint_edge[mid]], 0)
    assert (fine["edge_markers"].reshape(-1) == want).all()

    # neighbors: entry k is the triangle that shares the side opposite corner k, -1 on a side that
    # only one triangle has
    nb = fine["neighbors"]
    counts = dict(zip(*np.unique(_edge_keys(sides, Vf), return_counts=True)))
    for k in range(3):
        side = _edge_keys(tri[:, [(k + 1) % 3, (k + 2) % 3]], Vf)
        alone = np.array([counts[s] == 1 for s in side])
        assert ((nb[:, k] == -1) == alone).all()
        has = np.flatnonzero(~alone)
        other = tri[nb[has, k]]
        assert (nb[has, k] != has).all()
        shared = [(set(other[i]) & set(tri[t])) == set(tri[t, [(k + 1) % 3, (k + 2) % 3]]) for i, t in enumerate(has)]
        assert all(shared)


@pytest.mark.parametrize("name", MESHES)
def test_fine_mesh_builds_and_refines_again(name):
    import torch

    from pytorch_fem_solver_amd import MeshTri, meshgen

    fine, _ = meshgen.refine_uniform(_mesh(name))
    torch.set_default_dtype(torch.float64)
    try:
        mesh = MeshTri(triangulation=fine)
        assert tuple(mesh["cells", "vertices"].shape) == fine["triangles"].shape
        assert tuple(mesh["vertices", "coordinates"].shape) == fine["vertices"].shape
    finally:
        torch.set_default_dtype(torch.float32)
    finer, parents = meshgen.refine_uniform(fine)
    assert finer["vertices"].shape[0] == fine["vertices"].shape[0] + fine["edges"].shape[0]
    assert parents.max() < fine["vertices"].shape[0]


@pytest.mark.parametrize("name", MESHES)
def test_prolongation_reproduces_linear_functions(name):
    from pytorch_fem_solver_amd import meshgen
    from pytorch_fem_solver_amd.multigrid import transpose_parents

    coarse = _mesh(name)
    fine, parents = meshgen.refine_uniform(coarse)
    xc, xf = np.asarray(coarse["vertices"]), np.asarray(fine["vertices"])
    P = mgref.prolongation(parents, xc.shape[0])
    a, b, c = 0.7, -1.3, 2.1
    scale = abs(a) + abs(b) * np.abs(xc[:, 0]).max() + abs(c) * np.abs(xc[:, 1]).max()
    got = P @ (a + b * xc[:, 0] + c * xc[:, 1])
    assert np.abs(got - (a + b * xf[:, 0] + c * xf[:, 1])).max() <= 4 * np.finfo(np.float64).eps * scale
    assert np.abs(P.sum(axis=1) - 1).max() == 0

    # the transposed table of the kernels is P^T: every entry 0.5, a kept vertex listed twice
    ptr, idx = transpose_parents(parents, xc.shape[0])
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and ptr[-1] == 2 * xf.shape[0]
    rows = np.repeat(np.arange(xc.shape[0]), np.diff(ptr))
    import scipy.sparse as sp

    PT = sp.coo_matrix((np.full(idx.shape[0], 0.5), (rows, idx)), shape=(xc.shape[0], xf.shape[0])).tocsr()
    assert abs(PT - P.T).max() == 0
    for v in range(xc.shape[0]):
        assert (np.diff(idx[ptr[v]:ptr[v + 1]]) >= 0).all()
    assert np.diff(ptr).max() <= 17


@pytest.mark.parametrize("name,dirichlet,beta", [("structured", True, 0.0), ("clockwise", True, 0.0),
                                                  ("delaunay", True, 0.0), ("structured", False, 1.0)])
def test_model_cycle_is_symmetric(name, dirichlet, beta):
    model = mgref.Model(_mesh(name), 2, order=2, alpha=1.0, beta=beta, dirichlet=dirichlet)
    rng = np.random.default_rng(3)
    n = model.K[-1].shape[0]
    r1, r2 = rng.standard_normal(n), rng.standard_normal(n)
    z1, z2 = model.vcycle(r1), model.vcycle(r2)
    assert abs(z1 @ r2 - r1 @ z2) <= 1e-12 * np.linalg.norm(z1) * np.linalg.norm(r2)
    assert (z1[model.mask[-1] == 0] == 0).all()
    if name != "clockwise":  # positive definite where every triangle is stored counter-clockwise
        assert z1 @ r1 > 0


def test_model_iteration_counts():
    """V(2,2)-PCG on unit_square(8, 0.25, 3), stiffness, order 2, Dirichlet, rtol 1e-10, masked
    standard-normal right-hand side of seed 2: 11, 12, 13 iterations at levels 1, 2, 3 -- and the
    solution is the one a direct solve gives."""
    from pytorch_fem_solver_amd import meshgen

    import scipy.sparse.linalg

    counts = []
    for levels in (1, 2, 3):
        model = mgref.Model(meshgen.unit_square(8, 0.25, 3), levels)
        b = mgref.masked_rhs(model)
        x, it, res = model.pcg(b)
        assert res <= 1e-10
        counts.append(it)
        free = np.flatnonzero(model.mask[-1])
        direct = np.zeros_like(x)
        direct[free] = scipy.sparse.linalg.spsolve(model.K[-1][free][:, free].tocsc(), b[free])
        assert np.abs(x - direct).max() <= 1e-9 * np.abs(direct).max()
    assert counts == [11, 12, 13]
    assert model.K[-1].shape[0] == 65 * 65
