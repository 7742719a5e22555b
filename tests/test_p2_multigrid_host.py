"""The CPU model of the P2 multigrid (tests/p2_multigrid_reference.py) and the host tables of
P2Multigrid, without a GPU: P, the Galerkin property P^T K2 P = K1 that lets the P1 hierarchy stand
below the P2 level without a triple product, the symmetry of the cycle, and the iteration counts
the GPU tests compare against."""

import numpy as np
import pytest

import p2_multigrid_reference as p2ref

_MODELS = {}


def _coarse(name):
    from pytorch_fem_solver_amd import meshgen

    return {"square4": lambda: meshgen.unit_square(4, 0.25, 1), "delaunay60": lambda: meshgen.delaunay_square(60, 7),
            "square8": lambda: meshgen.unit_square(8, 0.25, 3), "delaunay80": lambda: meshgen.delaunay_square(80, 7)}[name]()


def _model(name, levels, **kw):
    key = (name, levels, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = p2ref.P2Model(_coarse(name), levels, **kw)
    return _MODELS[key]


SMALL = ["square4", "delaunay60"]


@pytest.mark.parametrize("name", SMALL)
def test_prolongation_has_row_sums_one_and_matches_the_device_tables(name):
    from pytorch_fem_solver_amd.multigrid import transpose_edges

    model = _model(name, 1)
    P, n_v, n = model.P2, model.n_v, model.n
    assert P.shape == (n, n_v)
    assert (np.asarray(P.sum(axis=1)).reshape(-1) == 1.0).all()
    assert (P[:n_v].toarray() == np.eye(n_v)).all()
    # the table of the restriction kernel is P^T without the identity: 0.5 at (v, idx[p])
    edges = np.asarray(model.mesh["edges"])
    ptr, idx = transpose_edges(edges, n_v)
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and ptr.shape == (n_v + 1,) and idx.shape == (2 * (n - n_v),)
    rows = np.repeat(np.arange(n_v), np.diff(ptr))
    table = np.zeros((n_v, n))
    np.add.at(table, (rows, idx), 0.5)
    table[np.arange(n_v), np.arange(n_v)] += 1.0
    assert (table == P.T.toarray()).all()
    for v in range(n_v):
        row = idx[ptr[v]:ptr[v + 1]]
        assert (np.diff(row) > 0).all() and (row >= n_v).all()


@pytest.mark.parametrize("name", SMALL)
def test_p1_operator_is_the_galerkin_operator_of_the_p2_one(name):
    """Stiffness at order 3: P^T K2 P equals the model's K1 to 1e-13 of max|K1|."""
    model = _model(name, 1)
    defect = model.galerkin_defect()
    print(f"{name}: max|P^T K2 P - K1| / max|K1| = {defect:.2e}")
    assert defect <= 1e-13


@pytest.mark.parametrize("name", SMALL)
def test_model_cycle_is_symmetric(name):
    model = _model(name, 1)
    rng = np.random.default_rng(31)
    r1, r2 = rng.standard_normal(model.n), rng.standard_normal(model.n)
    z1, z2 = model.vcycle(r1), model.vcycle(r2)
    asym = abs(z1 @ r2 - r1 @ z2) / (np.linalg.norm(z1) * np.linalg.norm(r2))
    print(f"{name}: asymmetry of the cycle {asym:.2e}")
    assert asym <= 1e-12
    assert (z1[model.mask2 == 0] == 0).all()


#: (coarse mesh, refinements) -> (P2 DoFs, P2-multigrid PCG iterations, Jacobi CG iterations): V(2,2),
#: omega = 2/3, order 3, rtol 1e-10, masked standard-normal right-hand side of seed 2
PINNED = {
    ("square8", 0): (289, 11, 79), ("square8", 1): (1089, 13, 161), ("square8", 2): (4225, 14, 334),
    ("square8", 3): (16641, 16, 679),
    ("delaunay80", 0): (281, 16, 89), ("delaunay80", 1): (1049, 23, 187), ("delaunay80", 2): (4049, 35, 385),
    ("delaunay80", 3): (15905, 46, 754),
}


@pytest.mark.parametrize("name,levels", sorted(PINNED))
def test_model_iteration_counts(name, levels):
    model = _model(name, levels)
    b = p2ref.masked_rhs(model)
    _, it, res = model.pcg(b)
    _, it_jacobi, res_jacobi = model.jacobi_cg(b)
    assert res <= 1e-10 and res_jacobi <= 1e-10
    assert (model.n, it, it_jacobi) == PINNED[name, levels]


def test_model_iteration_counts_with_a_mass_term_and_no_dirichlet():
    model = _model("square8", 2, beta=1.0, dirichlet=False)
    b = p2ref.masked_rhs(model)
    assert (model.n, model.pcg(b)[1], model.jacobi_cg(b)[1]) == (4225, 14, 526)


def test_half_damping_on_the_p2_level_is_no_better():
    """omega = 0.5 on the P2 level alone costs iterations: the default stays 2/3."""
    b = p2ref.masked_rhs(_model("square8", 2))
    assert p2ref.P2Model(_coarse("square8"), 2, omega_top=0.5).pcg(b)[1] >= _model("square8", 2).pcg(b)[1] + 1
