"""The long-double operator reference (tests/operator_reference.py) and the shared random-mesh
generator (tests/random_meshes.py), checked without a GPU: the generator still names the same mesh
per seed as it did inside tests/test_hip_fuzz.py; the float64 oracle and the numpy walk of the
ring plan (tests/test_operator_plan.py: the fan formula of the apply kernels) agree with the
reference within 1e-12, row-scaled, on seeds of the operator sweep; rows of isolated vertices are
exactly zero."""

import hashlib

import numpy as np
import pytest

import operator_reference as oref
from random_meshes import has_elements, random_mesh
from test_operator_plan import apply_ring_plan

TOL = 1e-12

#: sha256 of verts.tobytes() + tris.tobytes() per rng seed, recorded with the generator as it stood
#: in tests/test_hip_fuzz.py before it moved (1000 + seed: the assembly sweep, 5000 + seed: the
#: operator sweep)
MESH_HASHES = {
    1000: "a15f3a00db7f2d8689cf061c4329c6b33532e9e186b21050d1d15ec2e2d5ecbc",  # 3279 vertices, 6166 elements
    1003: "abb1cb554fea0225b3b3ed39e0171dd8f58fae80cbc831fa4b09e97344dac23c",  # 361 vertices, 648 elements
    1017: "8082b7e9c47322e28599643a5e923c2a70705dcfe4a82a29c198a4de0bb85525",  # 2946 vertices, 5674 elements
    1042: "e79a6eb4959303d3a2d542f72296b8ff01ab0f057028add94842326c06d91df2",  # 100 vertices, 144 elements
    1099: "2076728f7a3a202a2cb3277175bb4ff12cc6d93dbfe9cbcce967f6c22fe0afc3",  # 33306 vertices, 65882 elements
    5000: "9f484622d4808ca165785c8a7b809527b720c7980cfa7338b5c32b90e0238e91",  # 14641 vertices, 22043 elements
    5004: "6c2c90b1679de30fbd98ee1c08221a960e8ec1c98cea55b60c968f5f9e17dad4",  # 6889 vertices, 9566 elements
    5021: "ead974fb9581afa88992782701ec501c3e44a9c46b1277bdd7e98b5c2ee6c101",  # 3154 vertices, 6082 elements
    5063: "e53ce77b8bc74dc50909ab56e10408949507b8add9aaafc9b34592a22cc5cb36",  # 361 vertices, 648 elements
}


@pytest.mark.parametrize("rng_seed", sorted(MESH_HASHES))
def test_a_seed_still_names_the_same_mesh(rng_seed):
    verts, tris = random_mesh(np.random.default_rng(rng_seed))
    assert verts.dtype == np.float64 and tris.dtype == np.int32
    assert hashlib.sha256(verts.tobytes() + tris.tobytes()).hexdigest() == MESH_HASHES[rng_seed]


#: a dozen seeds of the operator sweep: with and without isolated vertices, structured and Delaunay,
#: renumbered (seed % 3 == 2) and with long rows, float32 coordinates among them
SEEDS = (2, 6, 7, 9, 13, 25, 27, 31, 44, 50, 55, 84, 96, 98)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_and_plan_walk_agree_with_the_long_double_reference(seed):
    case = oref.sweep_case(seed)
    verts, tris = case["verts"], case["tris"]
    order, alpha, beta = case["order"], case["alpha"], case["beta"]
    n = verts.shape[0]
    ref = oref.OperatorReference(verts, tris, order, alpha, beta)
    assert ref.values.dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63
    u = case["u"].astype(np.float64)
    want, scale = ref.apply(u)
    want_d, scale_d = ref.diagonal()
    # the float64 oracle
    low = oref.OperatorReference(verts, tris, order, alpha, beta, dtype=np.float64)
    assert low.values.dtype == np.float64
    e_values = oref.row_error(low.values, ref.values, scale_d[ref.rows])
    e_apply = oref.row_error(low.apply(u)[0], want, scale)
    e_diag = oref.row_error(low.diagonal()[0], want_d, scale_d)
    print(f"seed {seed}: n = {n}, oracle in float64: values {e_values:.2e}, K u {e_apply:.2e}, diag K {e_diag:.2e}")
    assert max(e_values, e_apply, e_diag) <= TOL
    # the fan formula of the apply kernels, walked over the plan the engine would build
    plan, pverts, _ = oref.plan_of(case)
    assert plan is not None
    w, md, mo = oref.fan_weights(order)
    perm = np.arange(n)
    if case["renumber"]:
        import torch

        from pytorch_fem_solver_amd.basis.engine import _morton_permutation

        perm = _morton_permutation(torch.tensor(verts)).numpy()
    y = np.empty(n)
    y[perm] = apply_ring_plan(plan, pverts, u[perm], alpha * w, beta * md, beta * mo)
    d = np.empty(n)
    d[perm] = apply_ring_plan(plan, pverts, None, alpha * w, beta * md, beta * mo)
    assert not np.isnan(y).any() and not np.isnan(d).any(), "every row written"
    e_walk, e_walk_d = oref.row_error(y, want, scale), oref.row_error(d, want_d, scale_d)
    print(f"seed {seed}: plan walk ({plan['slots']} slots, {plan['long_rows'].size // 24} long rows): "
          f"K u {e_walk:.2e}, diag K {e_walk_d:.2e}")
    assert max(e_walk, e_walk_d) <= TOL
    # vertices without elements
    lone = ~has_elements(tris, n)
    assert int(lone.sum()) == case["isolated"]
    for vec in (want, scale, want_d, scale_d, y, d):
        assert (vec[lone] == 0).all()
    assert (np.diff(ref.rowptr)[lone] == 0).all()


def test_the_chosen_seeds_cover_isolated_vertices_and_both_record_widths():
    cases = [oref.sweep_case(seed) for seed in SEEDS]
    assert len(SEEDS) >= 12
    assert sum(c["isolated"] > 0 for c in cases) >= 4 and sum(c["isolated"] == 0 for c in cases) >= 4
    slots = [oref.plan_of(c)[0]["slots"] for c in cases]
    assert slots.count(7) >= 3 and slots.count(15) >= 3
    assert any(c["long_rows"] and oref.plan_of(c)[0]["long_rows"].size for c in cases)
    assert any(c["renumber"] for c in cases) and any(c["single"] for c in cases)


def test_reference_on_a_hand_made_mesh():
    """Two open fans at vertex 0, vertex 5 without elements; the stiffness rows sum to zero and the
    mass matrix sums to the area, to long-double rounding."""
    verts = np.array([[0, 0], [1, 0], [1, 1], [-1, 0], [-1, -1], [5, 5], [0.3, 1.2]], dtype=np.float64)
    tris = np.array([[0, 1, 2], [0, 3, 4], [2, 6, 0]], dtype=np.int32)
    stiff = oref.OperatorReference(verts, tris, 3, 1.0, 0.0)
    sums, scale = stiff.apply(np.ones(7))
    assert float(np.abs(sums).max()) <= 8 * np.finfo(np.longdouble).eps * float(scale.max())
    mass = oref.OperatorReference(verts, tris, 3, 0.0, 1.0)
    area = 0.5 * np.abs(oref.signed_area2(verts, tris)).sum()
    assert abs(float(mass.values.sum()) - area) <= 1e-15 * area
    for ref in (stiff, mass):
        assert ref.apply(np.ones(7))[0][5] == 0 and ref.diagonal()[0][5] == 0 and ref.diagonal()[1][5] == 0
        assert np.array_equal(ref.dense(), ref.dense().T) or np.abs(ref.dense() - ref.dense().T).max() <= 1e-18
