"""The long-double P2 operator reference and the cases of the P2 operator sweep
(tests/p2_operator_reference.py), checked without a GPU: the reference in float64 is the oracle
the golden fixture pins; long double and float64 agree to 1e-13; a seed still names the same case;
the numpy walk of the P2 row plan (tests/p2rows_emulator.py, k_p2_rows) covers every CSR entry once
and reproduces the reference on the sweep's meshes -- holes, several fans per vertex, isolated
vertices, renumbered edge DoFs -- where the host tests walk full meshes only; the operator CG is
handed is positive definite; and the sweep's checker rejects what it is there to reject."""

import hashlib

import numpy as np
import pytest

import p2_operator_reference as p2ref
from conftest import load_golden, mesh_from_golden, scaled_error
from oracle import assembly_oracle as orc
from p2rows_emulator import run_p2_plan

N_SEEDS = 100
#: the plan walk is a Python loop over the rows: the seeds up to this many DoFs
WALK_MAX_DOFS = 3000


@pytest.fixture(scope="module")
def cases():
    """seed -> case, drawn once for the module."""
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = p2ref.sweep_case(seed)
        return made[seed]

    return get


@pytest.mark.parametrize("order", [2, 4])
def test_float64_reference_is_the_oracle_of_the_golden_fixture(order):
    from pytorch_fem_solver_amd import dofs

    d = load_golden("p2_global_n4.npz")
    mesh = mesh_from_golden(d)
    conn6, xy, _ = dofs.p2_dofs_numpy(mesh["vertices"], mesh["triangles"], mesh["edges"], mesh["edge_markers"],
                                      mesh["vertex_markers"])
    assert np.array_equal(conn6, d["in_p2_connectivity"])
    n = xy.shape[0]
    for (alpha, beta), name in (((1.0, 0.0), "K_stiffness"), ((1.0, 1.0), "K_stiffness_mass")):
        ref = p2ref.P2OperatorReference(mesh["vertices"], mesh["triangles"], conn6, n, order, alpha, beta, np.float64)
        assert ref.values.dtype == np.float64
        assert scaled_error(ref.dense(), d[f"out_q{order}_{name}"]) <= 1e-14
        # ... and the oracle's own CSR assembly, bit for bit
        geo = orc.geometry(mesh["vertices"][mesh["triangles"].astype(np.int64)], 2, order)
        local = orc.integrate_local(alpha * orc.integrand_stiffness(geo) + beta * orc.integrand_mass(geo), geo["dx"])
        rowptr, colind, slots = orc.csr_pattern(conn6, n)
        assert np.array_equal(ref.rowptr, rowptr) and np.array_equal(ref.colind, colind)
        assert scaled_error(ref.values, orc.assemble_csr_values(local, slots, colind.shape[0])) <= 1e-14


#: seeds of the sweep: pure stiffness, pure mass and both; every order; clockwise elements (4, 7, 8);
#: isolated vertices (2, 7, 16, 33); float32-rounded coordinates (16)
CLOSE_SEEDS = (2, 4, 7, 8, 16, 20, 33)


@pytest.mark.parametrize("seed", CLOSE_SEEDS)
def test_long_double_and_float64_agree_row_by_row(seed, cases):
    case = cases(seed)
    ref, low = p2ref.reference_of(case), p2ref.reference_of(case, np.float64)
    assert ref.values.dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63
    assert low.values.dtype == np.float64
    want, scale = ref.apply(case["u"])
    want_d, scale_d = ref.diagonal()
    e_values = p2ref.row_error(low.values, ref.values, scale_d[ref.rows])
    e_apply = p2ref.row_error(low.apply(case["u"])[0], want, scale)
    e_diag = p2ref.row_error(low.diagonal()[0], want_d, scale_d)
    print(f"seed {seed}: n = {ref.n}, float64 against long double: values {e_values:.2e}, K u {e_apply:.2e}, "
          f"diag K {e_diag:.2e}")
    assert max(e_values, e_apply, e_diag) < 1e-13
    lone = case["lone"]
    for vec in (want, scale, want_d, scale_d):
        assert (vec[lone] == 0).all()
    assert (np.diff(ref.rowptr)[lone] == 0).all() and int(lone.sum()) == case["isolated"]


#: sha256 over (verts, tris, order, k) of a case: the generator, the order of the draws and the edit
CASE_HASHES = {
    0: "e093e2403f06422fcee3e72d7081c9cfa57b368f2204c0671f83c146cc662884",  # 25 DoFs, float32, order 4, k = 6
    7: "1361456a26e7d80087cb8842703f456c49f39d37eba9e59bd74bd51f89c35893",  # 6584 DoFs, order 2, k = 3, 2 isolated vertices
    16: "6304117ea64f65a679c8f336705bda2b6e1a3b1aed96e5ec45f0f3fb16ddcc2a",  # 2398 DoFs, float32, order 3, k = 4
    45: "017f483311f5229202ccea66d4e493caafd99579171fbf997829d59fd701db2b",  # 2222 DoFs, order 4, k = 2, 3 isolated vertices
    82: "6c9f683e25db6502289d22c409f21e32d47b3e3f40cb89da454ab1eef9f0301c",  # 134467 DoFs, float32, order 4, k = 5
}


def case_hash(case):
    tail = np.array([case["order"], case["k"]], dtype=np.int64)
    return hashlib.sha256(case["verts"].tobytes() + case["tris"].tobytes() + tail.tobytes()).hexdigest()


@pytest.mark.parametrize("seed", sorted(CASE_HASHES))
def test_a_seed_still_names_the_same_case(seed, cases):
    case = cases(seed)
    assert case["tris"].dtype == np.int32 and case["verts"].dtype == (np.float32 if case["single"] else np.float64)
    assert case["u"].shape == (case["n_dofs"],) and case["U"].shape == (case["n_dofs"], case["k"])
    assert case_hash(case) == CASE_HASHES[seed]


def test_the_mesh_dictionary_is_the_case():
    """The dictionary the public API takes: the DoFs Basis derives from it are conn6."""
    from pytorch_fem_solver_amd import dofs

    case = p2ref.sweep_case(7)
    mesh = case["mesh"]
    conn6, xy, _ = dofs.p2_dofs_numpy(mesh["vertices"], mesh["triangles"], mesh["edges"], mesh["edge_markers"],
                                      mesh["vertex_markers"])
    assert np.array_equal(conn6, case["conn6"]) and np.array_equal(xy, case["xy"])
    assert conn6[:, 3:].min() == case["n_verts"] and conn6.max() == case["n_dofs"] - 1
    assert case["isolated"] > 0 and not np.isin(np.flatnonzero(case["lone"]), conn6).any()


WALKED = {}


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_plan_walk_covers_every_entry_once_and_matches_the_reference(seed, cases):
    case = cases(seed)
    if case["n_dofs"] > WALK_MAX_DOFS:
        return
    plan, conn6, perm, rowptr = p2ref.plan_of(case)
    if isinstance(plan, str):
        assert "tile capacity" in plan or "locality" in plan or "15 neighbours" in plan, plan
        return
    assert (perm is not None) == case["renumber"]
    coords = np.asarray(case["verts"], dtype=np.float64)
    order, alpha, beta = case["order"], case["alpha"], case["beta"]
    ref = p2ref.reference_of(case, conn6=conn6)  # in the engine's numbering, as the plan
    assert np.array_equal(ref.rowptr, rowptr)
    vals, writes = run_p2_plan(plan, coords, rowptr, case["n_verts"], order, alpha, beta)
    assert (writes == 1).all() and not np.isnan(vals).any()
    scale_d = ref.diagonal()[1]
    e_values = p2ref.row_error(vals, ref.values, scale_d[ref.rows])
    # K u from the walked values, in the plan's numbering
    u = case["u"].astype(np.float64)
    prod = vals * u[ref.colind]
    y = np.zeros(ref.n)
    np.add.at(y, ref.rows, prod)
    want, scale = ref.apply(u)
    e_apply = p2ref.row_error(y, want, scale)
    facts = p2ref.plan_facts(plan)
    print(f"seed {seed}: n = {ref.n}, {facts}, isolated {case['isolated']}, renumbered {case['renumber']}: "
          f"values {e_values:.2e}, K u {e_apply:.2e}")
    assert e_values <= 1e-13 and e_apply <= 1e-13
    lone = case["lone"] if perm is None else case["lone"][perm]
    assert (y[lone] == 0).all() and (np.diff(rowptr)[lone] == 0).all()
    WALKED[seed] = {**facts, "isolated": case["isolated"], "renumbered": case["renumber"],
                    "holes": int(np.sum(np.diff(rowptr)[case["n_verts"]:] == 6))}


def test_the_walked_seeds_reach_the_cases_the_host_tests_lack():
    """Runs behind the walk: conditions on what it met, counted beforehand (30 seeds walked: 9 with
    isolated vertices, 9 with long rows, 4 with both, 9 renumbered; the worst row-scaled error of
    the walked values against the long-double reference is 9.0e-15, of K u 4.1e-14, seed 60)."""
    if len(WALKED) < 10:
        pytest.skip("the plan walk did not run in this session")
    rows = list(WALKED.values())
    assert len(rows) >= 20
    assert sum(r["isolated"] > 0 for r in rows) >= 6
    assert sum(r["long_rows"] > 0 for r in rows) >= 4
    assert sum(r["long_rows"] > 0 and r["isolated"] > 0 for r in rows) >= 1
    assert sum(r["renumbered"] for r in rows) >= 5
    assert sum(r["holes"] > 0 for r in rows) >= 15  # edge rows of ONE triangle


#: CG seeds of the sweep small enough for a dense Cholesky: pure stiffness (20; 73 with an isolated
#: vertex), pure mass (35), both terms (51, 66)
PD_SEEDS = (20, 35, 51, 66, 73)


@pytest.mark.parametrize("seed", PD_SEEDS)
def test_the_operator_cg_is_handed_is_positive_definite(seed, cases):
    case = cases(seed)
    free = p2ref.cg_free_dofs(case)
    assert free is not None and free.size > 0
    assert not case["lone"][free].any() and not p2ref.on_outer_boundary(case["xy"][free]).any()
    K = np.asarray(p2ref.reference_of(case, np.float64).dense()[np.ix_(free, free)])
    assert np.abs(K - K.T).max() <= 1e-12 * np.abs(K).max()
    np.linalg.cholesky(0.5 * (K + K.T))  # raises LinAlgError unless positive definite
    # ... and the loads and starts have the sweep's shape: a zero third column
    B, X0 = p2ref.cg_loads(case), p2ref.cg_start(case)
    assert B.shape == X0.shape == (case["n_dofs"], 3) and not B[:, 2].any() and not X0[:, 2].any()


def test_cg_is_refused_where_the_operator_is_not_positive_definite(cases):
    seen = set()
    for seed in range(N_SEEDS):
        case = cases(seed)
        free = p2ref.cg_free_dofs(case)
        if free is None:
            continue
        seen.add(seed)
        assert not case["single"] and case["n_dofs"] <= p2ref.CG_MAX_DOFS
        assert (p2ref.signed_area2(case["verts"], case["tris"]) > 0).all()
        assert case["beta"] == 0.0 or case["order"] == 4
    assert len(seen) >= 10


def test_check_rows_rejects_what_it_is_there_to_reject(cases):
    """The checker of the sweeps (test_hip_operator_fuzz.check_rows) on a reference vector of a
    large seed: the vector itself passes, ONE entry moved by 2 * tol * scale_i fails, and a
    non-zero in the row of an isolated vertex fails at any size."""
    from test_hip_operator_fuzz import check_rows

    tol = 1e-12
    case = cases(3)  # 11100 DoFs, 4 isolated vertices
    assert case["n_dofs"] > 10000 and case["isolated"] > 0
    ref = p2ref.reference_of(case)
    want, scale = ref.apply(case["u"])
    good = np.asarray(want, dtype=np.float64)
    check_rows(good, want, scale, tol, "the reference rounded to float64")
    row = int(np.argmax(scale))  # the largest row: a norm-wise bound would not see the smallest one
    small = int(np.flatnonzero(scale > 0)[np.argmin(scale[scale > 0])])
    for i in (row, small):
        bad = good.copy()
        bad[i] += 2.0 * tol * float(scale[i])
        assert bad[i] != good[i]
        with pytest.raises(AssertionError, match="reference"):
            check_rows(bad, want, scale, tol, "one entry off the reference")
    lone = int(np.flatnonzero(case["lone"])[0])
    assert scale[lone] == 0 and want[lone] == 0
    for size in (1.0, 1e-30, 5e-324):
        bad = good.copy()
        bad[lone] = size
        with pytest.raises(AssertionError, match="isolated"):
            check_rows(bad, want, scale, tol, "a non-zero in an isolated vertex's row")
    # a block: the same, column by column
    wide = np.stack([good, good], axis=1)
    wide[small, 1] += 2.0 * tol * float(scale[small])
    with pytest.raises(AssertionError):
        check_rows(wide, np.stack([want, want], axis=1), np.stack([scale, scale], axis=1), tol, "a block")
