"""Extended-precision reference of the P2 operator alpha * stiffness + beta * mass, and the cases of
the seeded P2 operator sweep (tests/test_hip_p2_operator_fuzz.py) -- test infrastructure, a plain
module, the P2 sibling of tests/operator_reference.py.

oracle/assembly_oracle.py follows the dtype of its coordinates for P2 as well: fed np.longdouble
coordinates, geometry(..., 2, q) integrates the 6 x 6 local matrices with 64-bit mantissas.  The
sums are those of operator_reference.OperatorReference (np.add.at in the reference's precision);
a float32 case hands in its float32-ROUNDED coordinates, which are widened, never re-rounded.

Also here, so that the sweep on the GPU and the CPU measurements behind its tolerances draw the
same meshes: the cases (sweep_case), the plan the engine will build for a case or the reason it
will build none (plan_of), where CG runs (cg_free_dofs), and the measurements themselves.  Run this
file (`python tests/p2_operator_reference.py`) to print, in this order: one line per refused seed
and the route counts of the 100 default seeds; the float32 oracle's row-scaled error per float32
seed and the worst (K u, diag K); the drift of the CG recurrence per CG seed and load and the
worst |true - recurrence| / rtol."""

from __future__ import annotations

import os
import sys

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import operator_reference as oref
from operator_reference import LD, row_error, signed_area2, true_residual  # noqa: F401  (shared with the sweep)
from oracle import assembly_oracle as orc
from random_meshes import has_elements, random_mesh


class P2OperatorReference(oref.OperatorReference):
    """K = alpha * stiffness + beta * mass of a P2 mesh as CSR values in `dtype` (long double by
    default) in the numbering of `conn6` (the sorted-column pattern of oracle.csr_pattern).
    apply(), diagonal() and dense() are OperatorReference's."""

    def __init__(self, verts, tris, conn6, n_dofs, order, alpha, beta, dtype=LD):
        verts = np.asarray(verts).astype(dtype)  # widening is exact
        tris = np.asarray(tris).astype(np.int64)
        conn6 = np.asarray(conn6).astype(np.int64)
        self.n = int(n_dofs)
        self.dtype = np.dtype(dtype)
        geo = orc.geometry(verts[tris], 2, int(order))
        real = self.dtype.type
        integrand = real(alpha) * orc.integrand_stiffness(geo) + real(beta) * orc.integrand_mass(geo)
        local = orc.integrate_local(integrand, geo["dx"])
        assert local.dtype == self.dtype and local.shape[-2:] == (6, 6), (local.dtype, local.shape)
        self.rowptr, self.colind, slots = orc.csr_pattern(conn6, self.n)
        self.values = orc.assemble_csr_values(local, slots, self.colind.shape[0])
        self.rows = np.repeat(np.arange(self.n), np.diff(self.rowptr))
        self.has_row = np.diff(self.rowptr) > 0


def reference_of(case, dtype=LD, conn6=None):
    """The reference of a case, in the caller's numbering (or in that of another `conn6`)."""
    return P2OperatorReference(case["verts"], case["tris"], case["conn6"] if conn6 is None else conn6,
                               case["n_dofs"], case["order"], case["alpha"], case["beta"], dtype)


# --------------------------------------------------------------------------- #
# the cases of the P2 operator sweep
# --------------------------------------------------------------------------- #

#: block widths against the pass widths {2, 4} of k_p2_apply_rows_multi: one pass (2, 4), a pass
#: with a narrower tail (3: 4 with one column idle; 5, 6: 4 + 2), two full passes (8), two passes
#: and a tail (7, 9).  Under TFEM_P2_APPLY_NV=2 every pass has width 2: one to five passes.
BLOCK_WIDTHS = (2, 3, 4, 5, 6, 7, 8, 9)
SEED_BASE = 9000
#: CG runs on meshes up to this many DoFs: measure_cg() over the default seeds takes about a minute on a CPU
CG_MAX_DOFS = 6000
#: the engine renumbers the edge DoFs of a basis of this size on its own (AssemblyEngine.RENUMBER_MIN_DOFS)
RENUMBER_MIN_DOFS = 50000
EPS_BOUNDARY = 1e-12


def on_outer_boundary(points):
    """(n,) bool: the points on the boundary of the unit square."""
    points = np.asarray(points, dtype=np.float64)
    return ((np.abs(points) <= EPS_BOUNDARY) | (np.abs(points - 1.0) <= EPS_BOUNDARY)).any(axis=1)


def sweep_case(seed):
    """Everything seed `seed` of the P2 operator sweep draws, in a fixed order, as a dict.  No GPU.

    Drawn from default_rng(SEED_BASE + seed): the mesh (the FIRST draw: random_meshes.random_mesh),
    the quadrature order, (alpha, beta), the index type, the real type, the block width, the "one
    vertex keeps only its smallest element" edit, u and U.  From the seed itself: `renumber_env`
    (seed % 3 == 2: the sweep sets TFEM_RENUMBER=1) and `nv_cap` (seed % 4 == 1: TFEM_P2_APPLY_NV=2).
    `renumber` is what the engine then does: it renumbers the edge DoFs when told to, and on its own
    from RENUMBER_MIN_DOFS DoFs on (the sweep leaves TFEM_RENUMBER unset on the other seeds: the
    engine's default is what runs)."""
    from pytorch_fem_solver_amd import dofs, meshgen

    rng = np.random.default_rng(SEED_BASE + seed)
    verts, tris = random_mesh(rng)
    order = int(rng.integers(2, 5))
    r = rng.random()
    if r < 0.3:
        alpha, beta = 1.0, 0.0
    elif r < 0.5:
        alpha, beta = 0.0, 1.0
    else:
        alpha, beta = float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.0, 3.0))
    int64 = bool(rng.random() < 0.5)
    single = bool(rng.random() < 0.15)  # float32: the coordinates are rounded first
    k = int(rng.choice(BLOCK_WIDTHS))
    if rng.random() < 0.25:
        # a vertex that keeps ONE element, its smallest (the edit of operator_reference.sweep_case)
        counts = np.bincount(tris.reshape(-1), minlength=verts.shape[0])
        rich = np.flatnonzero(counts >= 3)
        if rich.size:
            v = int(rich[rng.integers(rich.size)])
            mine = np.flatnonzero((tris == v).any(axis=1))
            p = verts[tris[mine]]
            area2 = np.abs((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1])
                           - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1]))
            drop = np.delete(mine, int(np.argmin(area2)))
            tris = np.ascontiguousarray(np.delete(tris, drop, axis=0))
    if single:
        verts = verts.astype(np.float32)
    n_verts = verts.shape[0]
    # the mesh dictionary of the public API.  Edge markers: 1 on the edges of ONE triangle (the
    # outer boundary and the rims of the holes) -- MeshTri pairs every other edge with two cells;
    # vertex markers: 1 on the outer boundary of the unit square, as in the P1 sweep
    edges, one_sided = meshgen._edges_from_triangles(tris)
    vertex_markers = on_outer_boundary(verts).astype(np.int32).reshape(-1, 1)
    edge_markers = one_sided.astype(np.int32).reshape(-1, 1)
    conn6, xy, _ = dofs.p2_dofs_numpy(verts, tris, edges, edge_markers, vertex_markers)
    n_dofs = xy.shape[0]
    mesh = {"vertices": verts, "vertex_markers": vertex_markers,
            "triangles": tris.astype(np.int64) if int64 else tris, "edges": edges, "edge_markers": edge_markers,
            "neighbors": meshgen._neighbors_from_triangles(tris, n_verts)}
    real = np.float32 if single else np.float64
    u = rng.standard_normal(n_dofs).astype(real)
    U = rng.standard_normal((n_dofs, k)).astype(real)
    renumber_env = seed % 3 == 2
    lone = np.zeros(n_dofs, dtype=bool)
    lone[:n_verts] = ~has_elements(tris, n_verts)
    return {
        "seed": seed, "verts": verts, "tris": tris, "order": order, "alpha": alpha, "beta": beta,
        "int64": int64, "single": single, "k": k, "u": u, "U": U, "mesh": mesh, "edges": edges,
        "conn6": conn6, "xy": xy, "n_verts": n_verts, "n_dofs": n_dofs, "lone": lone,
        "renumber_env": renumber_env, "renumber": renumber_env or n_dofs >= RENUMBER_MIN_DOFS,
        "nv_cap": seed % 4 == 1, "isolated": int(lone.sum()),
    }


def engine_numbering(case):
    """(conn6, perm) of the engine for the case, formed on the host: the caller's when the engine
    does not renumber (perm None), else the edge DoFs along the Morton curve of the edge midpoints,
    by the statements of AssemblyEngine.__init__ with torch on the CPU (midpoints in the case's real
    type; the additions and the division of _morton_permutation are correctly rounded on either
    device, the sort is stable on both).  DoF perm[k] of the caller is DoF k of the engine."""
    if not case["renumber"]:
        return case["conn6"], None
    import torch

    from pytorch_fem_solver_amd.basis.engine import _morton_permutation

    n_v, n_e = case["n_verts"], case["n_dofs"] - case["n_verts"]
    cpu = torch.device("cpu")  # whatever the default device of the caller (the sweep's is the GPU)
    coords = torch.tensor(case["verts"], device=cpu)
    tri = torch.tensor(case["tris"].astype(np.int64), device=cpu)
    edge = torch.tensor(case["conn6"][:, 3:].astype(np.int64), device=cpu) - n_v
    mid = torch.zeros((n_e, 2), dtype=coords.dtype, device=cpu)
    for j in range(3):
        mid[edge[:, j]] = 0.5 * (coords[tri[:, j]] + coords[tri[:, (j + 1) % 3]])
    edge_perm = _morton_permutation(mid)
    edge_inv = torch.empty_like(edge_perm)
    edge_inv[edge_perm] = torch.arange(n_e, device=cpu)
    conn6 = torch.cat([tri, n_v + edge_inv[edge]], dim=1).numpy().astype(np.int32)
    perm = np.concatenate([np.arange(n_v), n_v + edge_perm.numpy()])
    return conn6, perm


def plan_of(case):
    """(plan, conn6, perm, rowptr): what p2_plan_host builds for the case in the engine's numbering
    (engine_numbering: renumbered cases included, their edge permutation needs no device), on the
    host.  `plan` is the plan's dict, or the MESSAGE of the refusal (a str) where the engine will
    have no plan; rowptr is the CSR row pointer in that numbering."""
    from pytorch_fem_solver_amd.basis.engine import p2_plan_host, pattern_host

    conn6, perm = engine_numbering(case)
    rowptr, colind = pattern_host(conn6, case["n_dofs"])
    try:
        plan = p2_plan_host(conn6, case["n_verts"], case["n_dofs"], np.asarray(case["verts"], dtype=np.float64),
                            rowptr, colind)
    except NotImplementedError as exc:
        plan = str(exc)
    return plan, conn6, perm, rowptr


def plan_facts(plan):
    """What the sweep records of a plan: tiles per kind, long rows."""
    z = [int(x) for x in plan["layout"]]
    return {"vertex_tiles": z[0], "edge_tiles": z[1], "long_rows": z[18]}


def cg_free_dofs(case):
    """The DoFs CG solves for, or None where CG has no business.

    CG is a method for symmetric positive definite operators.  The forms are integrated with the
    SIGNED determinant (operator_reference.cg_free_dofs), so every element has to be stored
    counter-clockwise; the case is float64 (rtol 1e-10 is below float32's resolution) with at most
    CG_MAX_DOFS DoFs; and a mass term needs the order-4 rule: the order-3 rule has a weight of
    -0.5625 and the order-2 rule (three points) gives a rank-3 P2 element mass matrix, so an
    under-integrated mass term is not positive definite.  The P2 stiffness integrand has degree 2
    and is exact from order 2 on.

    free = the vertex DoFs that have elements and all edge DoFs, without those on the outer
    boundary of the unit square (an edge is on it when its midpoint is).  For a pure stiffness form
    (beta = 0) the connected groups of free DoFs without a held neighbour carry the constants in
    their kernel (islands that element removal cut off) and leave `free` too; DoFs are neighbours
    when an element holds both (conn6)."""
    if case["single"] or case["n_dofs"] > CG_MAX_DOFS or (signed_area2(case["verts"], case["tris"]) <= 0).any():
        return None
    if case["beta"] != 0.0 and case["order"] != 4:
        return None
    n, conn6 = case["n_dofs"], case["conn6"].astype(np.int64)
    free = ~case["lone"] & ~on_outer_boundary(case["xy"])
    if case["beta"] == 0.0:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        a = np.concatenate([conn6[:, i] for i in range(6) for j in range(6) if i != j])
        b = np.concatenate([conn6[:, j] for i in range(6) for j in range(6) if i != j])
        both = free[a] & free[b]
        graph = coo_matrix((np.ones(int(both.sum())), (a[both], b[both])), shape=(n, n))
        _, label = connected_components(graph, directed=False)
        anchored = np.zeros(label.max() + 1, dtype=bool)
        held = free[a] & ~free[b]  # b is a DoF of this element and is held: a Dirichlet neighbour
        anchored[label[a[held]]] = True
        free &= anchored[label]
    idx = np.flatnonzero(free)
    return idx if idx.size else None


def cg_loads(case):
    """(N, 3) right-hand sides at the DoFs' coordinates: operator_reference.cg_loads (a smooth
    load, a random one, a zero column)."""
    return oref.cg_loads({"verts": case["xy"], "seed": case["seed"]})


def cg_start(case):
    """(N, 3) starting vectors: operator_reference.cg_start."""
    return oref.cg_start({"verts": case["xy"], "seed": case["seed"]})


# --------------------------------------------------------------------------- #
# the measurements behind the sweep's float32 bound, CG factor and coverage limits (CPU only)
# --------------------------------------------------------------------------- #


def measure_float32(n_seeds=100):
    """Worst row-scaled error of the ORACLE run in float32 (coordinates, tables, alpha / beta, the
    CSR values and the row sums all float32) against the long-double reference on the same
    float32-rounded coordinates, over the float32 seeds of the sweep: (K u, diag K)."""
    worst_apply = worst_diag = 0.0
    for seed in range(n_seeds):
        case = sweep_case(seed)
        if not case["single"]:
            continue
        ref, low = reference_of(case), reference_of(case, np.float32)
        assert low.values.dtype == np.float32
        want, scale = ref.apply(case["u"])
        e_apply = row_error(low.apply(case["u"])[0], want, scale)
        d_want, d_scale = ref.diagonal()
        e_diag = row_error(low.diagonal()[0], d_want, d_scale)
        print(f"seed {seed}: n = {ref.n}, order {case['order']}, K u {e_apply:.3e}, diag K {e_diag:.3e}")
        worst_apply, worst_diag = max(worst_apply, e_apply), max(worst_diag, e_diag)
    return worst_apply, worst_diag


def measure_cg(n_seeds=100, rtol=1e-10):
    """Worst |true residual - recurrence residual| / rtol of conjugate_gradients with the float64
    oracle's P2 CSR operator (torch on the CPU) over the CG seeds of the sweep and their two
    non-zero loads, the true residual from the long-double reference matrix."""
    import torch

    from pytorch_fem_solver_amd.sparse import conjugate_gradients

    worst = 0.0
    for seed in range(n_seeds):
        case = sweep_case(seed)
        free = cg_free_dofs(case)
        if free is None:
            continue
        ref, low = reference_of(case), reference_of(case, np.float64)
        K = torch.sparse_csr_tensor(torch.tensor(low.rowptr), torch.tensor(low.colind.astype(np.int64)),
                                    torch.tensor(low.values), size=(ref.n, ref.n))
        diag = torch.tensor(low.diagonal()[0])
        B, X0 = cg_loads(case), cg_start(case)
        for col in (0, 1):
            x, it, res = conjugate_gradients(lambda v: K @ v, diag, torch.tensor(B[:, col]), torch.tensor(free),
                                             torch.tensor(X0[:, col]), rtol)
            true = true_residual(ref, x.numpy(), B[:, col], free)
            drift = abs(true - res) / rtol
            print(f"seed {seed}: n = {ref.n}, column {col}, {it} iterations, recurrence {res:.3e}, true {true:.3e}, "
                  f"drift / rtol {drift:.3e}")
            assert res <= rtol
            worst = max(worst, drift)
    return worst


def route_of(case, plan):
    """What a seed reaches, from its case and its host plan (or refusal): the record the sweep keeps."""
    has_plan = not isinstance(plan, str)
    facts = plan_facts(plan) if has_plan else {"vertex_tiles": 0, "edge_tiles": 0, "long_rows": 0}
    return {"plan": has_plan, **facts, "isolated": case["isolated"], "int64": case["int64"],
            "float32": case["single"], "renumbered": case["renumber"], "nv_cap": case["nv_cap"], "k": case["k"],
            "n": case["n_dofs"], "cg": cg_free_dofs(case) is not None}


def count_routes(routes):
    """The coverage counts of a list of route records (route_of)."""
    def count(pred):
        return sum(1 for r in routes if pred(r))

    return {
        "plan": count(lambda r: r["plan"]), "refused": count(lambda r: not r["plan"]),
        "long_rows": count(lambda r: r["plan"] and r["long_rows"] > 0),
        "isolated": count(lambda r: r["plan"] and r["isolated"] > 0),
        "long_and_isolated": count(lambda r: r["plan"] and r["long_rows"] > 0 and r["isolated"] > 0),
        "many_tiles": count(lambda r: r["vertex_tiles"] > 1 and r["edge_tiles"] > 1),
        "int64": count(lambda r: r["int64"]), "int32": count(lambda r: not r["int64"]),
        "float32": count(lambda r: r["float32"]), "float32_with_plan": count(lambda r: r["float32"] and r["plan"]),
        "renumbered": count(lambda r: r["renumbered"]), "nv_cap": count(lambda r: r["nv_cap"] and r["plan"]),
        "k": {k: count(lambda r, k=k: r["k"] == k and r["plan"]) for k in BLOCK_WIDTHS},
        "cg": count(lambda r: r["cg"]), "cg_with_plan": count(lambda r: r["cg"] and r["plan"]),
        "cg_with_isolated": count(lambda r: r["cg"] and r["plan"] and r["isolated"] > 0),
    }


def route_counts(n_seeds=100):
    """What the sweep's cases reach, from p2_plan_host on the CPU."""
    routes = []
    for seed in range(n_seeds):
        case = sweep_case(seed)
        plan = plan_of(case)[0]
        if isinstance(plan, str):
            print(f"seed {seed}: no P2 row plan ({case['n_dofs']} DoFs): {plan}")
        routes.append(route_of(case, plan))
    return count_routes(routes)


if __name__ == "__main__":
    print(route_counts())
    print("float32, worst row-scaled error of the float32 oracle (K u, diag K):", measure_float32())
    print("CG, worst |true - recurrence residual| / rtol:", measure_cg())
