"""Extended-precision reference of the P1 operator alpha * stiffness + beta * mass -- test
infrastructure, a plain module.

oracle/assembly_oracle.py follows the dtype of its coordinates: fed np.longdouble coordinates it
integrates the local matrices with 64-bit mantissas (x86 extended precision), about 3 decimal
digits beyond the float64 the kernels and the float64 oracle work in.  Everything here is summed
in long double as well (np.add.at: np.bincount would round its weights to float64).  A float32
case hands in the float32-ROUNDED coordinates; they are widened, never re-rounded.

Also here: the cases of the seeded operator sweep (tests/test_hip_operator_fuzz.py), so that the
sweep on the GPU and the CPU measurements its tolerances come from draw the same meshes, and those
measurements themselves (run this file: `python tests/operator_reference.py`)."""

from __future__ import annotations

import os
import sys

import numpy as np

if __name__ == "__main__":  # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import assembly_oracle as orc
from random_meshes import has_elements, random_mesh

LD = np.longdouble


class OperatorReference:
    """K = alpha * stiffness + beta * mass of a P1 mesh as long-double CSR values in the caller's
    numbering (the sorted-column pattern of oracle.csr_pattern)."""

    def __init__(self, verts, tris, order, alpha, beta, dtype=LD):
        verts = np.asarray(verts).astype(dtype)  # widening is exact
        tris = np.asarray(tris).astype(np.int64)
        self.n = int(verts.shape[0])
        self.dtype = np.dtype(dtype)
        geo = orc.geometry(verts[tris], 1, int(order))
        real = self.dtype.type
        integrand = real(alpha) * orc.integrand_stiffness(geo) + real(beta) * orc.integrand_mass(geo)
        local = orc.integrate_local(integrand, geo["dx"])
        assert local.dtype == self.dtype, local.dtype
        self.rowptr, self.colind, slots = orc.csr_pattern(tris, self.n)
        self.values = orc.assemble_csr_values(local, slots, self.colind.shape[0])
        self.rows = np.repeat(np.arange(self.n), np.diff(self.rowptr))
        self.has_row = np.diff(self.rowptr) > 0

    def _row_sums(self, per_entry):
        out = np.zeros(self.n, dtype=self.dtype)
        np.add.at(out, self.rows, per_entry)
        return out

    def apply(self, u):
        """(K u, sum_j |K_ij u_j|), both (N,) in the reference's precision."""
        prod = self.values * np.asarray(u).astype(self.dtype)[self.colind]
        return self._row_sums(prod), self._row_sums(np.abs(prod))

    def diagonal(self):
        """(diag K, sum_j |K_ij|): 0 where a row stores no entry."""
        hit = self.colind == self.rows
        diag = np.zeros(self.n, dtype=self.dtype)
        diag[self.rows[hit]] = self.values[hit]
        return diag, self._row_sums(np.abs(self.values))

    def dense(self):
        out = np.zeros((self.n, self.n), dtype=self.dtype)
        out[self.rows, self.colind] = self.values
        return out


def fan_weights(order):
    """(stiffness weight, mass diagonal, mass off-diagonal) per unit of the signed determinant, of
    the quadrature rule `order`: the three numbers the fan formula of the apply kernels multiplies
    (tests/test_operator_plan.py walks it in numpy)."""
    nodes, weights = orc.gauss_rule(order)
    weights = np.asarray(weights).reshape(-1)
    bary = np.asarray(orc.barycentric_coordinates(nodes)).reshape(-1, 3)
    return (0.5 * weights.sum(), float((0.5 * weights * bary[:, 0] * bary[:, 0]).sum()),
            float((0.5 * weights * bary[:, 0] * bary[:, 1]).sum()))


# --------------------------------------------------------------------------- #
# the cases of the operator sweep
# --------------------------------------------------------------------------- #

#: block widths: one pass (2, 4, 8), a pass plus a narrower tail (3, 5, 7, 9, 11, 17), two full
#: passes (16); 15-slot records cap a pass at 4 columns, so every width above 4 is several passes there
BLOCK_WIDTHS = (2, 3, 4, 5, 7, 8, 9, 11, 16, 17)
SEED_BASE = 5000
#: seeds (mod 10) that run under TFEM_RING_LONG=1: three in ten, so that more than ten of a hundred
#: meshes have a vertex with 8 .. 15 neighbours AND list it apart (a structured mesh has none)
LONG_ROW_SEEDS = (3, 4, 9)
#: CG runs on meshes up to this many vertices ("a few thousand")
CG_MAX_VERTS = 3000


def sweep_case(seed):
    """Everything seed `seed` of the operator sweep draws, in a fixed order, as a dict.  No GPU."""
    rng = np.random.default_rng(SEED_BASE + seed)
    verts, tris = random_mesh(rng)
    order = int(rng.integers(1, 5))
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
        # a vertex that keeps ONE element, its smallest: an open fan of one triangle, a small diagonal
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
    n = verts.shape[0]
    real = np.float32 if single else np.float64
    u = rng.standard_normal(n).astype(real)
    U = rng.standard_normal((n, k)).astype(real)
    long_rows = seed % 10 in LONG_ROW_SEEDS
    return {
        "seed": seed, "verts": verts, "tris": tris, "order": order, "alpha": alpha, "beta": beta,
        "int64": int64, "single": single, "k": k, "u": u, "U": U,
        "renumber": seed % 3 == 2, "long_rows": long_rows,
        "coefficients": seed % 2 == 0 and not long_rows,
        "isolated": int((~has_elements(tris, n)).sum()),
    }


def signed_area2(verts, tris):
    p = np.asarray(verts, dtype=np.float64)[tris]
    return (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])


def cg_free_dofs(case):
    """The DoFs CG solves for, or None where CG has no business.

    The forms are integrated with the SIGNED determinant of the connectivity's own orientation (as
    the reference does): an element stored clockwise contributes with a minus sign, and the operator
    of a mesh with mixed orientation is indefinite.  CG is a method for symmetric positive definite
    operators, so it runs where every element is stored counter-clockwise, in float64 (rtol 1e-10
    is below float32's resolution), on meshes of at most CG_MAX_VERTS vertices, and not for a mass
    form under the one-point rule (its element matrix is rank one, the global one may be singular).

    free = the vertices that have elements and do not lie on the outer boundary of the unit square;
    isolated vertices stay outside.  For a pure stiffness form (beta = 0) a connected group of free
    vertices with no Dirichlet neighbour carries the constants in its kernel; such groups (islands
    that element removal cut off) leave `free` too."""
    verts, tris = np.asarray(case["verts"], dtype=np.float64), case["tris"]
    n = verts.shape[0]
    if case["single"] or n > CG_MAX_VERTS or (signed_area2(verts, tris) <= 0).any():
        return None
    if case["alpha"] == 0.0 and case["order"] == 1:
        return None
    eps = 1e-12
    outer = ((np.abs(verts) <= eps) | (np.abs(verts - 1.0) <= eps)).any(axis=1)
    free = has_elements(tris, n) & ~outer
    if case["beta"] == 0.0:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        a = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]])
        b = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 0]])
        both = free[a] & free[b]
        graph = coo_matrix((np.ones(int(both.sum())), (a[both], b[both])), shape=(n, n))
        _, label = connected_components(graph, directed=False)
        anchored = np.zeros(label.max() + 1, dtype=bool)
        for p, q in ((a, b), (b, a)):
            edge = free[p] & ~free[q]  # q has elements (it is on this edge) and is held: a Dirichlet neighbour
            anchored[label[p[edge]]] = True
        free &= anchored[label]
    idx = np.flatnonzero(free)
    return idx if idx.size else None


def cg_loads(case):
    """(N, 3) right-hand sides of different difficulty: a smooth load, a random one, a zero column."""
    verts = np.asarray(case["verts"], dtype=np.float64)
    rng = np.random.default_rng(7000 + case["seed"])
    B = np.zeros((verts.shape[0], 3))
    B[:, 0] = np.sin(np.pi * verts[:, 0]) * np.sin(np.pi * verts[:, 1])
    B[:, 1] = rng.standard_normal(verts.shape[0])
    return B


def cg_start(case):
    """(N, 3) starting vectors: random everywhere (the entries outside `free` are Dirichlet values the
    solve must keep), zero for the zero column."""
    X0 = 0.1 * np.random.default_rng(8000 + case["seed"]).standard_normal((case["verts"].shape[0], 3))
    X0[:, 2] = 0.0
    return X0


def plan_of(case):
    """The ring plan the engine builds for the case under the environment the sweep sets (Morton
    renumbering, long rows), on the host; None when the mesh has no ring form."""
    import torch

    from pytorch_fem_solver_amd.basis.engine import _morton_permutation, ring_plan_host, symbolic_host

    verts, tris = np.asarray(case["verts"], dtype=np.float64), case["tris"]
    if case["renumber"]:
        perm = _morton_permutation(torch.tensor(case["verts"])).numpy()
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        verts, tris = verts[perm], inv[tris].astype(np.int32)
    n = verts.shape[0]
    rowptr, colind, _ = symbolic_host(tris, n)
    saved = {key: os.environ.get(key) for key in ("TFEM_RING_LONG", "TFEM_RING_WGS")}
    os.environ["TFEM_RING_LONG"] = "1" if case["long_rows"] else "0"
    os.environ["TFEM_RING_WGS"] = "1024"  # four workgroups on each of 256 CUs, what the engine sets on an MI355X
    try:
        return ring_plan_host(tris, n, verts, rowptr, colind), verts, tris
    except NotImplementedError:
        return None, verts, tris
    finally:
        for key, value in saved.items():
            if value is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = value


def row_error(got, want, scale):
    """conftest.rowwise_error with a caller's scale, spelled for long-double inputs: the difference
    is formed before anything is rounded to float64."""
    from conftest import rowwise_error

    diff = np.asarray(got).astype(LD) - np.asarray(want).astype(LD)
    return rowwise_error(np.asarray(diff, dtype=np.float64), np.zeros(diff.shape), scale=np.asarray(scale, dtype=np.float64))


# --------------------------------------------------------------------------- #
# the measurements behind the sweep's float32 bound and CG factor (CPU only)
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
        args = (case["verts"], case["tris"], case["order"], case["alpha"], case["beta"])
        ref, low = OperatorReference(*args), OperatorReference(*args, dtype=np.float32)
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
    oracle's CSR operator (torch on the CPU) over the CG seeds of the sweep and their two non-zero
    loads, the true residual from the long-double reference matrix."""
    import torch

    from pytorch_fem_solver_amd.sparse import conjugate_gradients

    worst = 0.0
    for seed in range(n_seeds):
        case = sweep_case(seed)
        free = cg_free_dofs(case)
        if free is None:
            continue
        args = (case["verts"], case["tris"], case["order"], case["alpha"], case["beta"])
        ref, low = OperatorReference(*args), OperatorReference(*args, dtype=np.float64)
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


def true_residual(ref, x, b, free):
    """||b - K x|| / ||b|| on `free`, K the long-double reference."""
    r = (np.asarray(b).astype(LD) - ref.apply(x)[0])[free]
    return float(np.sqrt((r * r).sum()) / np.sqrt((np.asarray(b).astype(LD)[free] ** 2).sum()))


def route_counts(n_seeds=100):
    """What the plans of the sweep's cases look like, from ring_plan_host on the CPU."""
    counts = {"matrix_free": 0, "slots_7": 0, "slots_15": 0, "chunked": 0, "isolated": 0, "long_rows": 0,
              "float32": 0, "int64": 0, "cg": 0, "coefficients": 0}
    for seed in range(n_seeds):
        case = sweep_case(seed)
        plan = plan_of(case)[0]
        if plan is None:
            print(f"seed {seed}: no ring plan")
            continue
        counts["matrix_free"] += 1
        counts[f"slots_{plan['slots']}"] += 1
        counts["chunked"] += plan["chunked"]
        counts["isolated"] += case["isolated"] > 0
        counts["long_rows"] += case["long_rows"] and plan["long_rows"].size > 0
        counts["float32"] += case["single"]
        counts["int64"] += case["int64"]
        counts["cg"] += cg_free_dofs(case) is not None
        counts["coefficients"] += case["coefficients"]
    return counts


if __name__ == "__main__":
    print(route_counts())
    print("float32, worst row-scaled error of the float32 oracle (K u, diag K):", measure_float32())
    print("CG, worst |true - recurrence residual| / rtol:", measure_cg())
