"""P1 forms with coefficient DATA on a real MI355X: the data launches (csrc/tfem_rings_field.hip)
through the C ABI, the engine and the public API, every path against ONE reference
(tests/field_reference.py: the oracle's quadrature on the same (E, Q) arrays; tolerance = the ring
kernels' parity tolerance times max |K^ref|, row-wise for K u and diag K, times max |gradient| for the
adjoint).  The data are seeded, uniform in [0.5, 1.5], independent per (e, q): a wrong element,
point weight, local index or orientation shows."""

import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import field_reference as fref
from conftest import REPO, load_golden, mesh_from_golden

pytestmark = pytest.mark.gpu

RATIOS = []  # max |err| / tol of every comparison of the running test


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    del RATIOS[:]
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)
    if RATIOS:  # real numbers were compared: somewhere the error is not exactly zero
        print(f"{len(RATIOS)} comparisons, max |err| / tol = {max(RATIOS):.3e}")
        assert 0.0 < max(RATIOS) <= 1.0


def tf():
    import pytorch_fem_solver_amd

    return pytorch_fem_solver_amd


#: (alpha, beta, kappa given, c given): stiffness alone, mass alone, one field beside a plain term, both
FORMS = {
    "kappa": (1.0, 0.0, True, False),
    "c": (0.0, 1.0, False, True),
    "kappa_plain_mass": (2.0, 0.5, True, False),
    "plain_stiffness_c": (1.0, 3.0, False, True),
    "kappa_c": (0.5, 2.0, True, True),
}


def _holes(mesh_np, seed=11):
    tri = mesh_np["triangles"].copy()
    rng = np.random.default_rng(seed)
    tri = tri[rng.random(tri.shape[0]) >= 0.1]
    flip = rng.random(tri.shape[0]) < 0.4
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return {"vertices": mesh_np["vertices"], "vertex_markers": mesh_np["vertex_markers"], "triangles": tri}


def _mesh(name):
    from pytorch_fem_solver_amd import meshgen

    if name.endswith(".npz"):
        return mesh_from_golden(load_golden(name))
    if name == "square_chunked":  # 4 tiles of consecutive vertices, element lists in run form
        return meshgen.unit_square(30, 0.25, 4)
    if name == "square_multi_tile":  # 7 tiles, vertex ids and row offsets from the plan
        return meshgen.unit_square(40, 0.25, 1)
    if name == "delaunay_15_slots":  # 15-slot records, rows of up to 12 entries
        return meshgen.delaunay_square(2500, 9)
    if name == "mixed_orientation":
        m = meshgen.unit_square(30, 0.25, 4)
        tri = m["triangles"].copy()
        flip = np.random.default_rng(5).random(tri.shape[0]) < 0.4
        tri[flip] = tri[flip][:, [0, 2, 1]]
        m["triangles"] = tri
        return m
    if name == "holes":  # removed elements, mixed orientation: open fans, flags 0 / 2, isolated rows
        return _holes(meshgen.unit_square(30, 0.25, 4))
    if name == "rotated_shuffled":  # local numbering rotated by e % 3, element order shuffled: list form, loc != 0
        m = meshgen.unit_square(30, 0.25, 4)
        tri = m["triangles"].copy()
        for r in (1, 2):
            tri[r::3] = np.roll(tri[r::3], r, axis=1)
        m["triangles"] = np.ascontiguousarray(tri[np.random.default_rng(3).permutation(tri.shape[0])])
        return m
    if name == "shuffled":  # a vertex numbering without locality: renumbered inside the engine (TFEM_RENUMBER=1)
        m = meshgen.unit_square(30, 0.25, 4)
        return meshgen.permute_mesh(m, vertex_order=np.random.default_rng(7).permutation(m["vertices"].shape[0]))
    raise KeyError(name)


def _engine(mesh_np, order, dtype=torch.float64):
    from pytorch_fem_solver_amd.basis.engine import AssemblyEngine

    idx = torch.tensor(np.ascontiguousarray(mesh_np["triangles"], dtype=np.int32))
    verts = torch.tensor(np.ascontiguousarray(mesh_np["vertices"]), dtype=dtype)
    return AssemblyEngine(verts, idx, idx, verts.shape[0], 1, order)


def _np_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _record(ratio):
    RATIOS.append(ratio)


def _host(t):
    return t.detach().double().cpu().numpy()


def _host_plan(rings):
    from pytorch_fem_solver_amd.basis.engine import unpack_ring_plan

    return unpack_ring_plan(rings["blob"].cpu().numpy(), rings["layout"])


def _elem_modes(plan):
    return set((plan["desc"].reshape(-1, 20)[:, 18] & 0xFF).tolist())


def _assert_plan(mesh, rings):
    """What each mesh of the table is meant to exercise."""
    slots, chunked, n_tiles = int(rings["layout"][6]), rings["chunked"], rings["n_tiles"]
    assert int(rings["layout"][23]) == 0 and int(rings["layout"][18]) == 1
    if mesh == "square_chunked":
        assert chunked and n_tiles > 1 and slots == 7 and 1 in _elem_modes(_host_plan(rings))
    if mesh == "square_multi_tile":
        assert not chunked and n_tiles > 1 and slots == 7
    if mesh == "delaunay_15_slots":
        assert slots == 15 and n_tiles > 1
    if mesh == "rotated_shuffled":
        plan = _host_plan(rings)
        assert _elem_modes(plan) == {0} and n_tiles > 1
        codes = plan["row_ecodes"]
        assert ((codes & 0xFFF) != 0xFFF).any() and (((codes & 0xFFF) >> 10) % 3 != 0).any()  # loc != 0


ENGINE_CASES = [
    ("p1_square_n8.npz", torch.float64), ("p1_square_n5_clockwise.npz", torch.float64),
    ("p1_square_n6_float32.npz", torch.float32),
    ("square_chunked", torch.float64), ("square_multi_tile", torch.float64), ("square_multi_tile", torch.float32),
    ("delaunay_15_slots", torch.float64), ("mixed_orientation", torch.float64), ("holes", torch.float64),
    ("rotated_shuffled", torch.float64),
]


def _data(mesh_np, order, given, seed, dtype, per_element=False):
    return fref.data(mesh_np, order, seed, _np_dtype(dtype), per_element) if given else None


def _dev(values, dtype):
    return None if values is None else torch.tensor(values, dtype=dtype)


def _head(eng, rings, order, alpha, beta, kappa, c):
    from pytorch_fem_solver_amd import _native

    d = eng._inputs()
    return (_native.ptr(d["coords"]), eng.real_bytes, eng.n_dofs, order, alpha, beta,
            _native.ptr(kappa), 0 if kappa is None else kappa.shape[1], _native.ptr(c), 0 if c is None else c.shape[1],
            eng.n_elems, _native.ptr(rings["blob"]), c_void_p(rings["layout"].ctypes.data))


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("mesh,dtype", ENGINE_CASES)
def test_c_abi_store_apply_and_diagonal_against_the_reference(mesh, dtype, order):
    """tfem_p1_rings_field and tfem_p1_apply_rings_field (K u, diag K) on the engine's plan; two
    identical launches give identical bits."""
    from pytorch_fem_solver_amd import _native

    mesh_np = _mesh(mesh)
    eng = _engine(mesh_np, order, dtype)
    rings = eng.ring_plan()
    assert rings is not None and not eng.renumbered
    _assert_plan(mesh, rings)
    n = eng.n_dofs
    u_np = np.random.default_rng(order).standard_normal(n)
    crow, ccol = eng.csr_structure()[0].cpu().numpy(), eng.csr_structure()[1].cpu().numpy()
    for name, (alpha, beta, has_k, has_c) in FORMS.items():
        kv, cv = _data(mesh_np, order, has_k, 10 + order, dtype), _data(mesh_np, order, has_c, 20 + order, dtype)
        parts = fref.reference_parts(mesh_np, order, alpha, beta, kv, cv, _np_dtype(dtype))
        rowptr, colind, want, tol = parts[:4]
        assert np.array_equal(crow, rowptr) and np.array_equal(ccol, colind)
        kd, cd = _dev(kv, dtype), _dev(cv, dtype)
        head = _head(eng, rings, order, alpha, beta, kd, cd)
        what = f"{mesh} {dtype} order {order} {name}"
        both = []
        for _ in range(2):
            vals = torch.full((colind.shape[0],), float("nan"), dtype=dtype)
            if eng.field_refusal(beta, "store") is None:
                _native.check(eng.lib.tfem_p1_rings_field(*head, _native.ptr(vals), eng._stream()))
            else:  # the launch says what the engine says, and writes nothing
                assert eng.lib.tfem_p1_rings_field(*head, _native.ptr(vals), eng._stream()) == 2
            u = torch.tensor(u_np, dtype=dtype)
            y = torch.full((n,), float("nan"), dtype=dtype)
            _native.check(eng.lib.tfem_p1_apply_rings_field(*head, _native.ptr(u), _native.ptr(y), eng._stream()))
            dg = torch.full((n,), float("nan"), dtype=dtype)
            _native.check(eng.lib.tfem_p1_apply_rings_field(*head, None, _native.ptr(dg), eng._stream()))
            torch.cuda.synchronize()
            both.append((vals, y, dg))
        for a, b in zip(*both):
            assert torch.equal(a, b) or bool(torch.isnan(a).all() and torch.isnan(b).all()), f"{what}: not repeatable"
        vals, y, dg = both[0]
        has_row = np.diff(rowptr) > 0
        if eng.field_refusal(beta, "store") is None:
            _record(fref.check(_host(vals), want, tol, f"{what}: values"))
        else:
            assert bool(torch.isnan(vals).all())
        want_y, tol_y = fref.apply_reference(parts, _host(u))
        got_y = _host(y)
        assert np.array_equal(got_y[~has_row], np.zeros(int((~has_row).sum())))  # a vertex without elements
        _record(fref.check(got_y[has_row], want_y[has_row], tol_y[has_row], f"{what}: K u"))
        diag_at = np.array([rowptr[i] + np.searchsorted(colind[rowptr[i]:rowptr[i + 1]], i) for i in range(n) if has_row[i]])
        _, tol_d = fref.apply_reference(parts, np.ones(n))
        _record(fref.check(_host(dg)[has_row], want[diag_at], tol_d[has_row], f"{what}: diag K"))


@pytest.mark.parametrize("mesh,dtype", [("square_chunked", torch.float64), ("rotated_shuffled", torch.float64),
                                        ("delaunay_15_slots", torch.float64), ("square_multi_tile", torch.float32)])
def test_one_value_per_element_gives_what_the_expanded_data_gives(mesh, dtype):
    from pytorch_fem_solver_amd import _native

    order = 3
    mesh_np = _mesh(mesh)
    eng = _engine(mesh_np, order, dtype)
    rings = eng.ring_plan()
    n = eng.n_dofs
    alpha, beta = 0.5, 2.0
    k1, c1 = (_data(mesh_np, order, True, s, dtype, per_element=True) for s in (31, 32))
    nq = eng.n_quad
    parts = fref.reference_parts(mesh_np, order, alpha, beta, np.repeat(k1, nq, 1), np.repeat(c1, nq, 1), _np_dtype(dtype))
    rowptr, colind, want, tol = parts[:4]
    u = torch.tensor(np.random.default_rng(4).standard_normal(n), dtype=dtype)
    want_y, tol_y = fref.apply_reference(parts, _host(u))
    has_row = np.diff(rowptr) > 0
    stored = eng.field_refusal(beta, "store") is None
    assert stored == (mesh != "delaunay_15_slots")  # fp64, 15 slots, mass: the store launch's LDS need is refused
    for label, kd, cd in (("per element", _dev(k1, dtype), _dev(c1, dtype)),
                          ("expanded", _dev(np.repeat(k1, nq, 1), dtype), _dev(np.repeat(c1, nq, 1), dtype)),
                          ("mixed", _dev(k1, dtype), _dev(np.repeat(c1, nq, 1), dtype))):
        head = _head(eng, rings, order, alpha, beta, kd, cd)
        y = torch.full((n,), float("nan"), dtype=dtype)
        _native.check(eng.lib.tfem_p1_apply_rings_field(*head, _native.ptr(u), _native.ptr(y), eng._stream()))
        _record(fref.check(_host(y)[has_row], want_y[has_row], tol_y[has_row], f"{mesh} {label}: K u"))
        if stored:
            vals = torch.full((colind.shape[0],), float("nan"), dtype=dtype)
            _native.check(eng.lib.tfem_p1_rings_field(*head, _native.ptr(vals), eng._stream()))
            _record(fref.check(_host(vals), want, tol, f"{mesh} {label}: values"))


def test_refusal_codes_on_the_device_leave_the_outputs_untouched(monkeypatch):
    from pytorch_fem_solver_amd import _native

    mesh_np = _mesh("p1_square_n8.npz")
    eng = _engine(mesh_np, 3)
    rings = eng.ring_plan()
    n = eng.n_dofs
    kd = _dev(fref.data(mesh_np, 3, 1), torch.float64)
    vals = torch.full((int(eng.csr_structure()[1].shape[0]),), 7.0)
    u, y = torch.ones(n), torch.full((n,), 7.0)
    good = _head(eng, rings, 3, 1.0, 1.0, kd, None)

    def store(head):
        return eng.lib.tfem_p1_rings_field(*head, _native.ptr(vals), eng._stream())

    def apply(head, u_, y_):
        return eng.lib.tfem_p1_apply_rings_field(*head, _native.ptr(u_), _native.ptr(y_), eng._stream())

    def but(**change):
        names = ("coords", "real_bytes", "n_verts", "order", "alpha", "beta", "kappa", "knq", "c", "cnq", "n_elems",
                 "plan", "layout")
        head = dict(zip(names, good))
        head.update(change)
        return tuple(head[k] for k in names)

    assert store(but(real_bytes=3)) == 1 and store(but(layout=None)) == 1 and store(but(n_verts=-1)) == 1
    assert store(but(knq=3)) == 1 and store(but(kappa=None)) == 1 and store(but(order=9)) == 2
    assert apply(good, u, u) == 1 and apply(good, y, y) == 1
    assert apply(but(n_elems=1 << 29), u, y) == 4
    layout = rings["layout"].copy()
    layout[18] = 0
    assert store(but(layout=c_void_p(layout.ctypes.data))) == 2
    layout[18], layout[23] = 1, 2
    assert apply(but(layout=c_void_p(layout.ctypes.data)), u, y) == 2
    layout[23], layout[0] = 0, 0
    assert store(but(layout=c_void_p(layout.ctypes.data))) == 0  # an empty plan: success, nothing launched
    torch.cuda.synchronize()
    assert bool((vals == 7.0).all()) and bool((y == 7.0).all()) and bool((u == 1.0).all())
    # a real plan with long rows: the engine does not offer it, the launch refuses it
    monkeypatch.setenv("TFEM_RING_LONG", "1")
    long_np = _mesh("delaunay_15_slots")
    eng_l = _engine(long_np, 3)
    rings_l = eng_l.ring_plan()
    assert rings_l is not None and int(rings_l["layout"][23]) > 0
    assert "long rows" in eng_l.field_refusal(0.0, "apply")
    kl = _dev(fref.data(long_np, 3, 2), torch.float64)
    assert eng_l.bilinear_field(1.0, 0.0, (kl, None)) is None
    yl = torch.full((eng_l.n_dofs,), 7.0)
    assert eng_l.lib.tfem_p1_apply_rings_field(*_head(eng_l, rings_l, 3, 1.0, 0.0, kl, None), None, _native.ptr(yl),
                                               eng_l._stream()) == 2
    torch.cuda.synchronize()
    assert bool((yl == 7.0).all())


def _basis(mesh_np, order):
    return tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(1, order))


class _Spy:
    """Counts the calls of the library's entry points that go through an engine."""

    NAMES = ("tfem_p1_rings_field", "tfem_p1_apply_rings_field", "tfem_p1_field_adjoint", "tfem_p1_rings_coef",
             "tfem_p1_apply_rings_coef", "tfem_p1_assemble_rings", "tfem_p1_apply_rings", "tfem_reduce_scatter_bilinear",
             "tfem_p1_assemble_tiles", "tfem_tri_bilinear_csr", "tfem_source_eval", "tfem_csr_spmv")

    def __init__(self, monkeypatch, lib):
        self.calls = {name: 0 for name in self.NAMES}
        for name in self.NAMES:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, inner):
        def call(*args):
            self.calls[name] += 1
            return inner(*args)

        return call


def _form(alpha, beta, kq, cq):
    """alpha * kq * stiffness + beta * cq * mass; kq / cq: a field, a tensor or None."""
    def bilinear(basis):
        out = None
        if alpha != 0.0:
            s = basis.v_grad @ basis.v_grad.mT
            s = kq * s if kq is not None else s
            out = s if alpha == 1.0 else alpha * s
        if beta != 0.0:
            m = basis.v @ basis.v.mT
            m = cq * m if cq is not None else m
            m = m if beta == 1.0 else beta * m
            out = m if out is None else out + m
        return out

    return bilinear


PUBLIC_CASES = [("p1_square_n8.npz", torch.float64), ("p1_square_n6_float32.npz", torch.float32),
                ("square_chunked", torch.float64), ("square_multi_tile", torch.float32),
                ("delaunay_15_slots", torch.float64), ("holes", torch.float64), ("rotated_shuffled", torch.float64),
                ("shuffled", torch.float64)]


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("mesh,dtype", PUBLIC_CASES)
def test_public_layouts_operator_and_the_materialised_path(mesh, dtype, order, monkeypatch):
    """csr / dense / operator / matrix_free against the reference and against the materialised path of
    the same callable under TFEM_KERNEL=gather; launch counts: the store launch once, no generic
    kernels, no assembly behind the operator."""
    mesh_np = _mesh(mesh)
    torch.set_default_dtype(dtype)
    npd = _np_dtype(dtype)

    def env():
        if mesh == "shuffled":
            monkeypatch.setenv("TFEM_RENUMBER", "1")

    env()
    n = mesh_np["vertices"].shape[0]
    u_np = np.random.default_rng(2).standard_normal(n).astype(npd).astype(np.float64)
    for name in ("kappa", "kappa_c"):
        alpha, beta, has_k, has_c = FORMS[name]
        kv, cv = _data(mesh_np, order, has_k, 41, dtype), _data(mesh_np, order, has_c, 42, dtype, per_element=True)
        parts = fref.reference_parts(mesh_np, order, alpha, beta, kv, cv, npd)
        rowptr, colind, want, tol = parts[:4]
        want_dense, tol_dense = fref.dense(rowptr, colind, want, n), fref.dense(rowptr, colind, tol, n)
        want_y, tol_y = fref.apply_reference(parts, u_np)
        tol_d = fref.apply_reference(parts, np.ones(n))[1]
        what = f"{mesh} {npd.__name__} order {order} {name}"
        basis = _basis(mesh_np, order)
        engine = basis._engine
        assert engine.dtype == dtype and engine.renumbered == (mesh == "shuffled")
        stored = engine.field_refusal(beta, "store") is None
        assert stored or (mesh == "delaunay_15_slots" and beta != 0.0)
        kq = basis.coefficient(torch.tensor(kv, dtype=dtype)) if has_k else None
        cq = basis.coefficient(torch.tensor(cv[:, 0], dtype=dtype)) if has_c else None  # (E,): one value per element
        a = _form(alpha, beta, kq, cq)
        spy = _Spy(monkeypatch, engine.lib)
        K = basis.integrate_bilinear_form(a, layout="csr")
        assert K.dtype == dtype
        assert spy.calls["tfem_p1_rings_field"] == int(stored) and spy.calls["tfem_reduce_scatter_bilinear"] == int(not stored)
        _record(fref.check(_host(K.to_dense()), want_dense, tol_dense, f"{what}: csr"))
        D = basis.integrate_bilinear_form(a, layout="dense")
        assert isinstance(D, torch.Tensor) and D.shape == (n, n)
        _record(fref.check(_host(D), want_dense, tol_dense, f"{what}: dense"))
        before = dict(spy.calls)
        u = torch.tensor(u_np, dtype=dtype)
        for layout in ("operator", "matrix_free"):
            op = basis.integrate_bilinear_form(a, layout=layout)
            assert op.matrix_free is True and "matrix-free, coefficient data" in repr(op) and op.dtype == dtype
            _record(fref.check(_host(op.matvec(u)), want_y, tol_y, f"{what}: {layout} matvec"))
            _record(fref.check(_host(op.diagonal()), np.diag(want_dense), tol_d, f"{what}: {layout} diagonal"))
            assert (op @ u.reshape(-1, 1)).shape == (n, 1)
            assert op._csr is None
        # nothing was assembled for them, and no integrand was reduced
        assert spy.calls["tfem_p1_apply_rings_field"] == before["tfem_p1_apply_rings_field"] + 6
        for quiet in ("tfem_p1_rings_field", "tfem_reduce_scatter_bilinear", "tfem_p1_assemble_rings", "tfem_csr_spmv",
                      "tfem_p1_rings_coef", "tfem_p1_apply_rings_coef"):
            assert spy.calls[quiet] == before[quiet], quiet
        # to_csr(): by the store launch
        _record(fref.check(_host(op.to_csr().to_dense()), want_dense, tol_dense, f"{what}: to_csr"))
        assert spy.calls["tfem_p1_rings_field"] == before["tfem_p1_rings_field"] + int(stored)
        monkeypatch.undo()
        env()
        # the materialised path of the same callable
        monkeypatch.setenv("TFEM_KERNEL", "gather")
        basis_t = _basis(mesh_np, order)
        kq_t = basis_t.coefficient(torch.tensor(kv, dtype=dtype)) if has_k else None
        cq_t = basis_t.coefficient(torch.tensor(cv[:, 0], dtype=dtype)) if has_c else None
        a_t = _form(alpha, beta, kq_t, cq_t)
        spy_t = _Spy(monkeypatch, basis_t._engine.lib)
        Kt = basis_t.integrate_bilinear_form(a_t, layout="csr")
        assert spy_t.calls["tfem_p1_rings_field"] == 0 and spy_t.calls["tfem_reduce_scatter_bilinear"] == 1
        _record(fref.check(_host(Kt.to_dense()), want_dense, tol_dense, f"{what}: materialised path"))
        op_t = basis_t.integrate_bilinear_form(a_t, layout="operator")
        assert op_t.matrix_free is False
        _record(fref.check(_host(op_t.matvec(u)), want_y, tol_y, f"{what}: materialised path matvec"))
        with pytest.raises(NotImplementedError, match="TFEM_KERNEL=gather"):
            basis_t.integrate_bilinear_form(a_t, layout="matrix_free")
        monkeypatch.undo()
        env()


def test_a_program_on_the_other_term_becomes_values_once(monkeypatch):
    mesh_np = _mesh("square_chunked")
    order, n = 3, mesh_np["vertices"].shape[0]
    basis = _basis(mesh_np, order)
    kv = fref.data(mesh_np, order, 5)
    kq = basis.coefficient(torch.tensor(kv))

    def a(b):
        x, _ = torch.split(b.integration_points, 1, dim=-1)
        return kq * (b.v_grad @ b.v_grad.mT) + torch.exp(-x) * (b.v @ b.v.mT)

    spy = _Spy(monkeypatch, basis._engine.lib)
    op = basis.integrate_bilinear_form(a, layout="matrix_free")
    u = torch.tensor(np.random.default_rng(3).standard_normal(n))
    y = op.matvec(u)
    assert spy.calls["tfem_source_eval"] == 1 and spy.calls["tfem_p1_apply_rings_field"] == 1
    tris = mesh_np["triangles"].astype(np.int64)
    from oracle import assembly_oracle as orc

    points = orc.geometry(mesh_np["vertices"][tris], 1, order)["integration_points"]
    cv = np.exp(-points[..., 0]).reshape(tris.shape[0], -1)
    parts = fref.reference_parts(mesh_np, order, 1.0, 1.0, kv, cv)
    want_y, tol_y = fref.apply_reference(parts, _host(u))
    # (exp on the device against numpy's: an ulp of the values, four orders below the bound)
    _record(fref.check(_host(y), want_y, tol_y, "kappa data + c program: matvec"))


def test_history_on_the_values_stored_layouts_refuse_and_p2_falls_back(monkeypatch):
    mesh_np = _mesh("square_chunked")
    basis = _basis(mesh_np, 3)
    values = torch.tensor(fref.data(mesh_np, 3, 6)).requires_grad_(True)
    a = _form(1.0, 0.0, basis.coefficient(values), None)
    for layout in ("csr", "dense", None):
        with pytest.raises(NotImplementedError, match="carries autograd history"):
            basis.integrate_bilinear_form(a, layout=layout)
    with torch.no_grad():
        assert basis.integrate_bilinear_form(a, layout="csr").shape[0] == basis._engine.n_dofs
    # P2: no data launch; stored layouts and "operator" materialise, "matrix_free" says why
    p2 = tf().Basis(tf().MeshTri(triangulation=mesh_np), tf().ElementTri(2, 3))
    kq = p2.coefficient(torch.tensor(fref.data(mesh_np, 3, 7)))
    a2 = _form(1.0, 0.0, kq, None)
    spy = _Spy(monkeypatch, p2._engine.lib)
    K = p2.integrate_bilinear_form(a2, layout="csr")
    assert spy.calls["tfem_p1_rings_field"] == 0 and spy.calls["tfem_reduce_scatter_bilinear"] == 1
    assert K.shape[0] == p2._engine.n_dofs
    assert p2.integrate_bilinear_form(a2, layout="operator").matrix_free is False
    with pytest.raises(NotImplementedError, match="coefficient"):
        p2.integrate_bilinear_form(a2, layout="matrix_free")


@pytest.mark.parametrize("mesh,dtype,per_element", [
    ("square_chunked", torch.float64, False), ("rotated_shuffled", torch.float64, True),
    ("p1_square_n5_clockwise.npz", torch.float64, False), ("delaunay_15_slots", torch.float64, False),
    ("square_multi_tile", torch.float32, False), ("shuffled", torch.float64, True)])
def test_gradients_in_kappa_c_and_u(mesh, dtype, per_element, monkeypatch):
    """(op.matvec(u) * g).sum().backward() against the numpy reference, for a vector and a (N, 3) block."""
    if mesh == "shuffled":
        monkeypatch.setenv("TFEM_RENUMBER", "1")
    torch.set_default_dtype(dtype)
    npd = _np_dtype(dtype)
    order, alpha, beta = 3, 0.5, 2.0
    mesh_np = _mesh(mesh)
    n = mesh_np["vertices"].shape[0]
    basis = _basis(mesh_np, order)
    assert basis._engine.renumbered == (mesh == "shuffled")
    kv, cv = fref.data(mesh_np, order, 51, npd, per_element), fref.data(mesh_np, order, 52, npd)
    rng = np.random.default_rng(8)
    for cols in (1, 3):
        shape = (n,) if cols == 1 else (n, cols)
        u_np, g_np = (rng.standard_normal(shape).astype(npd).astype(np.float64) for _ in range(2))
        kt = torch.tensor(kv[:, 0] if per_element else kv, dtype=dtype).requires_grad_(True)
        ct = torch.tensor(cv, dtype=dtype).reshape(-1, cv.shape[1], 1, 1).requires_grad_(True)
        op = basis.integrate_bilinear_form(_form(alpha, beta, basis.coefficient(kt), basis.coefficient(ct)),
                                           layout="matrix_free")
        u = torch.tensor(u_np, dtype=dtype).requires_grad_(True)
        g = torch.tensor(g_np, dtype=dtype)
        spy = _Spy(monkeypatch, basis._engine.lib)
        (op.matvec(u) * g).sum().backward()
        assert spy.calls["tfem_p1_field_adjoint"] == 1
        monkeypatch.undo()
        if mesh == "shuffled":
            monkeypatch.setenv("TFEM_RENUMBER", "1")
        want_k, want_c, tol_k, tol_c = fref.adjoint_reference(mesh_np, order, alpha, beta, g_np, u_np, npd)
        what = f"{mesh} {npd.__name__} {cols} column(s)"
        assert kt.grad.shape == kt.shape and ct.grad.shape == ct.shape
        if per_element:  # one value per element receives the sum over q
            want_k = want_k.sum(1)
            tol_k = fref.BASE_TOL[np.dtype(npd)] * np.abs(want_k).max()
        _record(fref.check(_host(kt.grad).reshape(want_k.shape), want_k, tol_k, f"{what}: d / d kappa"))
        _record(fref.check(_host(ct.grad).reshape(want_c.shape), want_c, tol_c, f"{what}: d / d c"))
        # d / d u = K^T g = K g
        parts = fref.reference_parts(mesh_np, order, alpha, beta, kv, cv, npd)
        for j in range(cols):
            col = (lambda t: t if cols == 1 else t[:, j])
            want_u, tol_u = fref.apply_reference(parts, col(g_np))
            _record(fref.check(col(_host(u.grad)), want_u, tol_u, f"{what}: d / d u, column {j}"))
    # values without grad: the plain path, no adjoint
    op = basis.integrate_bilinear_form(_form(alpha, beta, basis.coefficient(kt.detach()), None), layout="matrix_free")
    assert not op.matvec(torch.ones(n, dtype=dtype)).requires_grad


def test_fused_cg_equals_cg_on_the_assembled_operator(monkeypatch):
    """Order 4, smooth positive data (kappa = 1 + u_h^2 of a smooth u_h at the integration points, c per
    element): the fused loop on the matrix-free operator against CG on to_csr(), the bounds of
    tests/test_hip_fused_cg.py (residual <= rtol, solutions equal to 1e-9 of the largest entry)."""
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(40, 0.25, 1)
    order = 4
    basis = _basis(mesh_np, order)
    n = basis._engine.n_dofs
    x, y = torch.split(basis.integration_points, 1, dim=-1)
    kq = basis.coefficient(1.0 + (torch.sin(3.0 * x) * torch.cos(2.0 * y)) ** 2)
    cq = basis.coefficient(torch.tensor(1.0 + np.asarray(mesh_np["vertices"])[mesh_np["triangles"]].mean(1)[:, 0]))
    a = _form(1.0, 1.0, kq, cq)
    f = basis.integrate_linear_form(lambda b: torch.sin(np.pi * torch.split(b.integration_points, 1, dim=-1)[0]) * b.v)
    free = basis._basis_parameters["inner_dofs"]
    op = basis.integrate_bilinear_form(a, layout="matrix_free")
    spy = _Spy(monkeypatch, basis._engine.lib)
    x_f, it_f, res_f = op.solve_cg(f, free=free, rtol=1e-12, loop="fused")
    assert res_f <= 1e-12 and 0 < it_f < 10 * n
    assert spy.calls["tfem_p1_apply_rings_field"] >= it_f + 2 and spy.calls["tfem_p1_rings_field"] == 0
    assert spy.calls["tfem_csr_spmv"] == 0 and op._csr is None
    x_t, it_t, res_t = op.solve_cg(f, free=free, rtol=1e-12, loop="torch")
    x_c, it_c, res_c = op.to_csr().solve_cg(f, free=free, rtol=1e-12)
    assert res_t <= 1e-12 and res_c <= 1e-12
    scale = float(x_c.abs().max())
    assert float((x_f - x_c).abs().max()) <= 1e-9 * scale and float((x_t - x_c).abs().max()) <= 1e-9 * scale
    # a block of right-hand sides: column by column through the same launch
    B = torch.cat([f.reshape(-1, 1), 2.0 * f.reshape(-1, 1)], 1)
    X, its, res = op.solve_cg_multi(B, free=free, rtol=1e-12)
    assert float(res.max()) <= 1e-12
    assert float((X[:, 0] - x_c.reshape(-1)).abs().max()) <= 1e-9 * scale
    sol = basis.solve(op, basis.solution_tensor().to(f.device, f.dtype), f)
    assert float((sol.reshape(-1) - x_c.reshape(-1)).abs().max()) <= 1e-9 * scale


def test_example_runs():
    """examples/poisson_coefficient_field.py at a small size: exit code 0, its own assertions are the
    checks (Picard iteration converges, nothing is assembled, the gradient agrees with a difference
    quotient)."""
    done = subprocess.run([sys.executable, os.path.join(REPO, "examples", "poisson_coefficient_field.py"), "24"],
                          capture_output=True, text=True, timeout=600, cwd=REPO)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "Picard iterations" in done.stdout and "assembled: 0" in done.stdout
