"""Geometric multigrid for P1 forms: a hierarchy of red refinements of a coarse triangulation, a
V-cycle on it and conjugate gradients preconditioned by that cycle.

The spaces are nested, so the form re-discretised on a coarser mesh IS the Galerkin operator
P^T K P of the finer one (for coefficients that the quadrature integrates exactly; otherwise it
differs by the quadrature error, which a preconditioner does not mind): no sparse triple product.
Every level has its own ``Basis`` and its own matrix-free operator (``layout="operator"``), and the
transfers are the parent table of ``meshgen.refine_uniform`` and its transpose.

    l = 0:  z[free] = K0[free, free]^-1 r[free], 0 elsewhere          (dense Cholesky, factored once)
    else:   x = w r;  (nu - 1) x  x += w (r - K x)                    w = omega * m / diag K
            x += m P vcycle_{l-1}( m_c P^T( m (r - K x) ) )
            nu x  x += w (r - K x)

with m the 0/1 mask of the level's interior DoFs.  The cycle is a symmetric positive definite
operator (the post-smoothing is the adjoint of the pre-smoothing), so it may precondition CG.

The cycle is written once (``_Hierarchy._cycle``) over a list of levels, a list of their (x, K x, r)
buffers and a list of their applies.  A level makes the three vector launches of libtfem_hip itself:
its sweep, the restriction of its residual to the level below and the prolongation from there.  An
h-level (``_Level``) runs them on single vectors or on (n_l, k) blocks of right-hand sides
(``vcycle_multi``, ``solve_multi``); all of them are csrc/tfem_mg.hip.  ``P2Multigrid`` puts a P2
level (``_P2Level``) on the finest mesh of such a hierarchy: P1 is a subspace of P2 on one mesh, the
two transfers of that step are the other transfer kind of the same kernels (``tfem_mg_p2_*``), and
below it the same cycle goes on through the P1 levels.

The conjugate-gradient recurrence around the cycle runs on the device as well (``_fused_cycle_pcg``
over csrc/tfem_pcg.hip, the default of ``solve`` / ``solve_multi`` on a HIP device); ``_cycle_pcg``
and the body of ``solve_multi`` are the same recurrence in torch operations (``loop="torch"``).
"""

from __future__ import annotations

from collections.abc import Mapping

import numpy as np
import torch

from . import _native, meshgen
from .basis import Basis, forms
from .element import ElementTri
from .mesh import MeshTri
from .sparse import FormOperator, _cg_loop, _into, _is_block

__all__ = ["GeometricMultigrid", "P2Multigrid"]

_MESH_KEYS = ("vertices", "vertex_markers", "triangles", "edges", "edge_markers", "neighbors")
_ptr = _native.ptr


def _identity(v):
    return v


def transpose_parents(parents, n_coarse):
    """(ptr (n_coarse + 1,), idx (2 n_fine,)) int32: row v lists the fine vertices that name the
    coarse vertex v in ``parents`` (n_fine, 2), ascending; a kept vertex names itself twice and is
    listed twice.  With the weight 0.5 on every entry this is P^T of the P1 prolongation."""
    parents = np.asarray(parents)
    rows = parents.reshape(-1).astype(np.int64)
    fine = np.repeat(np.arange(parents.shape[0], dtype=np.int64), 2)
    order = np.argsort(rows, kind="stable")  # `fine` ascends, a stable sort keeps it ascending per row
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_coarse))])
    return ptr.astype(np.int32), fine[order].astype(np.int32)


def transpose_edges(edge_vertices, n_vertices):
    """(ptr (n_vertices + 1,), idx (2 n_edges,)) int32: row v lists the edge DoFs n_vertices + j of
    the edges j with an endpoint v in ``edge_vertices`` (n_edges, 2), ascending.  With the weight 0.5
    on every entry, plus the identity on the vertices, this is P^T of the step from P1 to P2 on one
    mesh."""
    ptr, idx = transpose_parents(edge_vertices, n_vertices)
    return ptr, (idx + np.int32(n_vertices)).astype(np.int32)


def _cycle_pcg(apply, cycle, mask, rhs, x0, rtol, maxiter):
    """Conjugate gradients on K x = rhs preconditioned by ``cycle``, the loop of ``solve``: ``apply(u,
    out)`` writes K u, ``cycle(r)`` returns the buffer that holds the V-cycle of r, ``mask`` is the
    0/1 vector of the free DoFs (None: all), every vector in one numbering.  ``x0`` (None: zero) is
    copied.  Returns (x, iterations, |r| / |m rhs|), the residual checked every iteration."""
    x = torch.zeros_like(rhs) if x0 is None else x0.clone()
    ap = torch.empty_like(rhs)
    if x0 is None:
        r = rhs.clone()
    else:
        apply(x, ap)
        r = rhs - ap
    if mask is not None:
        r *= mask
    b_norm = torch.linalg.vector_norm(rhs if mask is None else mask * rhs).clamp_min(torch.finfo(rhs.dtype).tiny)
    it, res = 0, float(torch.linalg.vector_norm(r) / b_norm)
    if res > rtol and maxiter > 0:
        p = cycle(r).clone()
        rz = torch.dot(r, p)
        while True:
            apply(p, ap)
            if mask is not None:
                ap *= mask
            alpha = rz / torch.dot(p, ap)
            x.add_(alpha * p)
            r.sub_(alpha * ap)
            it += 1
            res = float(torch.linalg.vector_norm(r) / b_norm)
            if res <= rtol or it >= maxiter:
                break
            z = cycle(r)
            rz_new = torch.dot(r, z)
            p.mul_(rz_new / rz).add_(z)
            rz = rz_new
    return x, it, res


#: how the fused loop reads |r|^2 every iteration: "drain" is one blocking copy after the update;
#: "overlap" copies it asynchronously into pinned memory and waits only after the next cycle, rz,
#: direction, apply and dot have been enqueued.  None: by the width of the block.  On an MI355X
#: (profiles/mg_fused.log, 986,049 DoFs) the overlapped read saves 0.5 - 1.8 ms of a 10 - 15 ms
#: solve on one and two columns, where the queue runs empty while the host decides; at four
#: columns the two are level and at eight the draining read is 1 % ahead on the P2 hierarchy,
#: because the launches are then long enough to keep the queue filled either way.
_PCG_READ = None
_PCG_OVERLAP_WIDTHS = 2  # the widest block that reads overlapped


def _fused_cycle_pcg(lib, apply, cycle, mask, rhs, R, Z, P, AP, x0, rtol, maxiter):
    """The recurrences of ``_cycle_pcg`` (rhs of shape (n,)) and of ``solve_multi`` (rhs of shape
    (n, k)) with the vector part in libtfem_hip (csrc/tfem_pcg.hip).  ``R`` is the residual buffer
    the cycle reads and ``Z`` the buffer it leaves z in (``cycle()`` takes no argument and copies
    nothing), ``P`` and ``AP`` the kept direction and its image, all shaped like rhs; ``mask`` is the
    (n,) vector whose zeros mark the held DoFs (None: none is held).  Per iteration: ``apply(P,
    AP)``, tfem_cg_dot, tfem_pcg_update, the check, ``cycle()``, tfem_pcg_rz, tfem_pcg_direction --
    alpha, beta and the dot products stay on the device, and the only torch operations are the sum
    of the G partial sums of |r_j|^2 and its copy to the host (in the form ``_PCG_READ`` names; the
    overlapped form has run one cycle, rz, direction, apply and dot more than it needed when the
    check ends the loop before ``maxiter``; they write neither x nor r).
    Returns (X shaped like rhs, iterations (k,) int64, relative residuals (k,) float64), the last
    two on the host."""
    from .sparse import cg_workspace

    read = _PCG_READ
    if read not in (None, "drain", "overlap"):
        raise ValueError(f"_PCG_READ must be None, 'drain' or 'overlap', not {read!r}")
    n = rhs.shape[0]
    k = 1 if rhs.dim() == 1 else rhs.shape[1]
    if read is None:
        read = "overlap" if k <= _PCG_OVERLAP_WIDTHS else "drain"
    device, dtype = rhs.device, rhs.dtype
    as_block = lambda t: t.view(n, k)  # noqa: E731
    if x0 is None:
        X = torch.zeros_like(R)
        R.copy_(rhs)
    else:
        X = x0.clone(memory_format=torch.contiguous_format)
        P.copy_(X)
        apply(P, AP)
        torch.sub(rhs, AP, out=R)
    if mask is None:
        b_norm = torch.linalg.vector_norm(as_block(rhs), dim=0)
        mask = torch.ones(n, dtype=dtype, device=device)  # the launches take a mask: nothing is held
    else:
        as_block(R).mul_(mask.view(n, 1))
        b_norm = torch.linalg.vector_norm(as_block(rhs) * mask.view(n, 1), dim=0)
    b_norm = b_norm.clamp_min(torch.finfo(dtype).tiny)
    res = (torch.linalg.vector_norm(as_block(R), dim=0) / b_norm).double().cpu()
    b_norm = b_norm.double().cpu()
    running = res > rtol  # (k,) on the host: it decides the loop
    its = torch.zeros(k, dtype=torch.int64, device="cpu")
    if n == 0 or maxiter <= 0 or not bool(running.any()):
        return X, its, res
    ws = cg_workspace(n, k, device)
    flags_host = running.to(torch.int32)
    flags = flags_host.to(device)
    stream = _native.current_stream(device)
    size = (rhs.element_size(), n, k)
    x_, r_, z_, p_, ap_, m_, f_, w_ = (_ptr(t) for t in (X, R, Z, P, AP, mask, flags, ws))
    dot, update, rz, direction = lib.tfem_cg_dot, lib.tfem_pcg_update, lib.tfem_pcg_rz, lib.tfem_pcg_direction
    dot_args = (p_, ap_, m_, *size, w_, stream)
    cycle()
    _native.check(lib.tfem_pcg_start(r_, z_, m_, p_, *size, w_, stream))
    if not bool(running.all()):
        as_block(P).mul_(flags)  # once: the direction of a column that starts converged is zero
    rr_partials = (ws[2], ws[4])  # the r.r buffers of the two parities
    overlap = read == "overlap"
    if overlap:
        rr = torch.empty(k, dtype=torch.float64, device=device)
        rr_host = torch.empty(k, dtype=torch.float64, device="cpu").pin_memory()
        flags_host = flags_host.pin_memory()
        arrived = torch.cuda.Event()
    apply(P, AP)
    status = dot(*dot_args)
    it = 0
    while True:
        status = status or update(x_, r_, p_, ap_, m_, f_, *size, it, w_, stream)
        if status:
            _native.check(status)
        partials = rr_partials[it & 1]  # (G, k): |r_j|^2 after this update
        if overlap:
            torch.sum(partials, dim=0, out=rr)
            rr_host.copy_(rr, non_blocking=True)
            arrived.record()
            if it + 1 < maxiter:  # ahead of the decision: none of these writes x or r
                cycle()
                status = (rz(r_, z_, m_, *size, it, w_, stream) or direction(p_, z_, m_, f_, *size, it, w_, stream))
                apply(P, AP)
                status = status or dot(*dot_args)
            arrived.synchronize()
            rr_now = rr_host
        else:
            rr_now = partials.sum(0).cpu()  # the host read of the iteration
        it += 1
        res = torch.where(running, rr_now.sqrt() / b_norm, res)  # a frozen column reports what froze it
        its[running] = it
        still = running & (res > rtol)
        if it >= maxiter or not bool(still.any()):
            break
        if not bool((still == running).all()):
            running = still
            flags_host.copy_(running)
            flags.copy_(flags_host, non_blocking=True)  # before the next update: the column's x and r stay
        if not overlap:
            cycle()
            status = (rz(r_, z_, m_, *size, it - 1, w_, stream)
                      or direction(p_, z_, m_, f_, *size, it - 1, w_, stream))
            apply(P, AP)
            status = status or dot(*dot_args)
    if status:
        _native.check(status)
    return X, its, res


class _Level:
    """One mesh of the hierarchy, a P1 level: what the cycle needs of it (``free``, ``mask``, ``w``,
    the single-vector buffers ``x``, ``ax``, ``r``: set by ``_Hierarchy._prepare_level``) and the
    three vector launches of the cycle on it.  Each launch takes the level's (x, K x, r) buffers --
    and those of the level below for a transfer -- and their width ``k``: None for vectors (n_l,),
    the number of columns for (n_l, k) blocks (k = 1 included), which go through the block kernels."""

    order = 1
    #: True: the level runs in the engine's numbering and vectors cross at the hierarchy's boundary
    crossing = False

    def __init__(self, triangulation, basis, op):
        self.triangulation = triangulation
        self.basis = basis
        self.op = op
        self.engine = basis._engine
        self.n = int(op.shape[0])

    def set_coarser(self, coarse, parents, device):
        """The transfers to and from ``coarse``, the level below: the parent table of the refinement
        (P) and its transpose (P^T)."""
        ptr, idx = transpose_parents(parents, coarse.n)
        self.coarse = coarse
        self.parents = torch.as_tensor(np.ascontiguousarray(parents, dtype=np.int32), device=device)
        self.pt_ptr = torch.as_tensor(ptr, device=device)
        self.pt_idx = torch.as_tensor(idx, device=device)

    def _launch(self, name, k, head, tail):
        """The entry point ``name`` on vectors (``k`` None) or ``name + "_multi"`` on (n_l, k) blocks,
        whose arguments are the single ones with n_vec = k between ``head`` and ``tail``."""
        if k is None:
            status = getattr(self.lib, name)(*head, *tail)
        else:
            status = getattr(self.lib, name + "_multi")(*head, k, *tail)
        if status:
            _native.check(status)

    def smooth(self, buffers, k, first, stream):
        """x = w r (``first``) or x += w (r - K x)."""
        x, ax, r = buffers
        self._launch("tfem_mg_smooth", k,
                     (_ptr(x), _ptr(r), None if first else _ptr(ax), _ptr(self.w), self.real_bytes, self.n),
                     (1 if first else 0, stream))

    def restrict_residual(self, buffers, coarser, k, stream):
        """r of the level below = m_c P^T( m (r - K x) )."""
        coarse, (_, ax, r), (_, _, coarse_r) = self.coarse, buffers, coarser
        self._launch("tfem_mg_restrict_residual", k,
                     (_ptr(self.pt_ptr), _ptr(self.pt_idx), _ptr(coarse.mask), _ptr(self.mask), _ptr(r), _ptr(ax),
                      _ptr(coarse_r), self.real_bytes, coarse.n, self.n), (stream,))

    def prolong_add(self, buffers, coarser, k, stream):
        """x += m P (x of the level below)."""
        coarse, (x, _, _), (coarse_x, _, _) = self.coarse, buffers, coarser
        self._launch("tfem_mg_prolong_add", k,
                     (_ptr(self.parents), _ptr(self.mask), _ptr(coarse_x), _ptr(x), self.real_bytes, self.n, coarse.n),
                     (stream,))

    def __repr__(self):
        extra = ", renumbered by the engine" if self.engine.renumbered else ""
        return f"<multigrid level: {self.n} DoFs, {self.op}{extra}>"


class _P2Level(_Level):
    """The P2 space on the mesh of the P1 level below it.  P is the identity on the vertex DoFs and
    0.5 / 0.5 on an edge DoF (the P2 numbering is "vertices, then edges"); the two transfers are its
    own (``tfem_mg_p2_*``, the P2 kind of the transfers of csrc/tfem_mg.hip) on one vector or on a
    block, the sweep is the P1 levels'.

    A matrix-free P2 operator is applied in the ENGINE's numbering (the engine renumbers the edge
    DoFs of a basis from 50,000 DoFs on; the vertex ids stay those of the P1 level): the level is
    then ``crossing``, and its tables, mask and weights are built in that numbering."""

    order = 2

    def __init__(self, triangulation, basis, op):
        super().__init__(triangulation, basis, op)
        self.n_v = int(np.asarray(triangulation["vertices"]).shape[0])
        self.crossing = bool(op.matrix_free and self.engine.renumbered)

    def set_coarser(self, coarse, device):
        """The transfers to and from ``coarse``, the P1 level of the same mesh: the edge table (P) and
        its transpose (P^T), edge DoF n_v + j of a crossing level being the caller's _perm[n_v + j]."""
        n_v = self.n_v
        edges = np.asarray(self.triangulation["edges"]).reshape(-1, 2)
        if self.n != n_v + edges.shape[0]:
            raise ValueError(f"P2Multigrid: {self.n} P2 DoFs on a mesh of {n_v} vertices and {edges.shape[0]} edges")
        if self.crossing:
            perm = self.engine._perm.cpu().numpy()
            if not (perm[:n_v] == np.arange(n_v)).all():
                raise NotImplementedError("P2Multigrid: an engine that renumbers the vertex DoFs of a P2 basis")
            edges = edges[perm[n_v:] - n_v]
        ptr, idx = transpose_edges(edges, n_v)
        self.coarse = coarse
        self.edge_vertices = torch.as_tensor(np.ascontiguousarray(edges, dtype=np.int32), device=device)
        self.pt_ptr = torch.as_tensor(ptr, device=device)
        self.pt_idx = torch.as_tensor(idx, device=device)

    def restrict_residual(self, buffers, coarser, k, stream):
        (_, ax, r), (_, _, coarse_r) = buffers, coarser
        self._launch("tfem_mg_p2_restrict_residual", k,
                     (_ptr(self.pt_ptr), _ptr(self.pt_idx), _ptr(self.coarse.mask), _ptr(self.mask), _ptr(r), _ptr(ax),
                      _ptr(coarse_r), self.real_bytes, self.n_v, self.n), (stream,))

    def prolong_add(self, buffers, coarser, k, stream):
        (x, _, _), (coarse_x, _, _) = buffers, coarser
        self._launch("tfem_mg_p2_prolong_add", k,
                     (_ptr(self.edge_vertices), _ptr(self.mask), _ptr(coarse_x), _ptr(x), self.real_bytes, self.n_v,
                      self.n), (stream,))


def _build_level(name, kind, mesh, element, bilinear, layouts):
    """The level of the class ``kind`` on ``mesh``: its ``Basis`` and the operator of ``bilinear`` in
    the first of ``layouts`` that the basis grants.  ``name``: the hierarchy's, for the messages."""
    basis = Basis(MeshTri(triangulation=mesh), element)
    engine = basis._engine
    if engine.n_fractures > 0 or engine.poly_order != kind.order:
        raise NotImplementedError(f"{name}: a P{kind.order} basis on one triangulation is needed")
    try:
        expr = forms.trace(bilinear, basis, (), {})
    except ValueError as err:
        if str(err).startswith("coefficient:"):
            raise NotImplementedError(f"{name}: coefficient data (basis.coefficient) has the shape of ONE mesh; "
                                      "write the coefficient as an expression of the integration points") from err
        raise
    if isinstance(expr, forms.BilinearExpr) and expr.has_coefficients and expr.has_data:
        raise NotImplementedError(f"{name}: coefficient data (basis.coefficient) has the shape of ONE mesh; write "
                                  "the coefficient as an expression of the integration points")
    for layout in layouts[:-1]:
        try:
            op = basis._bilinear_of(expr, layout)
            break
        except NotImplementedError:
            pass
    else:
        op = basis._bilinear_of(expr, layouts[-1])
    if not isinstance(op, FormOperator):
        raise TypeError(f"{name}: the bilinear form did not give an operator")
    return kind(mesh, basis, op)


class _Hierarchy:
    """What ``GeometricMultigrid`` and ``P2Multigrid`` share: the preparation of a level's vectors,
    its apply, THE cycle, ``vcycle`` / ``solve`` on one vector and ``vcycle_multi`` / ``solve_multi``
    on a block.  A subclass sets ``levels`` (coarsest first), ``nu``, ``omega``, ``dirichlet``,
    ``device``, ``dtype``, ``_buffers`` (per level the single-vector (x, ax, r)), ``_own`` (the levels
    whose applies and block buffers it keeps itself), ``_applies`` (stream -> the prepared applies of
    ``_own``) and ``_blocks`` (k -> the block buffers of ``_own``; insertion order = age of last
    use)."""

    #: how the refusal of a block (N, k) where one vector is expected ends
    _BLOCKS = "blocks: vcycle_multi, solve_multi"

    #: ``vcycle_multi`` keeps the block buffers (x, K x, r per level, (n_l, k) each) of this many
    #: widths k, the most recently used ones; an older width is dropped with the prepared launches
    #: that point into its buffers and allocated again when it comes back.
    BLOCK_WIDTHS_KEPT = 2

    #: the direction and its image of the fused loop of ``solve``, allocated by its first use
    _directions = None

    # ------------------------------------------------------------------ set-up
    def _prepare_level(self, level, inward):
        """Mask, smoothing weights and buffers of ``level`` in the numbering it runs in; ``inward``
        takes a vector of the caller's numbering there."""
        dev, dtype, n = self.device, self.dtype, level.n
        level.lib = _native.load()
        level.real_bytes = torch.empty((), dtype=dtype).element_size()
        diag = inward(level.op.diagonal().to(dev, dtype).reshape(-1))
        if self.dirichlet:
            level.free = level.basis._basis_parameters["inner_dofs"].to(dev).reshape(-1).long()
            mask = torch.zeros(n, dtype=dtype, device=dev)
            mask[level.free] = 1
            level.mask = inward(mask).contiguous()
            w = level.mask / torch.where(diag != 0, diag, torch.ones_like(diag))
        else:
            level.free, level.mask = None, None
            w = 1.0 / diag
        level.w = (self.omega * w).contiguous()
        level.x, level.ax, level.r = (torch.zeros(n, dtype=dtype, device=dev) for _ in range(3))

    def _apply_of(self, level):
        """``apply(u, out)``: out = K u on the level's buffers, in the numbering the level runs in."""
        op = level.op
        if op.matrix_free and (not level.engine.renumbered or level.crossing):
            return op._rows_into()
        if not op.matrix_free:
            csr = op.to_csr().to(self.device)
            if csr.perm is None:
                return _into(csr._prepared_spmv)

        def through_matvec(u, out):
            out.copy_(op.matvec(u))

        return through_matvec

    def _level_applies(self):
        """The applies of ``levels`` prepared for the current stream (those of ``_own`` are kept here)."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        applies = self._applies.get(key)
        if applies is None:
            applies = self._applies[key] = [self._apply_of(level) for level in self._own]
        return applies

    # ------------------------------------------------------------------ the cycle
    def _cycle(self, l, buffers, k, applies, stream):
        """r of level l -> x of level l on ``buffers``, per level (x, K x, r): vectors (k None) or
        (n_l, k) blocks.  The coarsest level is one dense product."""
        level, mine = self.levels[l], buffers[l]
        x, ax, r = mine
        if l == 0:
            if k is None:
                torch.mv(level.inverse, r, out=x)
            else:
                torch.mm(level.inverse, r, out=x)
            return
        coarser, apply = buffers[l - 1], applies[l]
        level.smooth(mine, k, True, stream)
        for _ in range(self.nu - 1):
            apply(x, ax)
            level.smooth(mine, k, False, stream)
        apply(x, ax)
        level.restrict_residual(mine, coarser, k, stream)
        self._cycle(l - 1, buffers, k, applies, stream)
        level.prolong_add(mine, coarser, k, stream)
        for _ in range(self.nu):
            apply(x, ax)
            level.smooth(mine, k, False, stream)

    def _vector(self, v, what):
        """``v`` as a flat vector of the hierarchy's type in the numbering of the finest level."""
        name, top = type(self).__name__, self.levels[-1]
        if _is_block(v):
            raise NotImplementedError(f"{name}.{what}: blocks (N, k) of vectors; one vector (N,) or (N, 1) "
                                      f"({self._BLOCKS})")
        flat = v.detach().to(self.device, self.dtype).reshape(-1)
        if flat.shape[0] != top.n:
            raise ValueError(f"{name}.{what}: {flat.shape[0]} entries, the finest level has {top.n} DoFs")
        return top.engine._dofs_in(flat) if top.crossing else flat

    def _result(self, x, like):
        top = self.levels[-1]
        if top.crossing:
            x = top.engine._dofs_out(x)
        return top.engine._home(x).reshape(like.shape)

    def _vcycle_into(self, r):
        """The cycle on the single-vector buffers, r in the finest level's numbering; returns the
        buffer that holds the result (valid until the next cycle)."""
        top = self.levels[-1]
        top.r.copy_(r)
        self._cycle(len(self.levels) - 1, self._buffers, None, self._level_applies(),
                    _native.current_stream(self.device))
        return top.x

    def vcycle(self, r):
        """One V-cycle on the residual ``r`` ((N,) or (N, 1), the DoFs of ``basis``): the approximate
        solution z of K z = r on the free DoFs, 0 on the held ones; shaped like r."""
        flat = self._vector(r, "vcycle")
        with torch.cuda.device(self.device):
            z = self._vcycle_into(flat).clone()
        return self._result(z, r)

    def _fused_pcg(self, rhs, start, k, rtol, maxiter):
        """``_fused_cycle_pcg`` on the hierarchy's own buffers: the vectors of the levels (k None) or
        their blocks of width k.  The residual lives in the top level's r buffer and z is read from
        its x buffer, so nothing is copied into the cycle or out of it."""
        top = len(self.levels) - 1
        buffers = self._buffers if k is None else self._block_buffers(k)
        P, AP = self._direction_buffers(k)
        applies, stream = self._level_applies(), _native.current_stream(self.device)
        Z, _, R = buffers[top]
        return _fused_cycle_pcg(self.levels[top].lib, applies[-1],
                                lambda: self._cycle(top, buffers, k, applies, stream), self.levels[top].mask, rhs,
                                R, Z, P, AP, start, rtol, maxiter)

    def solve(self, b, x0=None, rtol=1e-10, maxiter=100, free=None, loop=None):
        """Conjugate gradients preconditioned by ``vcycle`` for K x = b on the free DoFs (the held
        ones keep x0's values, 0 by default).  The relative residual |r| / |m b| is checked every
        iteration.  Returns (x shaped like b, iterations, relative residual).

        ``loop``: "fused" keeps the recurrence on the device (csrc/tfem_pcg.hip: four vector launches
        per iteration around the apply and the cycle, alpha, beta and the dot products never leave
        the device, one host read of |r|^2 per iteration); "torch" is the loop of torch operations;
        None is the fused loop for a ``b`` on a HIP device unless TFEM_CG=torch (``sparse._cg_loop``)."""
        if free is not None:
            raise NotImplementedError(f"{type(self).__name__}.solve: a custom set of free DoFs; the hierarchy holds "
                                      "the boundary DoFs of every level (dirichlet=True) or none")
        loop = _cg_loop(loop, b.device)
        rhs = self._vector(b, "solve")
        start = None if x0 is None else self._vector(x0, "solve")
        with torch.cuda.device(self.device):
            if loop == "fused":
                x, its, ress = self._fused_pcg(rhs, start, None, rtol, maxiter)
                it, res = int(its[0]), float(ress[0])
            else:
                x, it, res = _cycle_pcg(self._level_applies()[-1], self._vcycle_into, self.levels[-1].mask, rhs,
                                        start, rtol, maxiter)
        return self._result(x, b), it, res

    # ------------------------------------------------------------------ blocks of right-hand sides
    def _blocks_below(self, k):
        """Per level below ``_own`` the (x, ax, r) of shape (n_l, k): those of the hierarchy that owns
        these levels."""
        return []

    def _block_buffers(self, k):
        """Per level (x, ax, r) of shape (n_l, k), zero on first use of the width k and reused; the
        ``BLOCK_WIDTHS_KEPT`` most recently used widths are kept.  ``_blocks[k]`` holds those of
        ``_own`` and, behind them, the direction and its image of ``solve_multi``."""
        below = self._blocks_below(k)
        buffers = self._blocks.pop(k, None)
        if buffers is None:
            buffers = [tuple(torch.zeros(level.n, k, dtype=self.dtype, device=self.device) for _ in range(3))
                       for level in self._own]
            # behind the levels: the direction and its image of solve_multi, allocated by its first use
            buffers.append(None)
            if len(self._blocks) >= self.BLOCK_WIDTHS_KEPT:
                self._blocks.pop(next(iter(self._blocks)))
                # the prepared launches keep the buffers they point into: drop them with the width
                # (those of the widths that stay are prepared again on their next use)
                self._applies = {}
        self._blocks[k] = buffers  # the youngest
        return below + buffers[:-1]

    def _direction_buffers(self, k):
        """The direction of ``solve_multi`` and its image, (N, k) each, kept with the width k (a
        prepared launch keeps its two buffers); after ``_block_buffers(k)``.  k None: the two vectors
        (N,) of the fused loop of ``solve``."""
        if k is None:
            if self._directions is None:
                n = self.levels[-1].n
                self._directions = tuple(torch.empty(n, dtype=self.dtype, device=self.device) for _ in range(2))
            return self._directions
        kept = self._blocks[k]
        if kept[-1] is None:
            n = self.levels[-1].n
            kept[-1] = tuple(torch.empty(n, k, dtype=self.dtype, device=self.device) for _ in range(2))
        return kept[-1]

    def _block(self, V, what):
        """``V`` (N, k) in the hierarchy's type and in the numbering of the finest level."""
        top = self.levels[-1]
        if V.dim() != 2 or V.shape[0] != top.n or V.shape[1] < 1:
            raise ValueError(f"{type(self).__name__}.{what}: a block of shape ({top.n}, k) with k >= 1, "
                             f"got {tuple(V.shape)}")
        block = V.detach().to(self.device, self.dtype)
        return top.engine._dofs_in(block) if top.crossing else block

    def _block_result(self, X):
        top = self.levels[-1]
        if top.crossing:
            X = top.engine._dofs_out(X)
        return top.engine._home(X)

    def _vcycle_multi_into(self, R):
        """The cycle on the block buffers of R's width, R in the finest level's numbering; returns the
        buffer that holds the result (valid until the next block cycle of that width)."""
        k = int(R.shape[1])
        buffers = self._block_buffers(k)
        top = len(self.levels) - 1
        buffers[top][2].copy_(R)
        self._cycle(top, buffers, k, self._level_applies(), _native.current_stream(self.device))
        return buffers[top][0]

    def vcycle_multi(self, R):
        """One V-cycle on every column of ``R`` (N, k), k >= 1: Z (N, k) with column j the approximate
        solution of K z = r_j on the free DoFs, 0 on the held ones.  The cycle of ``vcycle``, every
        launch on (n_l, k) row-major blocks: the block applies of the levels, the block forms of the
        kernels of csrc/tfem_mg.hip (on a P2 level the P2 kind of its transfers), and one dense
        product on the coarsest level.  The block buffers are separate from those of
        ``vcycle`` and kept for the ``BLOCK_WIDTHS_KEPT`` most recently used widths."""
        block = self._block(R, "vcycle_multi")
        with torch.cuda.device(self.device):
            Z = self._vcycle_multi_into(block).clone()
        return self._block_result(Z)

    def solve_multi(self, B, X0=None, rtol=1e-10, maxiter=100, loop=None):
        """``solve`` for the k columns of ``B`` (N, k) at once: k conjugate-gradient recurrences
        preconditioned by ``vcycle_multi`` carried through one loop -- per iteration one block apply,
        one block cycle, column-wise dot products, one alpha and one beta per column, and one host
        read of the k relative residuals |r_j| / |m b_j|.  The contract of
        ``conjugate_gradients_multi``: a column whose residual is <= rtol at a check is frozen from
        then on -- its alpha and beta are 0 and its direction is zeroed, so its x and r stop
        changing and no 0/0 arises (a column that starts converged, e.g. an all-zero one, takes no
        iteration) -- and the loop ends when every column is frozen or after ``maxiter`` iterations.
        The held DoFs keep X0's values (0 by default).  Returns (X (N, k), iterations (k,) int64,
        relative residuals (k,)), the last two on the host; iterations[j] is the iteration at which
        column j was frozen.

        ``loop`` as in ``solve``.  The fused loop (csrc/tfem_pcg.hip) carries the k recurrences in the
        same four launches per iteration whatever k is; a frozen column's x and r are never written
        again (its direction is no longer updated instead of being zeroed), and the residuals come
        back in float64."""
        name, top = type(self).__name__, self.levels[-1]
        if B.dim() != 2 or B.shape[0] != top.n:
            raise ValueError(f"{name}.solve_multi: B must have shape ({top.n}, k), got {tuple(B.shape)}")
        loop = _cg_loop(loop, B.device)
        rhs = self._block(B, "solve_multi")
        n, k = rhs.shape
        if loop == "fused":
            start = None
            if X0 is not None:
                if tuple(X0.shape) != (n, k):
                    raise ValueError(f"{name}.solve_multi: X0 must have B's shape ({n}, {k})")
                start = self._block(X0, "solve_multi")
            with torch.cuda.device(self.device):
                X, its, res = self._fused_pcg(rhs, start, k, rtol, maxiter)
            return self._block_result(X), its, res
        with torch.cuda.device(self.device):
            # the blocks an apply is launched on are the kept ones of the width (a prepared launch
            # keeps its two buffers): x and K x of the finest level, the direction and its image
            buffers = self._block_buffers(k)
            P, AP = self._direction_buffers(k)
            apply = self._level_applies()[-1]
            mask = None if top.mask is None else top.mask.reshape(n, 1)
            if X0 is None:
                X = torch.zeros(n, k, dtype=self.dtype, device=self.device)
            else:
                if tuple(X0.shape) != (n, k):
                    raise ValueError(f"{name}.solve_multi: X0 must have B's shape ({n}, {k})")
                X = self._block(X0, "solve_multi").clone(memory_format=torch.contiguous_format)
            if X0 is None:
                R = rhs.clone(memory_format=torch.contiguous_format)
            else:
                top_x, top_ax, _ = buffers[len(self.levels) - 1]
                top_x.copy_(X)
                apply(top_x, top_ax)
                R = rhs - top_ax
            if mask is not None:
                R *= mask
            b_norm = torch.linalg.vector_norm(rhs if mask is None else mask * rhs, dim=0).clamp_min(
                torch.finfo(self.dtype).tiny)
            res = torch.linalg.vector_norm(R, dim=0) / b_norm
            active = res > rtol  # (k,) on the device; its host copy decides the loop
            running = active.cpu()
            its = torch.zeros(k, dtype=torch.int64, device="cpu")
            it = 0
            if maxiter > 0 and bool(running.any()):
                one, zero = torch.ones((), dtype=self.dtype, device=self.device), torch.zeros(k, dtype=self.dtype,
                                                                                              device=self.device)
                P.copy_(self._vcycle_multi_into(R))
                rz = (R * P).sum(0)
                P.mul_(active)
                while True:
                    apply(P, AP)
                    if mask is not None:
                        AP *= mask
                    pap = (P * AP).sum(0)
                    alpha = torch.where(active, rz / torch.where(active, pap, one), zero)
                    X.add_(alpha * P)
                    R.sub_(alpha * AP)
                    it += 1
                    res_new = torch.linalg.vector_norm(R, dim=0) / b_norm
                    res = torch.where(active, res_new, res)  # a frozen column reports what froze it
                    its[running] = it
                    active = active & (res > rtol)
                    running = active.cpu()  # the host read of the iteration
                    if it >= maxiter or not bool(running.any()):
                        break
                    Z = self._vcycle_multi_into(R)
                    rz_new = (R * Z).sum(0)
                    beta = torch.where(active, rz_new / torch.where(active, rz, one), zero)
                    P.mul_(beta).add_(Z * active)
                    rz = torch.where(active, rz_new, rz)
        return self._block_result(X), its, res.cpu()


class GeometricMultigrid(_Hierarchy):
    """V(nu, nu)-cycle and multigrid-preconditioned CG for a P1 form on ``levels`` uniform
    refinements of ``coarse_triangulation`` (a triangle-format dictionary, ``meshgen``).

    ``bilinear`` is the callable of ``Basis.integrate_bilinear_form``; it is traced on every level, so
    coefficients written as expressions of the integration points are evaluated on every mesh.
    ``dirichlet=True`` holds the boundary DoFs of every level at zero (``inner_dofs``);
    ``dirichlet=False`` solves on all DoFs, for forms with a mass term.  ``nu`` damped-Jacobi sweeps
    with damping ``omega`` before and after the coarse correction.  ``dtype``: the real type of the
    hierarchy (None: torch's default).  ``element``: the ``ElementTri`` of every level instead of
    ``ElementTri(1, quadrature_order)``.

    ``basis`` is the finest ``Basis`` (assemble the right-hand side with it), ``operator`` its
    ``FormOperator``, ``levels`` the list of levels, coarsest first (each with ``basis``, ``op``,
    ``engine``, ``n``), ``parents`` the parent tables of the refinements (``parents[l - 1]`` takes
    level l - 1 to level l).

    ``vcycle`` and ``solve`` take one vector.  Blocks (N, k) of right-hand sides go through
    ``vcycle_multi`` and ``solve_multi``: the same cycle on (n_l, k) buffers, so the same number of
    launches whatever k is.

    Refused with NotImplementedError: P2 elements (``P2Multigrid``), fracture bases, coefficient data
    (``basis.coefficient``: its shape belongs to one mesh), a custom set of free DoFs; and a coarse
    mesh with more than ``Basis.DENSE_SOLVE_LIMIT`` free DoFs."""

    def __init__(self, coarse_triangulation, levels, bilinear, quadrature_order=2, dirichlet=True, nu=2,
                 omega=2.0 / 3.0, dtype=None, *, element=None):
        from .basis import FractureBasis
        from .mesh import MeshesTri

        if isinstance(coarse_triangulation, (FractureBasis, MeshesTri)):
            raise NotImplementedError("GeometricMultigrid: fracture bases (batched meshes) have no hierarchy of "
                                      "refinements here")
        if not isinstance(coarse_triangulation, Mapping) or any(k not in coarse_triangulation for k in _MESH_KEYS):
            raise TypeError("GeometricMultigrid: the coarse mesh is a triangle-format dictionary with the keys "
                            + ", ".join(_MESH_KEYS))
        if element is not None and getattr(element, "polynomial_order", 1) != 1:
            raise NotImplementedError("GeometricMultigrid: P2 elements (the transfers are those of nested P1 spaces; "
                                      "P2Multigrid puts a P2 level on top of this hierarchy)")
        levels, nu = int(levels), int(nu)
        if levels < 0 or nu < 1:
            raise ValueError("GeometricMultigrid: levels >= 0 and nu >= 1")
        self.nu, self.omega, self.dirichlet = nu, float(omega), bool(dirichlet)

        meshes, self.parents = [{k: np.asarray(coarse_triangulation[k]) for k in _MESH_KEYS}], []
        for _ in range(levels):
            fine, parents = meshgen.refine_uniform(meshes[-1])
            meshes.append(fine)
            self.parents.append(parents)

        previous = torch.get_default_dtype()
        if dtype is not None:
            torch.set_default_dtype(dtype)
        try:
            if element is None:  # built here: an element keeps tables in the default dtype of its creation
                element = ElementTri(polynomial_order=1, integration_order=int(quadrature_order))
            self.levels = [_build_level("GeometricMultigrid", _Level, mesh, element, bilinear, ("operator",))
                           for mesh in meshes]
        finally:
            torch.set_default_dtype(previous)
        self.basis = self.levels[-1].basis
        self.operator = self.levels[-1].op
        self.device, self.dtype = self.levels[-1].engine.device, self.levels[-1].engine.dtype
        with torch.cuda.device(self.device):
            for l, level in enumerate(self.levels):
                self._prepare_level(level, _identity)
                if l > 0:
                    level.set_coarser(self.levels[l - 1], self.parents[l - 1], self.device)
            self._factor_coarse(self.levels[0])
        self._own = self.levels
        self._buffers = [(level.x, level.ax, level.r) for level in self.levels]
        self._applies = {}  # stream -> the prepared applies of the levels
        self._blocks = {}  # k -> per level (x, ax, r) of shape (n_l, k); insertion order = age of last use

    # ------------------------------------------------------------------ set-up
    def _factor_coarse(self, level):
        n_free = level.n if level.free is None else int(level.free.numel())
        if n_free > Basis.DENSE_SOLVE_LIMIT:
            raise NotImplementedError(f"GeometricMultigrid: the coarse mesh has {n_free} free DoFs, the dense "
                                      f"coarse solve takes at most {Basis.DENSE_SOLVE_LIMIT}: start from a coarser mesh")
        dense = level.op.to_csr().to_dense().to(self.device, self.dtype)
        if level.free is not None:
            dense = dense[level.free][:, level.free]
        # K0[free, free]^-1 from the factorisation, once, embedded in the rows and columns of all coarse
        # DoFs (zero on the held ones): the coarse solve of a cycle is then ONE matrix-vector product
        # instead of two triangular solves and a gather / scatter (0.35 ms of a 0.6 ms cycle at 900
        # coarse DoFs, profiles/mg_solve.log)
        level.inverse = torch.zeros(level.n, level.n, dtype=self.dtype, device=self.device)
        if n_free > 0:
            factor, info = torch.linalg.cholesky_ex(dense)
            if int(info) == 0:
                inverse = torch.cholesky_inverse(factor)
            else:
                # the forms carry the signed determinant: with triangles stored clockwise K0 is not
                # positive definite, and the factorisation is an LU
                inverse = torch.linalg.inv(dense)
            inverse = 0.5 * (inverse + inverse.mT)
            if level.free is None:
                level.inverse.copy_(inverse)
            else:
                level.inverse[level.free[:, None], level.free[None, :]] = inverse

    def __repr__(self):
        sizes = ", ".join(str(level.n) for level in self.levels)
        return (f"GeometricMultigrid({len(self.levels) - 1} refinements: {sizes} DoFs, V({self.nu},{self.nu}), "
                f"omega={self.omega:.3g}, dtype={self.dtype})")


class P2Multigrid(_Hierarchy):
    """V(nu, nu)-cycle and multigrid-preconditioned CG for a P2 form: a P2 level on the finest mesh
    of a P1 hierarchy (p-coarsening first, then the h-hierarchy of ``GeometricMultigrid``).

    P1 is a subspace of P2 on one mesh and both spaces are discretised from the same callable, so
    the P1 operator of the finest mesh IS the Galerkin operator P^T K2 P of the P2 one: no triple
    product here either.  The cycle is the one of ``GeometricMultigrid`` run over ``levels``, the P1
    levels and then the P2 level: the P2 level sweeps with w = omega * m2 / diag K2 and makes its own
    two transfers (``tfem_mg_p2_*``, csrc/tfem_mg.hip), and below it the cycle runs on the P1 hierarchy's own
    buffers with the P1 hierarchy's own prepared applies.

    The arguments are those of ``GeometricMultigrid`` (``levels`` refinements below the mesh that
    carries the P2 level, 0 allowed; ``quadrature_order`` of both elements).  ``p1`` is the P1
    hierarchy, ``basis`` the P2 ``Basis`` of its finest mesh (assemble the right-hand side with it),
    ``operator`` its ``FormOperator`` -- ``layout="matrix_free"`` where the basis grants it, the
    assembled CSR otherwise --, ``levels`` the P1 levels and then the P2 level.

    A matrix-free P2 operator is applied in the ENGINE's numbering (the engine renumbers the edge
    DoFs of a basis from 50,000 DoFs on; the vertex ids stay those of the P1 level): the tables,
    masks and weights of the P2 level are built in that numbering and vectors and blocks cross once
    at the boundary of ``vcycle`` / ``solve`` / ``vcycle_multi`` / ``solve_multi``.

    ``vcycle`` and ``solve`` take one vector.  Blocks (N, k) of right-hand sides go through
    ``vcycle_multi`` and ``solve_multi``, with the contracts of ``GeometricMultigrid``'s: the P2 level
    runs its sweeps, its block apply and its two transfers (``tfem_mg_p2_*_multi``) on its own
    (N, k) buffers, and below it the block cycle runs on the P1 hierarchy's block buffers of the same
    width, so the number of launches does not depend on k.

    Refused with NotImplementedError: what ``GeometricMultigrid`` refuses and a custom set of free
    DoFs."""

    _BLOCKS = "blocks: vcycle_multi, solve_multi of P2Multigrid"

    def __init__(self, coarse_triangulation, levels, bilinear, quadrature_order=3, dirichlet=True, nu=2,
                 omega=2.0 / 3.0, dtype=None):
        self.p1 = GeometricMultigrid(coarse_triangulation, levels, bilinear, quadrature_order, dirichlet, nu, omega,
                                     dtype)
        self.nu, self.omega, self.dirichlet = self.p1.nu, self.p1.omega, self.p1.dirichlet
        self.device, self.dtype = self.p1.device, self.p1.dtype
        previous = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)
        try:  # an element keeps tables in the default dtype of its creation
            element = ElementTri(polynomial_order=2, integration_order=int(quadrature_order))
            top = _build_level("P2Multigrid", _P2Level, self.p1.levels[-1].triangulation, element, bilinear,
                               ("matrix_free", "operator"))
        finally:
            torch.set_default_dtype(previous)
        self.basis, self.operator = top.basis, top.op
        self.levels = self.p1.levels + [top]
        with torch.cuda.device(self.device):
            top.set_coarser(self.p1.levels[-1], self.device)
            self._prepare_level(top, top.engine._dofs_in if top.crossing else _identity)
        self._own = [top]
        self._buffers = self.p1._buffers + [(top.x, top.ax, top.r)]
        self._applies = {}  # stream -> the prepared apply of the P2 level
        self._blocks = {}  # k -> (x, ax, r) of shape (N, k) of the P2 level; insertion order = age of last use

    def _level_applies(self):
        return self.p1._level_applies() + super()._level_applies()

    def _blocks_below(self, k):
        return self.p1._block_buffers(k)

    def __repr__(self):
        sizes = ", ".join(str(level.n) for level in self.levels)
        return (f"P2Multigrid(P2 over {len(self.p1.levels) - 1} refinements: {sizes} DoFs, V({self.nu},{self.nu}), "
                f"omega={self.omega:.3g}, dtype={self.dtype})")


