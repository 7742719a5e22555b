"""CSR global operator.

The reference assembles into a dense ``torch.zeros((N, N))`` (abstract_basis.py:81),
which is 2 TB at 5e5 DoFs.  The HIP path always produces CSR values; ``to_dense``
materialises the reference's layout when it fits.
"""

from __future__ import annotations

import os

import torch

from . import _native

#: TFEM_CG=torch: solve_cg / solve_cg_multi keep the loop of torch operations on the GPU as well
#: (read once, here: the solve path asks no environment variable).  Anything else: the fused loop.
_CG_LOOP = "torch" if os.environ.get("TFEM_CG", "").strip().lower() == "torch" else "fused"


def _cg_loop(loop, device):
    """The loop a solve runs: ``loop`` ("fused" | "torch" | None = the default: fused on a HIP
    device unless TFEM_CG=torch, the torch loop on the host)."""
    if loop not in (None, "fused", "torch"):
        raise ValueError(f"loop must be None, 'fused' or 'torch', not {loop!r}")
    on_gpu = torch.device(device).type == "cuda"
    if loop == "fused" and not on_gpu:
        raise ValueError("loop='fused': the fused CG kernels need the vectors on a HIP device")
    if loop is None:
        return _CG_LOOP if on_gpu else "torch"
    return loop


class CSRMatrix:
    """``crow_indices`` int64 (N+1), ``col_indices`` int32 (nnz, ascending per row),
    ``values`` (nnz); all on one device.

    ``perm`` (int64 (N,) or None): the operator is stored in a RENUMBERING of the caller's DoFs --
    row / column k of the stored pattern is DoF ``perm[k]`` of the caller.  The assembly engine
    renumbers a mesh whose vertex numbering has no locality along a space-filling curve once, at
    set-up, so that the row kernels stream coordinates and values contiguously; every method below
    takes and returns vectors in the CALLER's numbering, ``to_dense`` gives the caller's matrix, and
    ``caller_numbering()`` the plain CSR arrays in the caller's numbering."""

    def __init__(self, crow_indices, col_indices, values, shape, perm=None):
        self.crow_indices = crow_indices
        self.col_indices = col_indices
        self.values = values
        self.shape = tuple(shape)
        self.perm = perm
        self._inv = None

    def _inverse(self):
        if self._inv is None:
            self._inv = torch.empty_like(self.perm)
            self._inv[self.perm] = torch.arange(self.perm.numel(), device=self.perm.device)
        return self._inv

    def _stored(self):
        """The same stored arrays without the renumbering attached (vectors in stored numbering)."""
        return CSRMatrix(self.crow_indices, self.col_indices, self.values, self.shape)

    def caller_numbering(self):
        """Plain CSRMatrix (perm None) with rows, columns and values in the caller's numbering."""
        if self.perm is None:
            return self
        n = self.shape[0]
        counts = self.crow_indices[1:] - self.crow_indices[:-1]
        rows = self.perm[torch.repeat_interleave(torch.arange(n, device=self.device), counts)]
        cols = self.perm[self.col_indices.long()]
        order = torch.argsort(rows * n + cols)
        crow = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        crow[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
        return CSRMatrix(crow, cols[order].to(torch.int32), self.values[order], self.shape)

    @property
    def nnz(self):
        return int(self.values.shape[0])

    @property
    def device(self):
        return self.values.device

    @property
    def dtype(self):
        return self.values.dtype

    def to(self, device):
        return CSRMatrix(
            self.crow_indices.to(device), self.col_indices.to(device), self.values.to(device), self.shape,
            None if self.perm is None else self.perm.to(device),
        )

    def to_sparse_csr(self):
        if self.perm is not None:
            return self.caller_numbering().to_sparse_csr()
        return torch.sparse_csr_tensor(
            self.crow_indices, self.col_indices.to(torch.int64), self.values, size=self.shape
        )

    def to_dense(self):
        n = self.shape[0]
        if self.perm is not None:
            inv = self._inverse()
            return self._stored().to_dense()[inv][:, inv]
        if self.values.is_cuda:
            lib = _native.load()
            dense = torch.empty(self.shape, dtype=self.dtype, device=self.device)
            with torch.cuda.device(self.device):
                _native.check(
                    lib.tfem_csr_to_dense(
                        _native.ptr(self.crow_indices),
                        _native.ptr(self.col_indices),
                        _native.ptr(self.values),
                        self.values.element_size(),
                        n,
                        _native.ptr(dense),
                        _native.current_stream(self.device),
                    )
                )
            return dense
        # host copy of an already assembled operator: pure data movement, no arithmetic
        dense = torch.zeros(self.shape, dtype=self.dtype)
        rows = torch.repeat_interleave(torch.arange(n), self.crow_indices[1:] - self.crow_indices[:-1])
        dense[rows, self.col_indices.long()] = self.values
        return dense

    def matvec(self, x):
        """A @ x for x of shape (N,) or (N, 1): libtfem_hip's CSR kernel on the GPU (tfem_csr_spmv).
        (N, k) with k >= 2 gives (N, k): on the GPU ONE tfem_csr_spmm launch on the contiguous
        row-major block (the matrix is read once for the k columns; with ``perm`` one row gather
        on the way in and one on the way out), column j bit for bit what the single launch gives
        for column j; on the host column by column."""
        if _is_block(x):
            if x.shape[0] != self.shape[1]:
                raise ValueError(f"matvec: x has {x.shape[0]} rows, the operator {self.shape[1]} columns")
            if not self.values.is_cuda:
                return torch.stack([self.matvec(x[:, j]) for j in range(x.shape[1])], dim=1)
            block = x.to(self.device, self.dtype)
            if self.perm is not None:
                return self._stored().matvec(block[self.perm])[self._inverse()]
            block = block.contiguous()
            y = torch.empty(self.shape[0], block.shape[1], dtype=self.dtype, device=self.device)
            with torch.cuda.device(self.device):
                self._prepared_spmv(block, y)()
            return y
        if self.perm is not None:
            flat = x.to(self.device, self.dtype).reshape(-1)
            return self._stored().matvec(flat[self.perm])[self._inverse()].reshape(x.shape)
        if not self.values.is_cuda:
            return self.to_sparse_csr() @ x
        lib = _native.load()
        flat = x.to(self.device, self.dtype).reshape(-1).contiguous()
        if flat.shape[0] != self.shape[1]:
            raise ValueError(f"matvec: x has {flat.shape[0]} entries, the operator {self.shape[1]} columns")
        y = torch.empty(self.shape[0], dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._prepared_spmv(flat, y)()
        return y.reshape(x.shape)

    def _prepared_spmv(self, x, y):
        """y = A x in the STORED numbering into a given y, nothing allocated: x and y contiguous
        device tensors of the operator's dtype, (N,) or (N, k) of the same shape (a block: ONE
        tfem_csr_spmm launch straight on the two row-major buffers, no staging vector and no copy;
        (N,) and (N, 1): tfem_csr_spmv).  The arguments are converted once; the returned callable
        only enqueues, on the stream that is current now."""
        n = self.shape[0]
        for t, rows in ((x, self.shape[1]), (y, n)):
            if t.dtype != self.dtype or t.device != self.device or not t.is_contiguous() or t.shape[0] != rows:
                raise ValueError(f"spmv: contiguous {self.dtype} tensors of {rows} rows on {self.device}")
        matrix = (_native.ptr(self.crow_indices), _native.ptr(self.col_indices), _native.ptr(self.values),
                  self.values.element_size(), n)
        vectors = (_native.ptr(x), _native.ptr(y), _native.current_stream(self.device))
        if _is_block(x):
            if y.shape[1:] != x.shape[1:]:
                raise ValueError(f"spmv: x has {x.shape[1]} columns, y has shape {tuple(y.shape)}")
            fn = _native.load().tfem_csr_spmm
            args = (*matrix, self.shape[1], x.shape[1], *vectors)
        else:
            fn = _native.load().tfem_csr_spmv
            args = (*matrix, *vectors)
        keep = (self, x, y)  # what the raw pointers above point into

        def launch():
            status = fn(*args)
            if status:
                _native.check(status)
            return keep[2]

        return launch

    def diagonal(self):
        """Diagonal entries (0 where a row stores none)."""
        if self.perm is not None:
            return self._stored().diagonal()[self._inverse()]
        n = self.shape[0]
        counts = self.crow_indices[1:] - self.crow_indices[:-1]
        rows = torch.repeat_interleave(torch.arange(n, device=self.device), counts)
        hit = self.col_indices.long() == rows
        diag = torch.zeros(n, dtype=self.dtype, device=self.device)
        diag[rows[hit]] = self.values[hit]
        return diag

    def solve_cg(self, b, free=None, x0=None, rtol=1e-12, maxiter=None, loop=None):
        """Jacobi-preconditioned conjugate gradients for the symmetric positive definite
        operator restricted to the DoFs `free` (index tensor; the others keep x0's values, 0 by
        default: homogeneous Dirichlet rows and columns are simply masked, no submatrix is
        formed).  Returns (x, iterations, relative residual).  Stands where the reference's
        dense `reduce` + `torch.linalg.solve` (abstract_basis.py:114-117,177-195) stops being
        possible.  On the GPU the loop is ``fused_conjugate_gradients`` (the SpMV
        and three tfem_cg_* launches per iteration); ``loop="torch"`` or TFEM_CG=torch keeps the loop
        of torch operations (``conjugate_gradients``), ``loop="fused"`` insists on the kernels."""
        which = _cg_loop(loop, self.device)
        if self.perm is not None:  # solve in the stored numbering, vectors translated at the boundary
            inv = self._inverse()
            to_stored = lambda v: None if v is None else v.to(self.device, self.dtype).reshape(-1)[self.perm]  # noqa: E731
            free_s = None if free is None else inv[free.to(self.device).reshape(-1)]
            x, it, res = self._stored().solve_cg(to_stored(b), free_s, to_stored(x0), rtol, maxiter, which)
            return x[inv].reshape(b.shape), it, res
        if which == "fused":
            x, it, res = fused_conjugate_gradients(_into(self._prepared_spmv), self.diagonal(), b.reshape(-1), free,
                                                   None if x0 is None else x0.reshape(-1), rtol, maxiter)
        else:
            x, it, res = conjugate_gradients(self.matvec, self.diagonal(), b, free, x0, rtol, maxiter)
        return x.reshape(b.shape), it, res

    def solve_cg_multi(self, B, free=None, X0=None, rtol=1e-12, maxiter=None, loop=None):
        """``solve_cg`` for the k columns of B (N, k) at once (``conjugate_gradients_multi``, on the
        GPU ``fused_conjugate_gradients``; ``loop`` as in ``solve_cg``): one block application per
        iteration.  Returns (X (N, k), iterations (k,), relative residuals (k,))."""
        which = _cg_loop(loop, self.device)
        if self.perm is not None:  # solve in the stored numbering, rows translated at the boundary
            inv = self._inverse()
            to_stored = lambda v: None if v is None else v.to(self.device, self.dtype)[self.perm]  # noqa: E731
            free_s = None if free is None else inv[free.to(self.device).reshape(-1)]
            X, it, res = self._stored().solve_cg_multi(to_stored(B), free_s, to_stored(X0), rtol, maxiter, which)
            return X[inv], it, res
        if which == "fused":
            if B.dim() != 2 or B.shape[0] != self.shape[0]:
                raise ValueError(f"solve_cg_multi: B must have shape ({self.shape[0]}, k)")
            return fused_conjugate_gradients(_into(self._prepared_spmv), self.diagonal(), B, free, X0, rtol, maxiter)
        return conjugate_gradients_multi(self.matvec, self.diagonal(), B, free, X0, rtol, maxiter)

    def __repr__(self):
        extra = "" if self.perm is None else ", stored in a renumbering of the DoFs"
        return f"CSRMatrix(shape={self.shape}, nnz={self.nnz}, dtype={self.dtype}, device={self.device}{extra})"


def conjugate_gradients(matvec, diagonal, b, free=None, x0=None, rtol=1e-12, maxiter=None):
    """Jacobi-preconditioned conjugate gradients for a symmetric positive definite operator given
    by ``matvec`` (flat (N,) -> (N,)) and its ``diagonal`` ((N,) tensor), restricted to the DoFs
    ``free`` (index tensor; the others keep x0's values, 0 by default).  Vectors live on the
    diagonal's device and dtype.  Returns (x (N,), iterations, relative residual).  The loop of
    ``CSRMatrix.solve_cg`` and ``FormOperator.solve_cg``."""
    n = diagonal.shape[0]
    dtype, device = diagonal.dtype, diagonal.device
    b = b.to(device, dtype).reshape(-1)
    mask = torch.ones(n, dtype=dtype, device=device)
    if free is not None:
        mask.zero_()
        mask[free.to(device).reshape(-1)] = 1
    x = torch.zeros(n, dtype=dtype, device=device) if x0 is None else x0.to(device, dtype).reshape(-1).clone()
    inv_diag = mask / torch.where(diagonal != 0, diagonal, torch.ones_like(mask))
    r = mask * (b - matvec(x))
    x = x.clone()
    z = inv_diag * r
    p = z.clone()
    rz = torch.dot(r, z)
    b_norm = torch.linalg.vector_norm(mask * b).clamp_min(torch.finfo(dtype).tiny)
    maxiter = maxiter or 10 * n
    it, res = 0, float(torch.linalg.vector_norm(r) / b_norm)
    while it < maxiter and res > rtol:
        ap = mask * matvec(p)
        alpha = rz / torch.dot(p, ap)
        x += alpha * p
        r -= alpha * ap
        z = inv_diag * r
        rz_new = torch.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
        if it % 25 == 0 or it == maxiter:  # one host synchronisation every 25 iterations
            res = float(torch.linalg.vector_norm(r) / b_norm)
    res = float(torch.linalg.vector_norm(r) / b_norm)
    return x, it, res


def conjugate_gradients_multi(matvec, diagonal, B, free=None, X0=None, rtol=1e-12, maxiter=None):
    """``conjugate_gradients`` for the k columns of ``B`` (N, k) at once: k independent
    Jacobi-preconditioned CG recurrences carried through the same tensor operations -- one block
    application ``matvec`` ((N, k) -> (N, k)) per iteration, column-wise dot products, one alpha
    and one beta per column.  A column is converged when its relative residual is <= rtol at a
    check (every 25 iterations, as in ``conjugate_gradients``; a column that starts converged, e.g.
    an all-zero right-hand side, takes no iteration); from then on it is frozen -- its alpha and
    beta are zero and its search direction is zeroed, so x, r and p stop changing and no 0/0
    arises -- and the loop ends when every column is.  Returns (X (N, k), iterations (k,) int64,
    relative residuals (k,)), the last two on the host."""
    n = diagonal.shape[0]
    dtype, device = diagonal.dtype, diagonal.device
    B = B.to(device, dtype)
    if B.dim() != 2 or B.shape[0] != n:
        raise ValueError(f"conjugate_gradients_multi: B must have shape ({n}, k)")
    k = B.shape[1]
    mask = torch.ones(n, 1, dtype=dtype, device=device)
    if free is not None:
        mask.zero_()
        mask[free.to(device).reshape(-1)] = 1
    X = torch.zeros(n, k, dtype=dtype, device=device) if X0 is None else X0.to(device, dtype).reshape(n, k).clone()
    diag = diagonal.reshape(n, 1)
    inv_diag = mask / torch.where(diag != 0, diag, torch.ones_like(diag))
    R = mask * (B - matvec(X))
    Z = inv_diag * R
    P = Z.clone()
    rz = (R * Z).sum(0)
    b_norm = torch.linalg.vector_norm(mask * B, dim=0).clamp_min(torch.finfo(dtype).tiny)
    maxiter = maxiter or 10 * n
    res = torch.linalg.vector_norm(R, dim=0) / b_norm
    active = res > rtol  # (k,) on the device; its host copy decides the loop
    P = P * active
    running = active.cpu()
    its = torch.zeros(k, dtype=torch.int64)
    it = 0
    one = torch.ones((), dtype=dtype, device=device)
    while it < maxiter and bool(running.any()):
        AP = mask * matvec(P)
        pap = (P * AP).sum(0)
        alpha = torch.where(active, rz / torch.where(active, pap, one), torch.zeros_like(rz))
        X += alpha * P
        R -= alpha * AP
        Z = inv_diag * R
        rz_new = (R * Z).sum(0)
        beta = torch.where(active, rz_new / torch.where(active, rz, one), torch.zeros_like(rz))
        P = torch.where(active, Z + beta * P, P)
        rz = torch.where(active, rz_new, rz)
        it += 1
        if it % 25 == 0 or it == maxiter:  # one host synchronisation every 25 iterations
            res = torch.linalg.vector_norm(R, dim=0) / b_norm
            its[running] = it
            active = active & (res > rtol)
            P = P * active
            running = active.cpu()
    its[running] = it
    res = torch.linalg.vector_norm(R, dim=0) / b_norm
    return X, its, res.cpu()


def _into(prepare):
    """``matvec_into(u, out)`` for ``fused_conjugate_gradients`` from a ``prepare(u, out)`` that
    returns the launch with its arguments converted: one preparation per pair of buffers (the loop
    applies the same pair every iteration), then only the enqueue."""
    prepared = {}

    def matvec_into(u, out):
        key = (u.data_ptr(), out.data_ptr(), tuple(u.shape))
        launch = prepared.get(key)
        if launch is None:
            launch = prepared[key] = prepare(u, out)
        launch()

    return matvec_into


def cg_constants():
    """(lanes per workgroup, cap of the number of workgroups, columns per pass) of the tfem_cg_*
    launches (csrc/tfem_cg.hip)."""
    lib = _native.load()
    return tuple(int(lib.tfem_cg_constant(i)) for i in range(3))


def cg_workspace(n, k, device):
    """The workspace of the tfem_cg_* launches for n x k vectors, as a (5, G, k) float64 tensor:
    per-workgroup partial sums of p.Ap | r.z, r.r of parity 0 | r.z, r.r of parity 1."""
    size = int(_native.load().tfem_cg_workspace_bytes(n, k))
    if size < 0:
        raise ValueError(f"fused CG: vectors of {n} x {k} entries are beyond the kernels' 32-bit extent")
    return torch.empty(size // 8, dtype=torch.float64, device=device).view(5, -1, k)


def fused_conjugate_gradients(matvec_into, diagonal, B, free=None, X0=None, rtol=1e-12, maxiter=None):
    """``conjugate_gradients`` (B of shape (N,)) and ``conjugate_gradients_multi`` (B of shape
    (N, k)) on a HIP device with the vector part in libtfem_hip (csrc/tfem_cg.hip): per iteration
    ``matvec_into(P, AP)`` (writes A P into the preallocated AP, same shape as B) and three
    launches -- tfem_cg_dot, tfem_cg_update, tfem_cg_direction -- with alpha, beta and the dot
    products on the device; the host reads |r|^2 from the workspace at the check every 25
    iterations and at maxiter, as the torch loops do.  The same recurrence, contract and return
    values: (x, iterations, relative residual), or (X, iterations (k,), residuals (k,)) with the
    last two on the host for a block (the residuals in float64: the sums are kept in double).  A column that starts converged takes no iteration; a frozen
    column's direction is zeroed at the check and its x and r are never written again."""
    lib = _native.load()
    n = diagonal.shape[0]
    dtype, device = diagonal.dtype, diagonal.device
    if device.type != "cuda":
        raise ValueError("fused_conjugate_gradients: the vectors must be on a HIP device")
    single = B.dim() == 1
    B = B.to(device, dtype)
    if B.shape[0] != n or B.dim() > 2:
        raise ValueError(f"fused_conjugate_gradients: B must have shape ({n},) or ({n}, k)")
    B = B.reshape(n, -1)
    k = B.shape[1]
    shape = (n,) if single else (n, k)
    mask = torch.ones(n, 1, dtype=dtype, device=device)
    if free is not None:
        mask.zero_()
        mask[free.to(device).reshape(-1)] = 1
    X = torch.zeros(n, k, dtype=dtype, device=device) if X0 is None else X0.to(device, dtype).reshape(n, k).clone(memory_format=torch.contiguous_format)
    diag = diagonal.reshape(n, 1)
    inv_diag = (mask / torch.where(diag != 0, diag, torch.ones_like(diag))).reshape(-1).contiguous()
    AP, P = torch.empty(n, k, dtype=dtype, device=device), torch.empty(n, k, dtype=dtype, device=device)
    maxiter = maxiter or 10 * n
    its = torch.zeros(k, dtype=torch.int64, device="cpu")
    with torch.cuda.device(device):
        matvec_into(X.view(shape), AP.view(shape))
        R = mask * (B - AP)
        b_norm = torch.linalg.vector_norm(mask * B, dim=0).clamp_min(torch.finfo(dtype).tiny)
        res = torch.linalg.vector_norm(R, dim=0) / b_norm
        active = res > rtol  # (k,) on the device; its host copy decides the loop
        running = active.cpu()
        it = 0
        res0, flags0 = res.double(), active
        res = res0
        if n > 0 and k > 0 and maxiter > 0 and bool(running.any()):
            ws = cg_workspace(n, k, device)
            flags = active.to(torch.int32)
            stream = _native.current_stream(device)
            size = (B.element_size(), n, k)
            x_, r_, p_, ap_, d_, f_, w_ = (_native.ptr(t) for t in (X, R, P, AP, inv_diag, flags, ws))
            _native.check(lib.tfem_cg_start(r_, d_, p_, *size, w_, stream))
            if not bool(running.all()):
                P *= active
            dot, update, direction = lib.tfem_cg_dot, lib.tfem_cg_update, lib.tfem_cg_direction
            dot_args = (p_, ap_, d_, *size, w_, stream)
            P_view, AP_view = P.view(shape), AP.view(shape)
            b_norm2 = b_norm.double()
            while it < maxiter and bool(running.any()):
                matvec_into(P_view, AP_view)
                status = (dot(*dot_args) or update(x_, r_, p_, ap_, d_, f_, *size, it, w_, stream)
                          or direction(p_, r_, d_, f_, *size, it, w_, stream))
                if status:
                    _native.check(status)
                it += 1
                if it % 25 == 0 or it == maxiter:  # one host synchronisation every 25 iterations
                    res = ws[2 + 2 * ((it - 1) & 1)].sum(0).sqrt() / b_norm2
                    its[running] = it
                    active = active & (res > rtol)
                    P *= active
                    flags.copy_(active)
                    running = active.cpu()
            its[running] = it
            # the loop ended at a check: what it decided on is what is reported (a column that
            # took no iteration keeps the residual of the set-up)
            res = torch.where(flags0, res, res0)
    if single:
        return X.reshape(-1), int(its[0]), float(res[0])
    return X, its, res.cpu()


def _is_block(x):
    """A block of k >= 2 vectors, shape (N, k) ((N,) and (N, 1) are single vectors)."""
    return x.dim() == 2 and x.shape[1] > 1


class _OperatorApply(torch.autograd.Function):
    """u -> K u of a symmetric operator, differentiable in u: the backward is the same
    application (K^T = K), e.g. for energy-norm losses u^T K u."""

    @staticmethod
    def forward(ctx, u, op):
        ctx.op = op
        return op._apply(u.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return ctx.op._apply(grad_out), None


class _FieldApply(torch.autograd.Function):
    """u -> K u of an operator with coefficient DATA, differentiable in u (the same application:
    K^T = K) and in the values kappa, c at the integration points: one tfem_p1_field_adjoint call
    gives d (g^T K u) / d kappa[e][q] and d / d c[e][q].  `kappa` / `c` are the (E, Q) views of the
    marked tensors (an expanded view for one value per element: autograd sums over q through it) or
    None; the forward launch reads the operator's own compact copies, not these."""

    @staticmethod
    def forward(ctx, u, kappa, c, op):
        ctx.op = op
        ctx.save_for_backward(u.detach())
        return op._apply(u.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        op = ctx.op
        (u,) = ctx.saved_tensors
        need_u, need_kappa, need_c = ctx.needs_input_grad[:3]
        grad_u = op._apply(grad_out) if need_u else None
        grad_kappa = grad_c = None
        if need_kappa or need_c:
            grad_kappa, grad_c = op._engine.field_adjoint(op.alpha, op.beta, grad_out, u, need_kappa, need_c)
            sources = op._field_sources
            if grad_kappa is not None:
                grad_kappa = grad_kappa.to(sources[0].device)
            if grad_c is not None:
                grad_c = grad_c.to(sources[1].device)
        return grad_u, grad_kappa, grad_c, None


class FormOperator:
    """The global operator of a bilinear form, to apply and to solve with, without necessarily
    storing it (``Basis.integrate_bilinear_form(..., layout="operator")`` or ``layout="matrix_free"``).

    Matrix-free (``matrix_free`` True): ``alpha * stiffness + beta * mass`` of a P1 basis whose
    engine has a ring plan; every ``matvec`` is one tfem_p1_apply_rings launch that forms the rows
    of K in registers and writes K u -- the values of K are never stored.  The operator may carry
    the source programs of variable coefficients kappa(x, y), c(x, y) (tfem_p1_apply_rings_coef then:
    the programs are evaluated per triangle inside the launch), or coefficient DATA -- values of kappa
    and c at the integration points or per element (``basis.coefficient``; tfem_p1_apply_rings_field:
    the values of a tile's elements are read once per tile and reduced in LDS); ``matvec`` is then also
    differentiable in the values (tfem_p1_field_adjoint).  Otherwise the operator
    wraps the CSRMatrix of today's assembly and applies it with tfem_csr_spmv (P2, fractures, any
    other integrand, meshes without a ring plan); the interface and the results are the same.
    Vectors are taken and returned in the caller's DoF numbering, of shape (N,) or (N, 1); a block
    (N, k) of k >= 2 vectors gives (N, k): matrix-free on P1 by ONE call that forms the rows of K
    once for the k columns (tfem_p1_apply_rings_multi; with coefficient programs
    tfem_p1_apply_rings_coef_multi, which evaluates the programs once for the k columns; with
    coefficient data tfem_p1_apply_rings_field_multi, which reads and reduces the values once for the
    k columns -- also the forward and the ``K g`` of the backward of a differentiable ``matvec``), the
    operator that wraps the CSR by ONE tfem_csr_spmm launch that reads the matrix once for the k
    columns (``CSRMatrix.matvec``; also the backward of ``matvec`` in the block, and every iteration
    of the block CG loops), the P2 matrix-free operator by ONE tfem_p2_apply_rows_multi call that reads
    the records and colind and forms a row's entries once for the k columns; only the operator with
    coefficient data on a plan whose tiles leave no room in LDS for two columns runs its
    single-vector launch once per column.

    ``layout="matrix_free"`` is the strict request: the plan is built at the call, the operator it
    returns is matrix-free from the start (``matrix_free`` True), and a basis or form without the
    launch raises NotImplementedError there instead of assembling.  It also serves P2 bases
    (``p2_rows``): ``alpha * stiffness + beta * mass`` over the P2 row plan, every ``matvec`` one
    tfem_p2_apply_rows call (vertex rows, long vertex rows, edge rows) that reads the pattern's
    column indices but no values; a block (N, k) is one tfem_p2_apply_rows_multi call, column j with
    the bits of the single launch on column j."""

    def __init__(self, n, dtype, device, assemble, engine=None, alpha=0.0, beta=0.0, symmetric=True,
                 programs=None, p2_rows=False, matrix_free=None, fields=None, field_sources=None):
        self.shape = (int(n), int(n))
        self.dtype = dtype
        self.device = device
        self._assemble = assemble  # () -> CSRMatrix on `device`: the assembled form
        self._engine = engine      # None: the CSR path only
        self.alpha, self.beta = float(alpha), float(beta)
        #: (kappa, c) source programs of a variable-coefficient form (None: constant coefficients)
        self._programs = programs
        #: (kappa, c) coefficient DATA, (E, Q | 1) on the engine's device (None: no data), and the
        #: tensors the caller marked (the autograd leaves or their descendants)
        self._fields = fields
        self._field_sources = field_sources if field_sources is not None else (None, None)
        self._symmetric = symmetric
        self._csr = None
        #: P2 over the row plan (tfem_p2_apply_rows) instead of P1 over the ring plan
        self._p2_rows = bool(p2_rows)
        # matrix_free True: decided by the caller, who has built the plan (layout="matrix_free")
        self._matrix_free = (matrix_free if engine is not None else False)

    @classmethod
    def from_csr(cls, csr, symmetric=False):
        return cls(csr.shape[0], csr.dtype, csr.device, lambda: csr, symmetric=symmetric)

    @property
    def matrix_free(self):
        """Decided on first use: the ring plan is built then (as for an assembly), not before."""
        if self._matrix_free is None:
            try:
                if self._fields is not None:
                    self._matrix_free = self._engine.field_refusal(self.beta, "apply") is None
                elif self._programs is not None:
                    self._matrix_free = self._engine.supports_coefficients()
                else:
                    self._matrix_free = self._engine.ring_plan() is not None
            except NotImplementedError:
                self._matrix_free = False
        return self._matrix_free

    def _rows(self, u):
        """K u (u None: diag K) by one launch in the engine's numbering."""
        if self._fields is not None:
            return self._engine._apply_rings_field(self.alpha, self.beta, self._fields, u)
        if self._programs is not None:
            return self._engine._apply_rings_coef(self.alpha, self.beta, *self._programs, u)
        if self._p2_rows:
            return self._engine._apply_p2_rows(self.alpha, self.beta, u)
        return self._engine._apply_rings(self.alpha, self.beta, u)

    def to_csr(self):
        """The assembled operator (CSRMatrix) through the existing assembly path (cached)."""
        if self._csr is None:
            self._csr = self._assemble()
        return self._csr

    def _check(self, x):
        if _is_block(x):
            if x.shape[0] != self.shape[1]:
                raise ValueError(f"matvec: x has {x.shape[0]} rows, the operator {self.shape[1]} columns")
            return x
        flat = x.reshape(-1)
        if flat.shape[0] != self.shape[1]:
            raise ValueError(f"matvec: x has {flat.shape[0]} entries, the operator {self.shape[1]} columns")
        return flat

    def _apply(self, x):
        flat = self._check(x)
        if self.matrix_free:
            engine = self._engine
            if self._fields is not None:
                y = engine._home(engine.apply_field(self.alpha, self.beta, self._fields, flat))
            elif self._programs is not None:
                y = engine._home(engine.apply_coef(self.alpha, self.beta, *self._programs, flat))
            else:
                y = engine._home(engine.apply(self.alpha, self.beta, flat))
        else:
            y = self.to_csr().matvec(flat.to(self.device))
        return y.reshape(x.shape)

    def matvec(self, x):
        """K x for x of shape (N,), (N, 1) or (N, k); differentiable in x for symmetric forms, and in
        the values of coefficient data that require grad."""
        if torch.is_grad_enabled() and self.matrix_free and any(
                s is not None and s.requires_grad for s in self._field_sources):
            n_elems, n_quad = self._engine.n_elems, self._engine.n_quad
            views = [None if s is None else s.reshape(n_elems, -1).expand(n_elems, n_quad) for s in self._field_sources]
            return _FieldApply.apply(x, *views, self)
        if x.requires_grad and torch.is_grad_enabled():
            if not self._symmetric:
                raise NotImplementedError("matvec: the gradient needs the transpose of a non-symmetric form")
            return _OperatorApply.apply(x, self)
        return self._apply(x)

    def __matmul__(self, x):
        return self.matvec(x)

    def diagonal(self):
        """diag(K), shape (N,)."""
        if self.matrix_free:
            engine = self._engine
            if self._fields is not None:
                return engine._home(engine.operator_diagonal_field(self.alpha, self.beta, self._fields))
            if self._programs is not None:
                return engine._home(engine.operator_diagonal_coef(self.alpha, self.beta, *self._programs))
            return engine._home(engine.operator_diagonal(self.alpha, self.beta))
        return self.to_csr().diagonal()

    def _rows_into(self):
        """``matvec_into`` of ``fused_conjugate_gradients``: the launch of ``_rows`` into a given
        buffer, in the engine's numbering."""
        programs, fields = self._programs, self._fields
        return _into(lambda u, out: self._engine._prepared_apply(self.alpha, self.beta, u, out, programs, fields))

    def solve_cg(self, b, free=None, x0=None, rtol=1e-12, maxiter=None, loop=None):
        """Jacobi-preconditioned CG on the DoFs ``free``: the contract and the results of
        ``CSRMatrix.solve_cg`` (``loop`` included).  Matrix-free, every iteration is one apply launch
        (and, in the fused loop, three tfem_cg_* launches), and the loop runs in the engine's
        numbering (vectors translated once at the boundary)."""
        if not self.matrix_free:
            return self.to_csr().solve_cg(b, free, x0, rtol, maxiter, loop)
        which = _cg_loop(loop, self._engine.device)
        engine = self._engine
        dev, dtype = engine.device, engine.dtype
        inv = None if engine._inv is None else engine._inv.to(dev)

        def inward(v):
            return None if v is None else engine._dofs_in(v.to(dev, dtype).reshape(-1))

        free_e = None
        if free is not None:
            free_e = free.to(dev).reshape(-1)
            if inv is not None:
                free_e = inv[free_e]
        if which == "fused":
            x, it, res = fused_conjugate_gradients(
                self._rows_into(), self._rows(None), inward(b), free_e, inward(x0), rtol, maxiter,
            )
        else:
            x, it, res = conjugate_gradients(
                self._rows, self._rows(None),
                inward(b), free_e, inward(x0), rtol, maxiter,
            )
        return engine._home(engine._dofs_out(x)).reshape(b.shape), it, res

    def solve_cg_multi(self, B, free=None, X0=None, rtol=1e-12, maxiter=None, loop=None):
        """``solve_cg`` for the k columns of B (N, k) at once: one block apply per iteration
        (``conjugate_gradients_multi``, on the GPU ``fused_conjugate_gradients``; ``loop`` as in
        ``solve_cg``), in the engine's numbering when matrix-free.  Returns
        (X (N, k), iterations (k,), relative residuals (k,))."""
        if not self.matrix_free:
            return self.to_csr().solve_cg_multi(B, free, X0, rtol, maxiter, loop)
        which = _cg_loop(loop, self._engine.device)
        engine = self._engine
        dev, dtype = engine.device, engine.dtype
        inv = None if engine._inv is None else engine._inv.to(dev)

        def inward(v):
            if v is None:
                return None
            v = v.to(dev, dtype)
            return v if inv is None else v.index_select(0, engine._perm.to(dev))

        free_e = None
        if free is not None:
            free_e = free.to(dev).reshape(-1)
            if inv is not None:
                free_e = inv[free_e]
        if which == "fused":
            if B.dim() != 2 or B.shape[0] != self.shape[0]:
                raise ValueError(f"solve_cg_multi: B must have shape ({self.shape[0]}, k)")
            solver, matvec = fused_conjugate_gradients, self._rows_into()
        else:
            solver, matvec = conjugate_gradients_multi, self._rows
        X, it, res = solver(matvec, self._rows(None), inward(B), free_e, inward(X0), rtol, maxiter)
        if inv is not None:
            X = X.index_select(0, inv)
        return engine._home(X), it, res

    def __repr__(self):
        kind = "matrix-free" if self._matrix_free else ("CSR" if self._matrix_free is False else "unresolved")
        if self._programs is not None and self._matrix_free is not False:
            kind = "matrix-free, variable coefficients" if self._matrix_free else "unresolved, variable coefficients"
        if self._p2_rows and self._matrix_free:
            kind = "matrix-free, P2 rows"
        if self._fields is not None and self._matrix_free is not False:
            kind = "matrix-free, coefficient data" if self._matrix_free else "unresolved, coefficient data"
        return f"FormOperator(shape={self.shape}, dtype={self.dtype}, device={self.device}, {kind})"
