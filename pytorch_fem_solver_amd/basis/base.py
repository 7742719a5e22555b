"""``AbstractBasis``: the reference's integration API on top of the HIP assembly path.

Mirror of reference torch_fem/basis/abstract_basis.py.  What the reference does with a
chain of torch expressions per call -- geometry at quadrature points (:42-63),
``(integrand * dx).sum(-3)`` (:83,:104,:72) and ``index_put_(accumulate=True)`` into a
dense target (:81-91,:102-110) -- happens here inside libtfem_hip (csrc/), for tensors
on the GPU directly and for CPU tensors by staging through the GPU.  No torch
implementation of those steps exists in this class.
"""

from __future__ import annotations

import abc
import os
import warnings

import torch

from .. import _native
from ..sparse import CSRMatrix, FormOperator
from . import forms

#: above this many bytes the dense (N, N) layout of the reference is not materialised
DENSE_LIMIT_BYTES = int(os.environ.get("TORCH_FEM_DENSE_LIMIT_BYTES", str(4 << 30)))


class _LinearFormFunction(torch.autograd.Function):
    """Differentiable quadrature-reduce + scatter (the VPINN training step differentiates
    through integrate_linear_form, reference examples/example_weak.py:132-152)."""

    @staticmethod
    def forward(ctx, integrand, basis):
        ctx.basis = basis
        ctx.in_shape = integrand.shape
        ctx.in_device = integrand.device
        return basis._engine.reduce_linear(integrand.detach(), basis._dx)

    @staticmethod
    def backward(ctx, grad_out):
        basis = ctx.basis
        # the caller's DoF ids (the engine may work in a renumbering of its own)
        conn = basis._global_dofs4elements.to(grad_out.device).long()
        conn = conn.reshape(-1, conn.shape[-1])
        dx = basis._dx.to(grad_out.device)
        lead = tuple(dx.shape[:-3])
        g = grad_out.reshape(-1)[conn].reshape(lead + (1, conn.shape[-1], 1))
        grad_integrand = g * dx
        return grad_integrand.sum_to_size(ctx.in_shape).to(ctx.in_device), None


class _FunctionalFunction(torch.autograd.Function):
    """Differentiable per-element integral (abstract_basis.py:65-72): the reference's
    ``(f * dx).sum(-3).sum(-2)`` stays in the autograd graph and is the training loss of
    examples/example_loss_is_error.py:101-106, example_jump.py:147-151.  Forward: one
    tfem_reduce_functional launch; backward: the cotangent of every element times dx."""

    @staticmethod
    def forward(ctx, integrand, basis):
        ctx.basis = basis
        ctx.in_shape = integrand.shape
        ctx.in_device = integrand.device
        return basis._engine.reduce_functional(integrand.detach(), basis._dx)

    @staticmethod
    def backward(ctx, grad_out):
        dx = ctx.basis._dx.to(grad_out.device)  # (..., Q, 1, 1)
        full = torch.broadcast_shapes(tuple(ctx.in_shape), tuple(dx.shape))
        grad_integrand = (grad_out[..., None, None] * dx).expand(full)
        return grad_integrand.sum_to_size(ctx.in_shape).to(ctx.in_device), None


class _ResidualFormFunction(torch.autograd.Function):
    """The VPINN residual form ``f * v + s * v_grad @ g.mT`` (examples/example_weak.py:64-75), fused:
    forward = tfem_p1_residual_local + gather, backward = tfem_p1_residual_backward; neither
    direction materialises the (N_T, Q, 3, 1) integrand.  `coefficient` is a tensor (..., Q, 1, 1) or
    None (then `program`, a source program, or no source at all); `flux` a tensor (..., Q, 1, 2)."""

    @staticmethod
    def forward(ctx, coefficient, flux, basis, program, flux_sign):
        engine = basis._engine
        fq = None
        if coefficient is not None:
            fq = basis._source_values(coefficient.detach().to(engine.device, engine.dtype))
        ctx.basis, ctx.flux_sign = basis, flux_sign
        ctx.coefficient_meta = None if coefficient is None else (coefficient.shape, coefficient.device)
        ctx.flux_meta = (flux.shape, flux.device)
        return engine.residual(fq, program, engine._flat_flux(flux), flux_sign)

    @staticmethod
    def backward(ctx, grad_out):
        engine = ctx.basis._engine
        want_fq = ctx.coefficient_meta is not None and ctx.needs_input_grad[0]
        want_flux = ctx.needs_input_grad[1]
        grad_fq, grad_flux = engine.residual_backward(grad_out, ctx.flux_sign, want_fq, want_flux)
        lead = tuple(engine.lead_shape)
        g_coefficient = g_flux = None
        if want_fq:
            shape, device = ctx.coefficient_meta
            g_coefficient = grad_fq.reshape(lead + (engine.n_quad, 1, 1)).sum_to_size(shape).to(device)
        if want_flux:
            shape, device = ctx.flux_meta
            g_flux = grad_flux.reshape(lead + (engine.n_quad, 1, 2)).sum_to_size(shape).to(device)
        return g_coefficient, g_flux, None, None, None


#: what a stored operator says to an integrand (or coefficient data) that carries autograd history
_NOT_DIFFERENTIABLE = (
    "integrate_bilinear_form: the integrand carries autograd history, but the "
    "assembled operator is written by the HIP kernels and is not differentiable; "
    "detach() the integrand, or differentiate a linear form / functional instead"
)


class AbstractBasis(abc.ABC):
    """Finite-element basis on a mesh (abstract_basis.py:10-40)."""

    #: geometry attributes computed on first access by one tfem_tri_geometry launch
    _LAZY = ("v_grad", "integration_points", "_dx", "_inv_map_jacobian")

    def __init__(self, mesh, element):
        self._element = element
        self.mesh = mesh
        self._geometry_cache = {}
        (
            self._coords4global_dofs,
            self._global_dofs4elements,
            self._nodes4boundary_dofs,
            self._coords4elements,
        ) = self._compute_dofs(mesh, element)
        self._basis_parameters = self._compute_basis_parameters(
            self._coords4global_dofs, self._global_dofs4elements, self._nodes4boundary_dofs
        )
        self._engine = self._make_engine(mesh, element)
        self.v = self._compute_shape_values(element)

    # ---- lazily materialised geometry cache (abstract_basis.py:42-63) -------------
    def __getattr__(self, name):
        if name in AbstractBasis._LAZY:
            cache = self.__dict__.get("_geometry_cache")
            if cache is None:
                raise AttributeError(name)
            if name not in cache:
                cache.update(self._compute_integral_values(self.mesh, self._element))
            return cache[name]
        raise AttributeError(f"{type(self).__name__!s} has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in AbstractBasis._LAZY:
            self._geometry_cache[name] = value
        else:
            object.__setattr__(self, name, value)

    def _compute_shape_values(self, element):
        bar = element.compute_barycentric_coordinates(element.gaussian_nodes)
        v, _ = element.compute_shape_functions(
            bar, torch.zeros((1, 1, 2, 2), dtype=bar.dtype, device=bar.device)
        )
        return v

    @abc.abstractmethod
    def _make_engine(self, mesh, element):
        ...

    @abc.abstractmethod
    def _compute_integral_values(self, mesh, element) -> dict:
        """Return {'v_grad','integration_points','_dx','_inv_map_jacobian'} in the
        reference's shapes."""

    @abc.abstractmethod
    def _compute_dofs(self, mesh, element):
        ...

    @abc.abstractmethod
    def _compute_basis_parameters(self, coords4global_dofs, global_dofs4elements, nodes4boundary_dofs):
        ...

    # ---- integration API ---------------------------------------------------------------
    def coefficient(self, values):
        """Mark ``values`` as a coefficient field of this basis (``forms.CoefficientField``): values at
        the integration points, ``(E, Q, 1, 1)`` or ``(E, Q)``, or one per element, ``(E, 1, 1, 1)``,
        ``(E, 1)`` or ``(E,)``.  ``field * (v_grad @ v_grad.mT) + field * (v @ v.mT)`` in a bilinear
        form is then assembled, applied and differentiated in the values by the coefficient-data
        launches on a P1 basis; anywhere else the field is the tensor ``(E, Q | 1, 1, 1)``."""
        return forms.CoefficientField(self, values)

    def integrate_functional(self, function, *args, **kwargs):
        """Per-element integral of ``function(basis, ...)`` (abstract_basis.py:65-72);
        differentiable in the integrand."""
        integrand = forms.materialize(forms.trace(function, self, args, kwargs))
        if integrand.requires_grad and torch.is_grad_enabled():
            out = _FunctionalFunction.apply(integrand, self)
        else:
            out = self._engine.reduce_functional(integrand.detach(), self._dx)
        return self._engine._home(out)

    def integrate_bilinear_form(self, function, *args, layout=None, **kwargs):
        """Global operator of a bilinear form (abstract_basis.py:74-93).

        ``layout``: "dense" (the reference's (N, N) tensor), "csr" (``CSRMatrix``), "operator"
        (``FormOperator``: to apply and solve with; matrix-free for ``alpha * v_grad @ v_grad.mT +
        beta * v @ v.mT`` on a P1 basis with a ring plan -- also with coefficients ``kappa(x, y)``,
        ``c(x, y)`` written as expressions of the integration points' columns in front of the two
        terms, or with coefficient DATA ``basis.coefficient(values)`` there -- the assembled CSR
        otherwise), "matrix_free" (a ``FormOperator`` that never stores K,
        decided here: what "operator" serves matrix-free on P1, and the same form on a P2 basis over
        its row plan; NotImplementedError naming the reason where no such launch applies) or None =
        dense while it fits ``DENSE_LIMIT_BYTES``, CSR beyond.
        """
        return self._bilinear_of(forms.trace(function, self, args, kwargs), layout)

    def _bilinear_of(self, expr, layout):
        """integrate_bilinear_form for the traced expression (the callable has run)."""
        if layout == "matrix_free":
            return self._matrix_free_operator(expr)
        if isinstance(expr, forms.BilinearExpr) and expr.has_coefficients:
            out = self._field_form(expr, layout) if expr.has_data else self._coefficient_form(expr, layout)
            if out is not None:
                return out
            expr = forms.materialize(expr)  # no launch for it on this basis: the integrand, with torch
        if layout == "operator" and isinstance(expr, forms.BilinearExpr) and self._engine.may_apply_matrix_free():
            # nothing is launched here: the ring plan is built on first use, and a basis whose fans
            # turn out to have no ring form assembles the CSR operator then
            engine, alpha, beta = self._engine, expr.alpha, expr.beta
            return FormOperator(
                engine.n_dofs, engine.dtype, engine.home,
                lambda: engine.wrap_csr_home(engine.bilinear(alpha, beta)), engine=engine, alpha=alpha, beta=beta,
            )
        if isinstance(expr, forms.BilinearExpr):
            vals = self._engine.bilinear(expr.alpha, expr.beta)
        else:
            vals = self._reduce_integrand(forms.materialize(expr))
        return self._finish_matrix(vals, layout)

    def _matrix_free_operator(self, expr):
        """layout="matrix_free": a FormOperator that never stores K -- the plan is built here -- or
        NotImplementedError saying why this form on this basis has no such launch."""
        def refuse(why):
            raise NotImplementedError(f'layout="matrix_free": {why}')

        engine = self._engine
        if engine.n_fractures > 0 or engine._host_conn_geo.dim() != 2:
            refuse("a fracture basis (batched meshes) has no row plan")
        if not isinstance(expr, forms.BilinearExpr):
            refuse("the integrand is not alpha * v_grad @ v_grad.mT + beta * v @ v.mT (with coefficient "
                   "expressions of the integration points in front of the terms on P1)")
        if engine.poly_order not in (1, 2):
            refuse(f"no row plan for polynomial order {engine.poly_order}")
        alpha, beta = expr.alpha, expr.beta
        if engine.poly_order == 2:
            if expr.has_coefficients:
                refuse("coefficient fields on a P2 basis (the P2 row launch takes constant coefficients)")
            if not engine.may_apply_p2_matrix_free():
                refuse(f"TFEM_KERNEL={engine.kernel} selects a path without the P2 row plan")
            if engine.p2_plan() is None:
                refuse("this P2 basis has no row plan: a DoF numbering without locality, or a vertex with "
                       "more than 15 neighbours")
            return FormOperator(
                engine.n_dofs, engine.dtype, engine.home,
                lambda: engine.wrap_csr_home(engine.bilinear(alpha, beta)), engine=engine, alpha=alpha, beta=beta,
                p2_rows=True, matrix_free=True,
            )
        if not engine.may_apply_matrix_free():
            if engine.kernel not in ("auto", "rings"):
                refuse(f"TFEM_KERNEL={engine.kernel} selects a path without the ring plan")
            refuse("the DoFs of this P1 basis are not the mesh's vertices: no ring plan")
        if expr.has_coefficients and expr.has_data:
            why = engine.field_refusal(beta, "apply")
            if why is not None:
                refuse(f"coefficient data: {why}")
            return self._field_operator(expr)
        if expr.has_coefficients:
            if not engine.supports_source():
                refuse("this basis takes no source programs for the coefficient fields")
            programs = self._coefficient_programs(expr)
            if programs is None:
                refuse("a coefficient field does not fit a source program")
            if not engine.supports_coefficients():
                refuse("no ring plan for the coefficient launch (fans without ring form, or long rows)")

            def assemble():
                return engine.wrap_csr_home(engine.bilinear_coef(alpha, beta, *programs))

            return FormOperator(engine.n_dofs, engine.dtype, engine.home, assemble, engine=engine, alpha=alpha,
                                beta=beta, programs=programs, matrix_free=True)
        if engine.ring_plan() is None:
            refuse("the fans of this P1 mesh have no ring form: no ring plan")
        return FormOperator(
            engine.n_dofs, engine.dtype, engine.home,
            lambda: engine.wrap_csr_home(engine.bilinear(alpha, beta)), engine=engine, alpha=alpha, beta=beta,
            matrix_free=True,
        )

    def _reduce_integrand(self, integrand):
        """CSR values of a materialised bilinear integrand: the generic reduce + scatter kernels."""
        if integrand.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(_NOT_DIFFERENTIABLE)
        return self._engine.reduce_bilinear(integrand, self._dx)

    def _coefficient_programs(self, expr):
        """(kappa, c) source programs of a traced variable-coefficient form, or None when a field
        does not fit a program (said once per basis) or the basis takes no source programs."""
        programs = []
        for field in (expr.kappa, expr.c):
            program = None
            if field is not None:
                program = self._source_program(field)
                if program is None:
                    return None
            programs.append(program)
        return tuple(programs)

    def _coefficient_form(self, expr, layout):
        """``alpha * kappa * stiffness + beta * c * mass`` through the coefficient launches
        (tfem_p1_rings_coef / tfem_p1_apply_rings_coef), or None when they do not apply."""
        engine, alpha, beta = self._engine, expr.alpha, expr.beta
        if not (engine.may_apply_matrix_free() and engine.supports_source()):
            return None
        if layout == "operator":
            # nothing is launched and no plan is built here (as for constant coefficients): the operator
            # decides on first use; without a plan for the launch it assembles the integrand's CSR
            programs = self._coefficient_programs(expr)
            if programs is None:
                return None

            def assemble():
                vals = engine.bilinear_coef(alpha, beta, *programs)
                if vals is None:
                    vals = self._reduce_integrand(forms.materialize(expr))
                return engine.wrap_csr_home(vals)

            return FormOperator(engine.n_dofs, engine.dtype, engine.home, assemble, engine=engine, alpha=alpha,
                                beta=beta, programs=programs)
        if not engine.supports_coefficients():  # builds the ring plan, as an assembly does
            return None
        programs = self._coefficient_programs(expr)
        if programs is None:
            return None
        return self._finish_matrix(engine.bilinear_coef(alpha, beta, *programs), layout)

    # ---- coefficient data (forms.CoefficientField) ---------------------------------------
    def _field_data(self, expr):
        """((kappa, c) values (E, Q | 1) on the engine's device, None: the constant 1; the tensors of
        the marked fields, for autograd).  A coefficient PROGRAM on the other term becomes values once
        (tfem_source_eval; torch where it does not fit a program)."""
        engine = self._engine
        values, sources = [], []
        for field in (expr.kappa, expr.c):
            value = source = None
            if isinstance(field, forms.CoefficientField):
                source = field.tensor
                value = source.detach().to(engine.device, engine.dtype).reshape(engine.n_elems, -1).contiguous()
            elif field is not None:
                program = self._source_program(field)
                if program is not None:
                    value = engine.source_values(program)
                else:
                    value = self._source_values(field.materialize()).to(engine.device, engine.dtype).contiguous()
            values.append(value)
            sources.append(source)
        return tuple(values), tuple(sources)

    def _field_operator(self, expr):
        """The matrix-free operator of a form with coefficient data (the caller has checked that the
        apply launch takes this basis)."""
        engine, alpha, beta = self._engine, expr.alpha, expr.beta
        fields, sources = self._field_data(expr)

        def assemble():
            vals = engine.bilinear_field(alpha, beta, fields)
            if vals is None:  # no store launch for this plan: the integrand, with torch
                with torch.no_grad():
                    vals = self._reduce_integrand(forms.materialize(expr))
            return engine.wrap_csr_home(vals)

        return FormOperator(engine.n_dofs, engine.dtype, engine.home, assemble, engine=engine, alpha=alpha,
                            beta=beta, fields=fields, field_sources=sources, matrix_free=True)

    def _field_form(self, expr, layout):
        """``alpha * kappa * stiffness + beta * c * mass`` with coefficient DATA through the data
        launches (tfem_p1_rings_field / tfem_p1_apply_rings_field), or None when they do not apply."""
        engine = self._engine
        if layout == "operator":
            if engine.field_refusal(expr.beta, "apply") is not None:
                return None
            return self._field_operator(expr)
        if engine.field_refusal(expr.beta, "store") is not None:
            return None
        fields, sources = self._field_data(expr)
        if torch.is_grad_enabled() and any(s is not None and s.requires_grad for s in sources):
            raise NotImplementedError(_NOT_DIFFERENTIABLE)
        return self._finish_matrix(engine.bilinear_field(expr.alpha, expr.beta, fields), layout)

    def assemble_system(self, bilinear, linear, *args, layout=None, **kwargs):
        """``(integrate_bilinear_form(bilinear, ...), integrate_linear_form(linear, ...))`` -- the
        pair every solve of the reference asks for (examples/example_fractures_fem.py:239-241,
        tests/test_assembly.py:86-93) -- in ONE launch when both callables are in the fused
        vocabulary: ``alpha * v_grad @ v_grad.mT + beta * v @ v.mT`` and ``f * v`` with ``f`` an
        expression of the integration points (evaluated inside the launch) or a tensor of source
        values.  Anything else: the two calls one after the other, same results."""
        a_expr = forms.trace(bilinear, self, args, kwargs)
        l_expr = forms.trace(linear, self, args, kwargs)
        fused = None
        if isinstance(a_expr, forms.BilinearExpr) and a_expr.has_coefficients:
            # the coefficient K launch, then the load vector's own launch (two launches)
            return self._bilinear_of(a_expr, layout), self._linear_of(l_expr)
        if layout == "matrix_free":  # no K to fuse the load vector with: the two calls
            return self._bilinear_of(a_expr, layout), self._linear_of(l_expr)
        if isinstance(a_expr, forms.BilinearExpr) and isinstance(l_expr, forms.LinearExpr) and l_expr.flux is None:
            coefficient = l_expr.coefficient
            if isinstance(coefficient, forms.SourceExpr):
                program = self._source_program(coefficient)
                if program is not None:
                    fused = self._engine.assemble_system(a_expr.alpha, a_expr.beta, source=program)
                else:
                    coefficient = coefficient.materialize()
            if fused is None and torch.is_tensor(coefficient) and not coefficient.requires_grad:
                values = self._source_values(coefficient)
                if values is not None:
                    fused = self._engine.assemble_system(a_expr.alpha, a_expr.beta, values)
        if fused is None:
            return (self.integrate_bilinear_form(bilinear, *args, layout=layout, **kwargs),
                    self.integrate_linear_form(linear, *args, **kwargs))
        vals, f = fused
        return self._finish_matrix(vals, layout), self._engine._home(f).reshape(-1, 1)

    def _source_program(self, coefficient):
        """The source program of a traced coefficient, or None -- said ONCE per basis when it is the
        program's limits that send the expression to torch (include/tfem_assembly.h: 32 operations,
        a stack of 4): the results are the same, the step then reads 8 Q bytes per element more."""
        if not self._engine.supports_source():
            return None
        program = coefficient.program()
        if program is None and not self.__dict__.get("_warned_source_limits"):
            self.__dict__["_warned_source_limits"] = True
            warnings.warn(
                "the source expression does not fit a source program (more than "
                f"{_native.SOURCE_MAX_OPS} operations or {_native.SOURCE_STACK} values at a time): torch evaluates it at the "
                "cached integration points and the assembly launch reads the values from memory",
                RuntimeWarning, stacklevel=3)
        return program

    def _finish_matrix(self, vals, layout):
        if layout == "operator":  # any form the matrix-free launch does not cover: the assembled CSR
            return FormOperator.from_csr(self._engine.wrap_csr_home(vals))
        matrix = self._engine.wrap_csr(vals)
        n = matrix.shape[0]
        if layout is None:
            layout = "dense" if n * n * vals.element_size() <= DENSE_LIMIT_BYTES else "csr"
        if layout == "csr":
            return self._engine.wrap_csr_home(vals)
        if layout != "dense":
            raise ValueError(f"unknown layout {layout!r}")
        return self._engine._home(matrix.to_dense())

    def integrate_linear_form(self, function, *args, **kwargs):
        """Global vector of a linear form, shape (N, 1) (abstract_basis.py:95-112)."""
        return self._linear_of(forms.trace(function, self, args, kwargs))

    def _linear_of(self, expr):
        """integrate_linear_form for the traced expression (the callable has run)."""
        if isinstance(expr, forms.LinearExpr) and expr.flux is None:
            coefficient = expr.coefficient
            if isinstance(coefficient, forms.SourceExpr):
                # f(x, y) recorded by the tracer: evaluated inside the assembly launch
                program = self._source_program(coefficient)
                if program is not None:
                    return self._engine._home(self._engine.load_source(program)).reshape(-1, 1)
                coefficient = coefficient.materialize()
            if not coefficient.requires_grad:
                values = self._source_values(coefficient)
                if values is not None:
                    return self._engine._home(self._engine.load(values)).reshape(-1, 1)
        if isinstance(expr, forms.LinearExpr) and expr.flux is not None and self._engine.supports_residual():
            out = self._residual_form(expr)
            if out is not None:
                return self._engine._home(out).reshape(-1, 1)
        integrand = forms.materialize(expr)
        if integrand.requires_grad and torch.is_grad_enabled():
            out = _LinearFormFunction.apply(integrand, self)
        else:
            out = self._engine.reduce_linear(integrand.detach(), self._dx)
        return self._engine._home(out).reshape(-1, 1)

    def _residual_form(self, expr):
        """f * v + s * v_grad @ g.mT through the fused residual kernels, or None when the
        operands do not have the reference's shapes (then torch evaluates the integrand)."""
        engine = self._engine
        if engine._flat_flux(expr.flux) is None:
            return None
        coefficient, program = expr.coefficient, None
        if isinstance(coefficient, forms.SourceExpr):
            program = coefficient.program()
            coefficient = None if program is not None else coefficient.materialize()
        if coefficient is not None and self._source_values(coefficient) is None:
            return None
        return _ResidualFormFunction.apply(coefficient, expr.flux, self, program, expr.flux_sign)

    def _source_values(self, coefficient):
        """(E, Q) source values if ``coefficient`` broadcasts to (..., Q, 1, 1), else None."""
        lead = tuple(self._engine.lead_shape)
        want = lead + (self._engine.n_quad, 1, 1)
        try:
            full = torch.broadcast_shapes(tuple(coefficient.shape), want)
        except RuntimeError:
            return None
        if tuple(full) != want:
            return None
        return coefficient.expand(want).reshape(-1, self._engine.n_quad)

    def reduce(self, tensor):
        """Restrict to interior DoFs (abstract_basis.py:114-117)."""
        idx = self._basis_parameters["inner_dofs"]
        if isinstance(tensor, CSRMatrix):
            tensor = tensor.to_dense()
        return tensor[idx, :][:, idx] if tensor.size(-1) != 1 else tensor[idx]

    def reshape_for_assembly(self, local_matrices, form):
        """abstract_basis.py:162-171"""
        if form == "bilinear":
            return local_matrices.reshape(-1)
        if form == "linear":
            return local_matrices.reshape(-1, 1)
        raise NotImplementedError(f"Unknown form type: {format(form)}")

    def solution_tensor(self):
        """Zero vector (N, 1) (abstract_basis.py:173-175)."""
        return torch.zeros(self._basis_parameters["linear_form_shape"])

    #: a CSR operator with more rows than this is solved by conjugate gradients on the CSR
    #: values instead of the reference's dense solve (its dense copy would not fit)
    DENSE_SOLVE_LIMIT = 20000

    def solve(self, matrix, solution, vector, only_inner_dofs=True, method=None):
        """Dense solve on the interior DoFs (abstract_basis.py:177-195).  A CSRMatrix beyond
        DENSE_SOLVE_LIMIT rows (or method="cg") is solved by Jacobi-preconditioned conjugate
        gradients on the CSR values (CSRMatrix.solve_cg; symmetric positive definite forms):
        the step after the assembly for operators the reference cannot hold.
        A FormOperator (layout="operator") is always solved by CG, matrix-free where it is.
        With ``solution`` and ``vector`` of shape (N, k), k >= 2, the CG path solves the k systems
        together (``solve_cg_multi``)."""
        if isinstance(matrix, FormOperator) or (
                isinstance(matrix, CSRMatrix) and (method == "cg" or (method is None and matrix.shape[0] > self.DENSE_SOLVE_LIMIT))):
            free = self._basis_parameters["inner_dofs"] if only_inner_dofs is True else None
            if vector.dim() == 2 and vector.shape[1] > 1:  # (N, k): the k systems in one block CG
                x, _, _ = matrix.solve_cg_multi(vector, free=free)
            else:
                x, _, _ = matrix.solve_cg(vector, free=free)
            if free is None:
                solution += x.reshape(solution.shape).to(solution.device)
            else:
                solution[free] += x.reshape(solution.shape)[free].to(solution.device)
            return solution
        if only_inner_dofs is True:
            matrix = self.reduce(matrix)
            vector = self.reduce(vector)
        elif isinstance(matrix, CSRMatrix):
            matrix = matrix.to_dense()
        solution[self._basis_parameters["inner_dofs"]] += torch.linalg.solve(matrix, vector)
        return solution


class LazyIndexDict(dict):
    """``_basis_parameters`` with the 2 x (n^2 N_T) dense scatter indices of the reference
    (basis.py:73-76) built only if somebody asks for them."""

    def __init__(self, *args, connectivity=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._connectivity = connectivity

    def __missing__(self, key):
        if key != "bilinear_form_idx":
            raise KeyError(key)
        conn = self._connectivity.reshape(-1, self._connectivity.shape[-1])
        n = conn.shape[-1]
        value = (conn.repeat(1, n).reshape(-1), conn.repeat_interleave(n).reshape(-1))
        self[key] = value
        return value
