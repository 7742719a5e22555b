/*
 * tfem_assembly.h -- C ABI of the MI355X (gfx950) element-wise FEM assembly path.
 *
 * Drop-in boundary for the hot path of Nicolas-Zamorano/pytorch_fem_solver
 * (package torch_fem).  The reference has no FFI: the path is a sequence of
 * torch tensor expressions inside AbstractBasis (torch_fem/basis/
 * abstract_basis.py:42-112).  Each entry point below names the reference
 * lines it replaces.  All signatures are plain pointers and sizes: no torch
 * types cross this boundary.
 *
 * Conventions
 *   - "device" pointers are HIP device pointers valid on the current device;
 *     "host" pointers are ordinary process memory.  The library never
 *     allocates or frees caller-visible memory and keeps no global state (the
 *     only library-owned object is the opaque tile-plan handle, below).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Device entry points only enqueue work; they never synchronise.
 *   - every function returns a tfem_status (0 = success).  tfem_last_error()
 *     returns a thread-local human-readable message for the last failure.
 *   - connectivity is row-major (n_elems, n_local) with 4- or 8-byte signed
 *     indices (`idx_bytes`), as the reference keeps it (int32 from MeshTri,
 *     abstract_mesh.py:51-54; int64 from FractureBasis, fracture_basis.py:80).
 *   - real type: `real_bytes` 8 = double (the graded path), 4 = float.
 *   - scatter convention (reference basis.py:73-76 + abstract_basis.py:166-167):
 *     local[i][j] is ADDED to A[conn[e][j]][conn[e][i]].
 *   - quadrature: `quad_order` 1..4 selects the 1/3/4/6-point triangle rule
 *     with the literals of element_tri.py:77-130.
 */
#ifndef TFEM_ASSEMBLY_H
#define TFEM_ASSEMBLY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFEM_ABI_VERSION 2

typedef enum tfem_status {
  TFEM_OK = 0,
  TFEM_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, negative size, bad idx_bytes ... */
  TFEM_ERR_UNSUPPORTED = 2,      /* quadrature / polynomial order the reference raises on */
  TFEM_ERR_HIP = 3,              /* a HIP runtime call failed */
  TFEM_ERR_INDEX_RANGE = 4,      /* connectivity entry outside [0, n_dofs) or nnz >= 2^31 */
  TFEM_ERR_NO_DEVICE = 5         /* no gfx950 device visible */
} tfem_status;

int tfem_abi_version(void);
const char *tfem_status_string(int status);
const char *tfem_last_error(void);
/* Number of visible HIP devices (0 when none); never fails. */
int tfem_device_count(void);
/* Number of quadrature points of `quad_order` (1,3,4,6), or 0 if unsupported.
 * Replaces the shape of ElementTri._compute_gauss_values (element_tri.py:77-130). */
int tfem_quadrature_size(int quad_order);
/* Copy the rule: nodes (Q,2) and weights (Q) as doubles (host pointers). */
int tfem_quadrature_rule(int quad_order, double *nodes_host, double *weights_host);

/* ------------------------------------------------------------------------- *
 * Symbolic phase (HOST memory, once per mesh).
 * Replaces Basis._compute_basis_parameters (basis.py:64-85): instead of the
 * 2 x (n^2 N_T) index tensors for a dense index_put_, it produces the CSR
 * pattern of the operator and, per element entry, the CSR position it adds to.
 * ------------------------------------------------------------------------- */

/* Pass 1: rowptr_host[n_dofs+1] (int64) and *nnz_host. */
int tfem_csr_symbolic_count(const void *conn_host, int idx_bytes, int64_t n_elems,
                            int n_local, int64_t n_dofs, int64_t *rowptr_host,
                            int64_t *nnz_host);
/* Pass 2: colind_host[nnz] (int32, ascending inside each row) and
 * slots_host[n_elems*n_local*n_local] (int32): slots[e][i][j] = CSR position of
 * (row conn[e][j], col conn[e][i]).  `rowptr_host` is the output of pass 1. */
int tfem_csr_symbolic_fill(const void *conn_host, int idx_bytes, int64_t n_elems,
                           int n_local, int64_t n_dofs, const int64_t *rowptr_host,
                           int32_t *colind_host, int32_t *slots_host);

/* The same in one pass (the pattern is built once, HOST, multi-threaded: TFEM_HOST_THREADS):
 *   create : builds the pattern, returns a handle (library memory; release with _destroy) and nnz;
 *            conn_host must stay valid until export
 *   export : rowptr_host[n_dofs+1], colind_host[nnz] (caller-owned)
 *   slots  : slots_host[n_elems*n_local*n_local] from the exported pattern -- only the scatter /
 *            gather paths need it, the row-form plans do not */
int tfem_csr_pattern_create(const void *conn_host, int idx_bytes, int64_t n_elems, int n_local,
                            int64_t n_dofs, void **pattern_out, int64_t *nnz_host);
int tfem_csr_pattern_export(const void *pattern, int64_t *rowptr_host, int32_t *colind_host);
void tfem_csr_pattern_destroy(void *pattern);
int tfem_csr_symbolic_slots(const void *conn_host, int idx_bytes, int64_t n_elems, int n_local,
                            int64_t n_dofs, const int64_t *rowptr_host, const int32_t *colind_host,
                            int32_t *slots_host);

/* ------------------------------------------------------------------------- *
 * Geometry cache (DEVICE).  Replaces AbstractBasis._compute_integral_values
 * (abstract_basis.py:42-63) with Basis._compute_jacobian_map /
 * _compute_integration_points / _compute_integral_weights (basis.py:87-96) and
 * ElementTri.compute_det_and_inv_map / compute_shape_functions
 * (element_tri.py:28-75,132-145), fused with the X[conn] gather
 * (abstract_mesh.py:257-262).  Any output pointer may be NULL (skipped).
 *   coords   (n_verts, 2)            conn (n_elems, 3) vertex ids
 *   v_grad   P1: (n_elems, 3, 2)     P2: (n_elems, Q, 6, 2)
 *   dx       (n_elems, Q)            = 0.5 * w_q * det   (signed det)
 *   points   (n_elems, Q, 2)         inv_jac (n_elems, 2, 2)
 * ------------------------------------------------------------------------- */
int tfem_tri_geometry(const void *coords, int real_bytes, const void *conn, int idx_bytes,
                      int64_t n_elems, int64_t n_verts, int poly_order, int quad_order,
                      void *v_grad, void *dx, void *points, void *inv_jac, void *stream);

/* ------------------------------------------------------------------------- *
 * Fused bilinear forms (DEVICE): alpha * grad(u).grad(v) + beta * u v,
 * i.e. the integrands `v_grad @ v_grad.mT`, `v @ v.mT` and their sum
 * (tests/test_assembly.py:68-73, examples/example_fractures_fem.py:112-116),
 * integrated as abstract_basis.py:83 and scattered as :87-91, gather fused.
 *   conn_geo  (n_elems, 3) vertex ids into coords (geometry)
 *   slots     (n_elems, n, n) from tfem_csr_symbolic_fill, n = 3 (P1) or 6 (P2)
 *   vals      (nnz) CSR values; OVERWRITTEN (zero-filled by this call, then summed)
 *   slots == NULL: LOCAL-BLOCK mode -- vals (n*n, n_elems) receives the element blocks
 *             entry-major (vals[(i*n+j) * n_elems + e] = local[e][i][j]), nnz = n*n*n_elems;
 *             tfem_csr_gather then forms the CSR values without atomics.
 * Fracture variant (fracture_basis.py:20-26,189-197): if `frac_pinv` is not NULL
 * the elements are `n_fractures` consecutive groups of n_elems/n_fractures; the
 * reference gradients are post-multiplied by frac_pinv[f] (2x3) and dx by
 * frac_det[f].
 * ------------------------------------------------------------------------- */
int tfem_tri_bilinear_csr(const void *coords, int real_bytes, const void *conn_geo,
                          int idx_bytes, int64_t n_elems, int64_t n_verts, int poly_order,
                          int quad_order, double alpha, double beta, const int32_t *slots,
                          void *vals, int64_t nnz, const void *frac_pinv,
                          const void *frac_det, int n_fractures, int64_t coords_per_fracture,
                          void *stream);

/* Fused linear form f(x_q) * v (tests/test_assembly.py:79-84): `fq` (n_elems, Q) are
 * the user's source values at the integration points.  out (n_dofs) is overwritten.
 * conn_dof (n_elems, n) are the global DoF ids (P1: n = 3, may equal conn_geo).
 * conn_dof == NULL: LOCAL-VECTOR mode -- out (n, n_elems) receives the element vectors
 * entry-major (out[i * n_elems + e]), n_dofs = n * n_elems; tfem_csr_gather with the gather
 * map of conn_dof (tfem_csr_gather_map(conn_dof, n_elems, n, n_dofs, ...)) then forms the
 * vector without atomics, in the reference's accumulation order. */
int tfem_tri_load_vector(const void *coords, int real_bytes, const void *conn_geo,
                         const void *conn_dof, int idx_bytes, int64_t n_elems,
                         int64_t n_verts, int poly_order, int quad_order, const void *fq,
                         void *out, int64_t n_dofs, const void *frac_det, int n_fractures,
                         int64_t coords_per_fracture, void *stream);

/* ------------------------------------------------------------------------- *
 * Generic quadrature-reduce + scatter (DEVICE) for integrands torch evaluated
 * from an arbitrary user callable.  integrand is (n_elems, Q, n, m) addressed by
 * element strides `es`,`qs` (in elements of the real type; 0 = broadcast) with
 * the inner (n, m) block contiguous.  Computes sum_q integrand * dx exactly as
 * abstract_basis.py:83 / :104 / :72 and
 *   bilinear  (m = n): adds into CSR vals through `slots`      (:87-91)
 *   linear    (m = 1): adds into out[conn_dof]                 (:106-110)
 *   functional(m = 1): writes out[e] = sum_k sum_q (n_inner = n, usually 1)  (:65-72)
 * `vals` / `out` are overwritten.  tfem_reduce_scatter_bilinear with slots == NULL works in
 * LOCAL-BLOCK mode like tfem_tri_bilinear_csr, tfem_reduce_scatter_linear with
 * conn_dof == NULL in LOCAL-VECTOR mode like tfem_tri_load_vector.
 * ------------------------------------------------------------------------- */
int tfem_reduce_scatter_bilinear(const void *integrand, int real_bytes, int64_t es, int64_t qs,
                                 const void *dx, int64_t n_elems, int n_quad, int n_local,
                                 const int32_t *slots, void *vals, int64_t nnz, void *stream);
int tfem_reduce_scatter_linear(const void *integrand, int real_bytes, int64_t es, int64_t qs,
                               const void *dx, int64_t n_elems, int n_quad, int n_local,
                               const void *conn_dof, int idx_bytes, void *out, int64_t n_dofs,
                               void *stream);
int tfem_reduce_functional(const void *integrand, int real_bytes, int64_t es, int64_t qs,
                           const void *dx, int64_t n_elems, int n_quad, int n_inner, void *out,
                           void *stream);

/* Gather map (HOST, once per mesh) and gather (DEVICE): the deterministic, atomic-free form
 * of the scatter abstract_basis.py:87-91.  map: from the slots of tfem_csr_symbolic_fill,
 * gptr_host (nnz+1) int64 and gsrc_host (n_elems*nn) int32 = for every CSR entry the
 * entry-major indices of the local-block entries that add to it, in ascending (element,
 * local entry) order -- the order a sequential index_put_(accumulate=True) adds them in.
 * gather: vals[p] = sum_t local[gsrc[t]], t in [gptr[p], gptr[p+1]); local = the
 * LOCAL-BLOCK output of tfem_tri_bilinear_csr / tfem_reduce_scatter_bilinear. */
int tfem_csr_gather_map(const int32_t *slots_host, int64_t n_elems, int nn, int64_t nnz,
                        int64_t *gptr_host, int32_t *gsrc_host);
int tfem_csr_gather(const void *local, int real_bytes, const int64_t *gptr, const int32_t *gsrc,
                    int64_t nnz, void *vals, void *stream);

/* y = A x for the assembled CSR operator (DEVICE; x, y of n_rows entries).  The consumer of
 * the assembled values: Krylov solves where the reference's dense reduce + torch.linalg.solve
 * (abstract_basis.py:114-117,177-195) cannot go. */
int tfem_csr_spmv(const int64_t *rowptr, const int32_t *colind, const void *vals, int real_bytes,
                  int64_t n_rows, const void *x, void *y, void *stream);

/* Y = A X of the same operator for n_vec vectors at once (DEVICE): x is n_cols x n_vec and y
 * n_rows x n_vec reals, ROW-major (the n_vec values of a DoF consecutive: the layout of the
 * tfem_cg_* launches and of tfem_p1_apply_rings_multi), y[i][c] = sum_p vals[p] * x[colind[p]][c].
 * Replaces, like tfem_csr_spmv, the consumer of the assembled operator on the reference side
 * (abstract_basis.py:177-195) where that operator meets several right-hand sides: one launch for
 * any n_vec >= 1 instead of n_vec launches that each read the matrix.  Eight lanes per row, lane
 * `sub` takes the entries start + sub + 8 t in order, butterfly over 4, 2, 1 -- the arithmetic of
 * tfem_csr_spmv, so column c of y is bit for bit what tfem_csr_spmv gives for the contiguous copy
 * of column c of x, whatever n_vec is.  n_vec in {2, 4, 8} with x and y both aligned to
 * min(16, n_vec * real_bytes) bytes: rows move in accesses of that width; any other width or
 * alignment: passes over 8 columns with scalar accesses, inside the one launch.  Every entry of y
 * is written once (0 for an empty row), nothing else.  No allocation, no synchronisation.
 * Refused before anything is launched (TFEM_ERR_INVALID_ARGUMENT): real_bytes not 4 or 8, a
 * negative n_rows, n_cols or n_vec, NULL rowptr, x (with n_cols > 0) or y, overlapping extents of
 * x and y; TFEM_ERR_INDEX_RANGE: n_rows >= 2^36 or an extent beyond 2^62 bytes.  n_rows == 0 or
 * n_vec == 0 succeeds and launches nothing.  colind is trusted to lie in [0, n_cols). */
int tfem_csr_spmm(const int64_t *rowptr, const int32_t *colind, const void *vals, int real_bytes,
                  int64_t n_rows, int64_t n_cols, int n_vec, const void *x, void *y, void *stream);

/* A P1 DoF vector u (n_verts entries) on both sides of every interior edge: replaces the
 * tensor branch of Basis.interpolate(InteriorEdgesBasis, u) (reference basis.py:98-177;
 * SURVEY 8(f) f-2).  conn: (n_elems, 3) int32 cell vertices; edge_cells: (n_edges, 2) int64
 * = mesh["interior_edges", "cells"]; points: (n_edges, n_points, 2) = the edge basis's
 * integration points.  value: (n_edges, 2, n_points); grad: (n_edges, 2, 2) (constant along
 * the edge for P1).  All DEVICE pointers; ids are trusted (they come from the mesh topology). */
int tfem_edge_interpolate_p1(const void *coords, int real_bytes, const int32_t *conn,
                             const int64_t *edge_cells, const void *points, int64_t n_edges,
                             int n_points, const void *u, void *value, void *grad, void *stream);

/* Adjoint of tfem_edge_interpolate_p1 in u: grad_u (n_verts entries, overwritten) =
 * A^T g_value + B^T g_grad for value = A u, grad = B u; g_value (n_edges, 2, n_points) and
 * g_grad (n_edges, 2, 2) are the cotangents of the two outputs.  What autograd derives from the
 * reference's expressions (basis.py:150-158) when u carries history; floating-point atomics, the
 * summation order is not fixed. */
int tfem_edge_interpolate_p1_backward(const void *coords, int real_bytes, const int32_t *conn,
                                      const int64_t *edge_cells, const void *points, int64_t n_edges,
                                      int n_points, const void *g_value, const void *g_grad,
                                      void *grad_u, int64_t n_verts, void *stream);

/* The same adjoint WITHOUT atomics (fixed summation order, bitwise reproducible): one lane per
 * vertex walks the (edge, side) pairs around it.  inc_ptr (n_verts + 1) / inc_side: for every
 * vertex the entries 4 * (2 * edge + side) + local index of the vertex in that side's cell,
 * ascending (DEVICE int64 arrays, built once per edge table by the caller). */
int tfem_edge_interpolate_p1_backward_rows(const void *coords, int real_bytes, const int32_t *conn,
                                           const int64_t *edge_cells, const void *points,
                                           int64_t n_edges, int n_points, const void *g_value,
                                           const void *g_grad, const int64_t *inc_ptr,
                                           const int64_t *inc_side, void *grad_u, int64_t n_verts,
                                           void *stream);

/* FractureBasis.interpolate(InteriorEdgesFractureBasis, u) (fracture_basis.py:225-272): a P1
 * DoF vector on both sides of every interior edge of every fracture.  All DEVICE:
 *   coords2d (F, n_verts, 2), coords3d (F, n_verts, 3) = mesh["vertices", "coordinates_3d"],
 *   conn (F, n_cells, 3) int32 per-fracture vertex ids, edge_cells (F, n_edges, 2) int64 per-
 *   fracture cell ids, points (F, n_edges, n_points, 3) the edge basis's 3-D integration points,
 *   pinv (F, 2, 3) = mesh["inv_jacobian_fracture_map"], u (n_u).
 *   value (F, n_edges, 2, n_points), grad (F, n_edges, 2, 3).
 * u is indexed with the PER-FRACTURE vertex ids of the cells, exactly as the reference does
 * (fracture_basis.py:229-231) -- reproduced, not repaired. */
int tfem_edge_interpolate_p1_fracture(const void *coords2d, const void *coords3d, int real_bytes,
                                      const int32_t *conn, const int64_t *edge_cells, const void *points,
                                      const void *pinv, int64_t n_fractures, int64_t n_verts,
                                      int64_t n_cells, int64_t n_edges, int n_points, const void *u,
                                      int64_t n_u, void *value, void *grad, void *stream);

/* CSR -> dense (n_dofs, n_dofs) row-major, the layout integrate_bilinear_form
 * returns in the reference (abstract_basis.py:81).  dense is overwritten. */
int tfem_csr_to_dense(const int64_t *rowptr, const int32_t *colind, const void *vals,
                      int real_bytes, int64_t n_dofs, void *dense, void *stream);

/* ------------------------------------------------------------------------- *
 * Tile plan (HOST, once per mesh) + tile kernel (DEVICE): the P1 headline path.
 * The CSR rows (= vertices) are cut into spatially compact tiles along a Z-order
 * curve; a tile owns its rows, processes every element incident to them,
 * accumulates in LDS and writes each CSR value once (no global atomics, no
 * zero-fill).  Replaces, like tfem_tri_bilinear_csr, abstract_basis.py:74-93
 * fused with abstract_mesh.py:257-262 and basis.py:64-96; requires P1 with DoFs =
 * vertices (conn indexes coords) and rows of at most 16 entries.
 *   create : plan handle from connectivity, coordinates (for the curve) and the CSR
 *            pattern of tfem_csr_symbolic_*; capacities bound a tile's elements,
 *            local vertices, accumulator entries and owned rows.
 *   sizes  : fills layout[24]:
 *            [0] n_tiles [1] n_records [2] n_local_verts [3] n_owned_rows [4] n_runs
 *            [5] max elems/tile [6] max verts/tile [7] max owned/tile
 *            [8] max accumulator entries/tile [9] max row length [10] max runs/tile
 *            [11] n_run_starts (= n_runs + n_tiles)
 *            [12..18] byte offsets of desc, records, vert_gid, row_loff, run_delta,
 *            run_lstart, elem_id inside the packed plan; [19] bytes of the packed plan;
 *            [20] 32-bit words per element record: 3 (12-byte form) or 2 (8-byte form, used
 *            when no row has more than 8 entries); [21..23] reserved
 *   pack   : write the packed plan (layout[19] bytes, caller-owned HOST memory):
 *            desc int32 (12 per tile) | records (12-byte form: per vertex 16 * local id |
 *            4-bit column positions << 16; 8-byte form: three 10-bit local ids, nine 3-bit
 *            positions) | vert_gid int32 | row_loff uint16 |
 *            run_delta int32 | run_lstart uint16 | elem_id int32 (original element of every
 *            record).  An output run is a maximal group of owned rows that is contiguous in
 *            the CSR value array.  The caller copies the blob to the device once.
 * The handle is internal library memory and must be released with _destroy.
 * ------------------------------------------------------------------------- */
int tfem_tile_plan_create(const void *conn_host, int idx_bytes, int64_t n_elems,
                          int64_t n_verts, const double *coords_host,
                          const int64_t *rowptr_host, const int32_t *colind_host,
                          int elem_cap, int vert_cap, int acc_cap, int own_cap,
                          void **plan_out);
int tfem_tile_plan_sizes(const void *plan, int64_t layout[24]);
int tfem_tile_plan_pack(const void *plan, void *blob_host);
void tfem_tile_plan_destroy(void *plan);
/* Largest capacity the compiled kernel accepts: what = 0 elements, 1 local vertices,
 * 2 owned rows, 3 accumulator entries per tile. */
int tfem_tile_capacity(int what);
/* One launch over the tile plan (`plan_device` = DEVICE copy of the packed plan,
 * `plan_layout_host` = the HOST layout[24] of tfem_tile_plan_sizes):
 *   vals != NULL : CSR values of alpha * stiffness + beta * mass (every entry written
 *                  once; vals need not be initialised)        [abstract_basis.py:74-93]
 *   fq   != NULL : load vector fout[n_verts] = sum_e sum_q fq[e][q] phi_i(x_q) dx_q from
 *                  the user's source values fq (n_elems, Q) in ORIGINAL element order
 *                  (every entry written once)                 [abstract_basis.py:95-112]
 * Either or both.  The kernel addresses every array through range-checked buffer
 * resources (each array must stay below 4 GiB). */
int tfem_p1_assemble_tiles(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                           double alpha, double beta, const void *plan_device,
                           const int64_t *plan_layout_host, void *vals, int64_t nnz,
                           const void *fq, int64_t n_elems, void *fout, void *stream);

/* ------------------------------------------------------------------------- *
 * Ring plan (HOST, once per mesh) + ring kernel (DEVICE): P1 alpha * stiffness +
 * beta * mass in owner-computes ROW form.  Same operation as tfem_p1_assemble_tiles
 * with vals != NULL (abstract_basis.py:74-93 fused with abstract_mesh.py:257-262,
 * basis.py:64-96, element_tri.py:132-145), same requirements (P1, DoFs = vertices,
 * rows of at most 16 entries), no atomics at all: one lane owns one CSR row, walks
 * the fan of triangles around its vertex (neighbours listed in fan order as 10-bit
 * tile-local ids, the triangle of every slot flagged with its stored orientation)
 * and writes the row once.
 *   create : TFEM_ERR_UNSUPPORTED when the triangles around some vertex do not form
 *            one closed fan or open fans (an edge with three triangles, duplicated or
 *            degenerate elements): use the tile plan for such a mesh.
 *   sizes  : fills layout[32]: [0] n_tiles [1] n_rows [2] n_local_verts
 *            [3] max local verts/tile [4] max owned rows/tile [5] max row length
 *            [6] neighbour slots per row record (7 | 15) [7] dwords per row record (4 | 8)
 *            [8..11] byte offsets of desc, rows, rowstart, vert_gid in the packed plan
 *            [12] bytes of the packed plan [13] 1 when every wave's rows are consecutive
 *            vertices (tiles made of chunks of the numbering) [14] max halo vertices/tile
 *            [15] byte offset of row_ecodes, [16] of tile_elems in the packed plan [17] max
 *            elements per tile [18] 1 when every tile's elements fit the kernel's LDS stage
 *            (the fused load vector needs it) [19] entries of tile_elems [20] byte offset of
 *            tile_tverts (uint32 per tile element, in the order of the tile's ascending element
 *            list: the three tile-local vertex ids of the element in its own local order,
 *            10 bits each; desc[19] of a tile = its offset into this array), 0 when absent
 *            [21] entries of tile_tverts [22] byte offset and [23] number of the long rows (24-dword
 *            records of the vertices with 8 .. 15 neighbours in a plan with 4-dword records: their
 *            rows are written by a second launch; csrc/tfem_rings_host.cpp)
 *            [24] byte offset of chain_order (int32 per tile: the order in which the launches that
 *            evaluate a source program walk the tiles -- along the space-filling curve, the tiles
 *            owning flagged vertices first) [25] chain length L: a workgroup takes L consecutive
 *            positions of that order; inside such a block an element in the fans of two
 *            consecutive tiles is evaluated once, by the earlier one [26] byte offset of hand_in
 *            (uint16 per owned row, parallel to rowstart: the local id the row's vertex has in the
 *            PREVIOUS tile of its block, 0xFFFF: none -- the earlier tile sums the shares of all its
 *            local vertices, the row adds that sum to its own)
 *            [27] most elements a tile evaluates itself (desc[18] >> 8 of a tile = its count,
 *            tile_tverts holds exactly those; desc[18] & 0xFF = element-list mode)
 *   pack   : desc int32 (20 per tile: vert_off, n_vert, row_off, first row of wave 0..3 of
 *            the 256-lane workgroup (the first is 0), n_own, vertex id of the first row of
 *            wave 0..3, CSR offset of the first row of wave 0..3, offset into tile_elems,
 *            number of elements of the tile, 0, 0) | row records
 *            (bit layout: csrc/tfem_rings_host.cpp) | rowstart int32 (CSR offset of every
 *            owned row) | vert_gid int32 (owned rows first, ascending, then the halo)
 *   capacity: what = 0 owned rows per tile, 1 local vertices per tile
 * ------------------------------------------------------------------------- */
int tfem_ring_plan_create(const void *conn_host, int idx_bytes, int64_t n_elems,
                          int64_t n_verts, const double *coords_host,
                          const int64_t *rowptr_host, const int32_t *colind_host,
                          int own_cap, int vert_cap, void **plan_out);
int tfem_ring_plan_sizes(const void *plan, int64_t layout[32]);
int tfem_ring_plan_pack(const void *plan, void *blob_host);
void tfem_ring_plan_destroy(void *plan);
int tfem_ring_capacity(int what);
/* vals (nnz) = CSR values of alpha * stiffness + beta * mass; every entry of a row with
 * at least one element is written exactly once (vals need not be initialised).
 * fq != NULL: the same launch also writes the load vector fout[n_verts] = sum_e sum_q
 * fq[e][q] phi_i(x_q) dx_q from the user's source values fq (n_elems, Q) in ORIGINAL element
 * order (abstract_basis.py:95-112; every entry written once, 0 for a vertex without
 * elements).  vals == NULL with fq != NULL: the load vector alone. */
int tfem_p1_assemble_rings(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                           double alpha, double beta, const void *plan_device,
                           const int64_t *plan_layout_host, void *vals, int64_t nnz,
                           const void *fq, int64_t n_elems, void *fout, void *stream);
/* y[n_verts] = (alpha * stiffness + beta * mass) u over the same ring plan, without the CSR values
 * (abstract_basis.py:74-93 with basis.py:64-85: the operator the reference assembles, applied
 * instead of stored).  Every entry of y is written once (0 for a vertex without elements); u and y
 * (DEVICE, n_verts reals each, the plan's vertex numbering) must not overlap.  u == NULL: y =
 * diag(K).  Plans with long rows (layout[23] > 0) are served by a second launch for those rows. */
int tfem_p1_apply_rings(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                        double alpha, double beta, const void *plan_device,
                        const int64_t *plan_layout_host, const void *u, void *y, void *stream);
/* Y = (alpha * stiffness + beta * mass) U for n_vec vectors at once: U and Y (DEVICE, n_verts x n_vec
 * reals each, ROW-major: the n_vec values of a vertex are consecutive; the plan's vertex numbering)
 * must not overlap; every entry of Y is written once.  The rows of K are formed once per pass of up
 * to 8 columns (as many as the plan's tiles hold in 64 KB of LDS), a larger n_vec is served in
 * several passes over column ranges.  n_vec >= 1 of any size within the 32-bit extent (n_vec = 1
 * gives what tfem_p1_apply_rings gives); u == NULL is an error here (the diagonal has one column:
 * tfem_p1_apply_rings).  No allocation, no synchronisation. */
int tfem_p1_apply_rings_multi(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                              double alpha, double beta, const void *plan_device,
                              const int64_t *plan_layout_host, const void *u, void *y,
                              int64_t n_vec, void *stream);

/* ------------------------------------------------------------------------- *
 * Source programs: the coefficient f of the linear form f(x_q) * v
 * (abstract_basis.py:95-112 with the callers' closed vocabulary, SURVEY 8 a-7:
 * tests/test_assembly.py:75-84, examples/example_weak.py:59-61 ...) as a postfix
 * program over the coordinates (x, y) of an integration point, evaluated inside the
 * kernels at x_q = bar(q)^T X (basis.py:90-91).  The reference evaluates the user's
 * torch expressions on the cached (n_elems, Q, 1, 2) tensor and multiplies by v on
 * every call; here the Python tracer (pytorch_fem_solver_amd/basis/forms.py) records
 * those expressions once and the assembly launch re-evaluates them, so the 8 Q bytes
 * per element of pre-evaluated source values never exist in HBM.
 *   A stack machine of TFEM_SOURCE_STACK entries.  ops[i] with constant consts[i]:
 *   PUSH_X / PUSH_Y / PUSH_C   push c * x, c * y, or the constant c
 *   ADD SUB MUL DIV            pop hi, pop lo, push lo (op) hi;  SUB_R, DIV_R: hi (op) lo
 *   ADD_C MUL_C RSUB_C RDIV_C  top = top + c, top * c, c - top, c / top
 *   NEG ABS                    top = -top, |top|
 *   SIN COS EXP SQRT LOG TANH  top = c * fn(top)
 *   POW_I                      top = top^n, n = (int)c in 2..8, by multiplications
 *                              from the left (x*x, x*x*x as torch evaluates them)
 * A valid program never pops an empty stack, never exceeds the stack and leaves
 * exactly one entry: the value of f.
 * ------------------------------------------------------------------------- */
#define TFEM_SOURCE_MAX_OPS 32
#define TFEM_SOURCE_STACK 4
enum tfem_source_op {
  TFEM_SRC_END = 0,
  TFEM_SRC_PUSH_X = 1, TFEM_SRC_PUSH_Y = 2, TFEM_SRC_PUSH_C = 3,
  TFEM_SRC_ADD = 4, TFEM_SRC_SUB = 5, TFEM_SRC_SUB_R = 6, TFEM_SRC_MUL = 7,
  TFEM_SRC_DIV = 8, TFEM_SRC_DIV_R = 9,
  TFEM_SRC_ADD_C = 10, TFEM_SRC_MUL_C = 11, TFEM_SRC_RSUB_C = 12, TFEM_SRC_RDIV_C = 13,
  TFEM_SRC_NEG = 14, TFEM_SRC_ABS = 15, TFEM_SRC_POW_I = 16,
  TFEM_SRC_SIN = 17, TFEM_SRC_COS = 18, TFEM_SRC_EXP = 19, TFEM_SRC_SQRT = 20,
  TFEM_SRC_LOG = 21, TFEM_SRC_TANH = 22,
  TFEM_SRC_OP_COUNT = 23
};
typedef struct tfem_source_program {
  int32_t n_ops;
  int32_t reserved;
  uint8_t ops[TFEM_SOURCE_MAX_OPS];
  double consts[TFEM_SOURCE_MAX_OPS];
} tfem_source_program;

/* TFEM_OK when `program` (HOST) is a valid source program, TFEM_ERR_INVALID_ARGUMENT
 * (tfem_last_error says why) otherwise. */
int tfem_source_validate(const tfem_source_program *program);

/* fq (n_elems, Q) = f at the integration points of every element (DEVICE; conn (n_elems, 3)
 * vertex ids, `program` HOST): what the reference's callers compute with torch from
 * basis.integration_points before multiplying by v (tests/test_assembly.py:79-84).  Feeds the
 * entry points that take pre-evaluated source values (tfem_tri_load_vector,
 * tfem_p1_assemble_tiles, P2) when the ring kernel does not apply. */
int tfem_source_eval(const void *coords, int real_bytes, const void *conn, int idx_bytes,
                     int64_t n_elems, int64_t n_verts, int quad_order,
                     const tfem_source_program *program, void *fq, void *stream);

/* tfem_p1_assemble_rings with the source values computed in the launch: the load vector
 * fout[n_verts] = sum_e sum_q f(x_q) phi_i(x_q) dx_q of the program `source` (HOST), and, with
 * vals != NULL, the CSR values of alpha * stiffness + beta * mass in the same launch.  The
 * plan must carry the per-tile element vertex table (layout[20] != 0). */
int tfem_p1_assemble_rings_source(const void *coords, int real_bytes, int64_t n_verts,
                                  int quad_order, double alpha, double beta,
                                  const void *plan_device, const int64_t *plan_layout_host,
                                  void *vals, int64_t nnz, const tfem_source_program *source,
                                  int64_t n_elems, void *fout, void *stream);

/* The caller vouches for ONE coordinate array (DEVICE pointer `coords`, as it is passed to the
 * launches): every |x|, |y| in it is <= max_abs_coord (finite, >= 0).  Array and bound are kept in
 * plan_layout_host[29] and [31] (HOST, the 32 values of tfem_ring_plan_sizes; [29] = 0: no bound)
 * and travel with the layout to the launches.  An fp64 tfem_p1_assemble_rings_source / _range launch
 * that is given THAT array proves ONCE, on the host, that a SIN / COS applied to a coordinate push
 * stays on the fast path (tfem_source_trig_proof) and skips the range test of every value; a launch
 * with another coordinate array, without a bound, or where the proof fails tests every value as
 * before.  The integration points are convex combinations of the vertices, so the bound holds for
 * them.  A NULL array or a negative or non-finite max_abs_coord withdraws the bound.  The bound is
 * a statement about the array's CONTENTS: a caller that writes other coordinates into the same
 * array must withdraw or renew it.  (The bound is state of the layout and not an argument of a
 * launch so that the launches keep their entry points and signatures.) */
int tfem_ring_plan_vouch_coords(int64_t *plan_layout_host, const void *coords, double max_abs_coord);

/* ops_out[i] (HOST, TFEM_SOURCE_MAX_OPS entries, 0 behind the program) = the operation codes a
 * tfem_p1_assemble_rings_source / _range launch with these arguments hands to its kernel: the
 * program's own, with TFEM_SRC_OP_COUNT (sine) / TFEM_SRC_OP_COUNT + 1 (cosine) in place of the
 * SIN / COS whose range the launch has proven from the vouched bound.  For tests and tools: what a
 * launch decided is otherwise visible in its time only. */
int tfem_p1_rings_source_ops(const void *coords, int real_bytes, int quad_order,
                             const int64_t *plan_layout_host, const tfem_source_program *source,
                             uint8_t *ops_out);

/* What evaluates the program in a tfem_p1_assemble_rings_source / _range launch with these arguments
 * (those of tfem_p1_rings_source_ops): 0 the general interpreter (one element per pass), 1 the wide
 * interpreter (programs that hold at most two values, up to four points), 2 straight-line code for a
 * separable program -- after the proof exactly PUSH_a(c0) F(c1) PUSH_b(c2) G(c3) MUL with {a, b} =
 * {X, Y} and F, G proven SIN / COS, in an fp64 launch with the 4-point rule.  TFEM_RINGS_SEPARABLE=0 in
 * the environment keeps such a program on route 1.  The kernel receives the same operation codes on
 * routes 1 and 2 (tfem_p1_rings_source_ops).  A negative value is minus the status of a refused call. */
int tfem_p1_rings_source_route(const void *coords, int real_bytes, int quad_order,
                               const int64_t *plan_layout_host, const tfem_source_program *source);

/* The three constants an fp64 launch with the 4-point rule multiplies the source values with when it forms
 * an element's shares g_i = W0 f_0 + W1 (f_1 + f_2 + f_3) + W2 f_q(i) -> weights_out[0..2] (HOST); zeros
 * for float32 and the other rules.  On routes 0 and 1 they are the rule's own (c0 w_0 / 2, b w_1 / 2,
 * d w_1 / 2); on route 2 the kernel evaluates the two bare functions and the factors c1, c3 behind them
 * ride on the constants as k = c1 c3, whichever coordinate the program pushes first.  A program whose k is
 * not finite, or is subnormal while c1 and c3 are not, is not taken on route 2.  Returns the route
 * (tfem_p1_rings_source_route) or minus the status of a refused call.  For tests and tools. */
int tfem_p1_rings_source_weights(const void *coords, int real_bytes, int quad_order,
                                 const int64_t *plan_layout_host, const tfem_source_program *source,
                                 double *weights_out);

/* fast_out[i] (HOST, TFEM_SOURCE_MAX_OPS entries) = 1 where operation i of `program` is a SIN or
 * COS whose operand is the PUSH_X / PUSH_Y directly in front of it, with constant c, and
 *   |c| * max_abs_coord * (1 + 1e-9) < 1e9 / 2
 * (1e9: below it the fp64 kernels take their own sin / cos, above it the library's), 0 elsewhere.
 * Returns the number of such operations; 0 for an invalid program or a max_abs_coord that is
 * negative or not finite. */
int tfem_source_trig_proof(const tfem_source_program *program, double max_abs_coord,
                           uint8_t *fast_out);

/* Variable coefficients: the CSR values of
 *   alpha * int kappa(x, y) grad u . grad v + beta * int c(x, y) u v
 * over a ring plan, kappa and c source programs (HOST) evaluated at the integration points inside
 * the launch (replaces abstract_basis.py:74-93 applied to a caller's `kappa * (v_grad @ v_grad.mT)
 * + c * (v @ v.mT)`, whose (n_elems, Q, 3, 3) integrand the reference builds with torch).  A NULL
 * program leaves that term its constant coefficient 1; with BOTH NULL the call fails with
 * TFEM_ERR_INVALID_ARGUMENT (tfem_p1_assemble_rings is the entry point then).  Both programs are
 * validated as by tfem_source_validate before anything is launched.  vals (DEVICE): the nnz values
 * of the CSR pattern the plan was built from; every entry of a row with at least one element is
 * written exactly once.  The call takes no nnz and the plan's layout carries none: the value stores
 * are bounds-checked against rows * longest row (layout[1] * layout[5]) reals, an upper bound of
 * nnz, and that product times real_bytes must stay below 2^32 (TFEM_ERR_INDEX_RANGE otherwise,
 * somewhat earlier than tfem_p1_assemble_rings would refuse).  No allocation, no synchronisation.  Plans with long rows (layout[23] > 0)
 * are refused with TFEM_ERR_UNSUPPORTED.  K_ij and K_ji agree to rounding, not bit for bit: a row
 * visits the integration points of a triangle starting from its own vertex. */
int tfem_p1_rings_coef(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                       double alpha, double beta, const tfem_source_program *kappa,
                       const tfem_source_program *c, const void *plan_device,
                       const int64_t *plan_layout_host, void *vals, void *stream);
/* The same operator applied: y[n_verts] = K u without the CSR values (abstract_basis.py:74-93, applied
 * instead of stored); u == NULL: y = diag(K).  u and y as for tfem_p1_apply_rings. */
int tfem_p1_apply_rings_coef(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                             double alpha, double beta, const tfem_source_program *kappa,
                             const tfem_source_program *c, const void *plan_device,
                             const int64_t *plan_layout_host, const void *u, void *y, void *stream);
/* Y = K U of the same operator for n_vec vectors at once: U and Y (DEVICE, n_verts x n_vec reals each,
 * ROW-major as for tfem_p1_apply_rings_multi; the plan's vertex numbering) must not overlap; every
 * entry of Y is written once (0 for a vertex without elements).  The coefficient programs are
 * evaluated once per row and triangle for a pass of up to 8 columns (4 with 15-slot records), a
 * larger n_vec is served in several passes over column ranges; column j of Y is bit for bit what
 * tfem_p1_apply_rings_coef gives for column j of U.  n_vec >= 1 of any size within the 32-bit extent (n_vec = 1 IS
 * tfem_p1_apply_rings_coef); u == NULL is an error here (the diagonal has one column:
 * tfem_p1_apply_rings_coef).  Refused before anything is launched, Y untouched: both programs NULL
 * or an invalid one, overlapping U and Y (TFEM_ERR_INVALID_ARGUMENT), an extent n_verts * n_vec *
 * real_bytes >= 2^32 (TFEM_ERR_INDEX_RANGE), plans with long rows and unknown integration orders
 * (TFEM_ERR_UNSUPPORTED).  No allocation, no synchronisation. */
int tfem_p1_apply_rings_coef_multi(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                                   double alpha, double beta, const tfem_source_program *kappa,
                                   const tfem_source_program *c, const void *plan_device,
                                   const int64_t *plan_layout_host, const void *u, void *y,
                                   int64_t n_vec, void *stream);

/* Coefficient DATA: the CSR values of
 *   alpha * int kappa grad u . grad v + beta * int c u v
 * over a ring plan, kappa and c given as values at the integration points (replaces
 * abstract_basis.py:74-93 applied to a caller's `kq * (v_grad @ v_grad.mT) + cq * (v @ v.mT)` with
 * tensors kq, cq, whose (n_elems, Q, 3, 3) integrand the reference builds with torch).
 *   kappa / c: DEVICE, n_elems * kappa_nq (c_nq) reals, element-major in the element order of the
 *   connectivity the plan was built from, the q order of tfem_quadrature_rule; *_nq = Q (a value per
 *   integration point) or 1 (one value per element, read once per element and never expanded);
 *   NULL = the constant 1 (its *_nq is ignored); both NULL: TFEM_ERR_INVALID_ARGUMENT
 *   (tfem_p1_assemble_rings / tfem_p1_apply_rings are the entry points then).
 * One launch: per tile the values of the tile's elements (the plan's tile_elems, layout[16], as a
 * list or as runs) are read once, coalesced, and reduced to one number per element for the stiffness
 * term and six for the mass term, which the rows pick up from LDS through their slot codes
 * (row_ecodes, layout[15]) -- the lookup of the fused load vector; no atomics.  vals (DEVICE): the
 * values of the CSR pattern the plan was built from, bounds-checked against layout[1] * layout[5]
 * reals as for tfem_p1_rings_coef.  K_ij and K_ji agree to rounding, not bit for bit.
 * Refused before anything is launched, the outputs untouched: real_bytes not 4 or 8, a NULL layout,
 * negative sizes, *_nq neither 1 nor Q, both fields NULL, u overlapping y
 * (TFEM_ERR_INVALID_ARGUMENT); an extent of 2^32 bytes or more, n_elems * *_nq * real_bytes
 * included (TFEM_ERR_INDEX_RANGE); plans with long rows (layout[23] > 0), plans whose tiles do not
 * fit the element stage (layout[18] == 0), plans whose largest tile (layout[3] vertices, layout[17]
 * elements) needs more than 64 KB of LDS, unknown integration orders (TFEM_ERR_UNSUPPORTED).  Empty
 * plans succeed and launch nothing.  No allocation, no synchronisation. */
int tfem_p1_rings_field(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                        double alpha, double beta, const void *kappa, int kappa_nq, const void *c,
                        int c_nq, int64_t n_elems, const void *plan_device,
                        const int64_t *plan_layout_host, void *vals, void *stream);
/* The same operator applied: y[n_verts] = K u without the CSR values (abstract_basis.py:74-93, applied
 * instead of stored); u == NULL: y = diag(K).  u and y as for tfem_p1_apply_rings; they must not
 * overlap. */
int tfem_p1_apply_rings_field(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                              double alpha, double beta, const void *kappa, int kappa_nq,
                              const void *c, int c_nq, int64_t n_elems, const void *plan_device,
                              const int64_t *plan_layout_host, const void *u, void *y, void *stream);
/* Y = K U of the same operator for n_vec vectors at once: U and Y (DEVICE, n_verts x n_vec reals each,
 * ROW-major as for tfem_p1_apply_rings_multi; the plan's vertex numbering) must not overlap; every
 * entry of Y is written once (0 for a vertex without elements).  The values of a tile's elements are
 * read and reduced once for a pass of up to 8 columns (4 with 15-slot records; the widest width whose
 * LDS, ((2 + width) * lds_vert + (7 with a mass term, else 1) * lds_elem) * real_bytes, fits 64 KB),
 * a larger n_vec is served in several passes over column ranges; column j of Y is bit for bit what
 * tfem_p1_apply_rings_field gives for column j of U.  n_vec >= 1 of any size within the 32-bit extent
 * (n_vec = 1 IS tfem_p1_apply_rings_field); u == NULL is an error here (the diagonal has one column:
 * tfem_p1_apply_rings_field).  Refused before anything is launched, Y untouched, in this order:
 * real_bytes not 4 or 8, a NULL layout, negative sizes, n_vec < 1, u NULL, both fields NULL, *_nq
 * neither 1 nor Q (TFEM_ERR_INVALID_ARGUMENT); an extent n_verts * n_vec * real_bytes or n_elems *
 * *_nq * real_bytes >= 2^32 (TFEM_ERR_INDEX_RANGE); U and Y overlapping anywhere in the block
 * (TFEM_ERR_INVALID_ARGUMENT); plans with long rows, plans whose tiles do not fit the element stage
 * (layout[18] == 0, layout[17] > 768), plans whose largest tile needs more than 64 KB of LDS for two
 * columns -- the caller applies such a plan column by column --, unknown integration orders
 * (TFEM_ERR_UNSUPPORTED).  Empty plans succeed and launch nothing.  No allocation, no
 * synchronisation. */
int tfem_p1_apply_rings_field_multi(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                                    double alpha, double beta, const void *kappa, int kappa_nq,
                                    const void *c, int c_nq, int64_t n_elems, const void *plan_device,
                                    const int64_t *plan_layout_host, const void *u, void *y,
                                    int64_t n_vec, void *stream);
/* The derivative of sum_cols g^T K u with respect to the values (the backward of the apply launch in
 * kappa and c; abstract_basis.py:74-93 differentiated in the coefficient of the integrand), element
 * form, one lane per element:
 *   grad_kappa[e][q] = alpha * dx_q * sum_cols grad g_h . grad u_h
 *   grad_c[e][q]     = beta  * dx_q * sum_cols g_h(x_q) u_h(x_q),   dx_q = (w_q / 2) * det_e
 * with the reference's signed determinant (element_tri.py:139).  conn: (n_elems, 3) int32 vertex ids
 * (DEVICE) in the numbering of coords, g and u; g, u: n_verts x n_vec reals, ROW-major as for
 * tfem_p1_apply_rings_multi (n_vec >= 1).  grad_kappa / grad_c: (n_elems, Q) reals, either may be
 * NULL (both: nothing is launched); every entry is written once, no atomics.  Data with one value
 * per element takes the sum of its row. */
int tfem_p1_field_adjoint(const void *coords, int real_bytes, const void *conn, int64_t n_elems,
                          int64_t n_verts, int quad_order, double alpha, double beta, const void *g,
                          const void *u, int64_t n_vec, void *grad_kappa, void *grad_c, void *stream);

/* Multi-GPU: the rows shared with other ranks first.  create_priority = create with
 * vertex_priority_host (n_verts bytes, non-zero = flagged; NULL = none): the tiles that own a flagged
 * vertex come first in the plan's tile list (*n_priority_tiles of them), the order inside both groups
 * unchanged.  _range = tfem_p1_assemble_rings / _source (fq or source or neither) over the tiles
 * [tile_first, tile_first + tile_count) only (tile_count < 0: to the end): the launch over the
 * priority tiles completes every shared row, so their exchange can run beside the launch over the
 * remaining tiles.  (In a plan with long rows those are written with the range that ends the list.) */
int tfem_ring_plan_create_priority(const void *conn_host, int idx_bytes, int64_t n_elems, int64_t n_verts,
                                   const double *coords_host, const int64_t *rowptr_host,
                                   const int32_t *colind_host, int own_cap, int vert_cap,
                                   const uint8_t *vertex_priority_host, void **plan_out,
                                   int64_t *n_priority_tiles);
/* The same plan from a CSR pattern handle (tfem_csr_pattern_create of the P1 connectivity, still
 * alive, with the colind tfem_csr_pattern_export wrote): reuses the handle's connectivity, row
 * pointers and vertex -> elements incidence instead of building the incidence again (the lists of
 * the handle are sorted in place).  Same plan bytes as tfem_ring_plan_create_priority. */
int tfem_ring_plan_create_from_pattern(void *pattern, const double *coords_host, const int32_t *colind_host,
                                       int own_cap, int vert_cap, const uint8_t *vertex_priority_host,
                                       void **plan_out, int64_t *n_priority_tiles);
int tfem_p1_assemble_rings_range(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                                 double alpha, double beta, const void *plan_device,
                                 const int64_t *plan_layout_host, void *vals, int64_t nnz, const void *fq,
                                 const tfem_source_program *source, int64_t n_elems, void *fout,
                                 int64_t tile_first, int64_t tile_count, void *stream);


/* ------------------------------------------------------------------------- *
 * The VPINN residual linear form, fused (DEVICE; P1 on one 2-D mesh):
 *   r_i = sum_T sum_q dx_q ( f(x_q) v_i(q) + flux_sign * grad v_i . g_q )
 * = integrate_linear_form of `rhs(x, y) * v - v_grad @ gradient(points).mT`
 * (examples/example_weak.py:64-75 with abstract_basis.py:95-112; flux_sign = -1 there).
 *   fq (n_elems, Q) source values, or `source` (HOST) a source program, or neither
 *   flux (n_elems, Q, 2) = g at the integration points, or NULL
 *   out_local (3, n_elems): the element vectors entry-major (out[i * n_elems + e]); the global
 *   vector follows from tfem_csr_gather with the gather map of the connectivity, as for
 *   tfem_tri_load_vector in LOCAL-VECTOR mode (no atomics, the reference's accumulation order).
 * backward: the adjoint, for the training step that differentiates through the form
 * (example_weak.py:132-152): from the cotangent of r (n_verts entries)
 *   grad_flux[e][q][k] = flux_sign * dx_q * sum_i cot[conn[e][i]] * (grad v_i)_k
 *   grad_fq[e][q]      = dx_q * sum_i cot[conn[e][i]] * v_i(q)
 * either may be NULL; every entry is written once, no atomics.
 * ------------------------------------------------------------------------- */
int tfem_p1_residual_local(const void *coords, int real_bytes, const void *conn, int idx_bytes,
                           int64_t n_elems, int64_t n_verts, int quad_order, const void *fq,
                           const tfem_source_program *source, const void *flux, double flux_sign,
                           void *out_local, void *stream);
int tfem_p1_residual_backward(const void *coords, int real_bytes, const void *conn, int idx_bytes,
                              int64_t n_elems, int64_t n_verts, int quad_order, const void *cotangent,
                              double flux_sign, void *grad_fq, void *grad_flux, void *stream);

/* ------------------------------------------------------------------------- *
 * P2 row plan (HOST, once per mesh) + P2 row kernels (DEVICE): alpha * stiffness +
 * beta * mass for the quadratic element in owner-computes ROW form (one lane per CSR
 * row of a vertex DoF or of an edge DoF, no atomics).  Same operation as
 * tfem_tri_bilinear_csr with poly_order = 2 (abstract_basis.py:74-93, element_tri.py:43-70);
 * requires DoFs numbered "vertices, then edges" with the local edge order (v0,v1), (v1,v2),
 * (v2,v0) (conn_dof (n_elems, 6), vertex DoF id = vertex id), at most 15 neighbours per
 * vertex and a numbering with locality; otherwise create returns TFEM_ERR_UNSUPPORTED and
 * the caller uses the local-block + gather path.  Vertex rows with 8 .. 15 neighbours (every
 * Delaunay mesh has them) are written by a third launch, one lane per such row.
 *   sizes : layout[24]: [0] vertex-row tiles [1] edge-row tiles [2] n_verts [3] n_edges
 *           [4] max local vertices of a vertex tile [5] of an edge tile [6] max halo of a
 *           vertex tile [7],[8] local vertices listed for vertex / edge tiles
 *           [10..15] byte offsets of desc, rows, vert_gid of the vertex tiles and of the edge
 *           tiles in the packed plan [16] bytes of the packed plan [17] byte offset and [18] number
 *           of the long vertex rows (32-dword records) [19..21] element codes of the load-vector
 *           launch (tfem_p2_load_rows)
 *   pack  : record and descriptor layout: csrc/tfem_p2rows_host.cpp
 * ------------------------------------------------------------------------- */
int tfem_p2_plan_create(const int32_t *conn_dof_host, int64_t n_elems, int64_t n_verts,
                        int64_t n_dofs, const double *coords_host, const int64_t *rowptr_host,
                        const int32_t *colind_host, void **plan_out);
int tfem_p2_plan_sizes(const void *plan, int64_t layout[24]);
int tfem_p2_plan_pack(const void *plan, void *blob_host);
void tfem_p2_plan_destroy(void *plan);
/* vals (nnz): every entry written exactly once (launches: vertex rows, long vertex rows if
 * any, edge rows). */
int tfem_p2_assemble_rows(const void *coords, int real_bytes, int quad_order, double alpha,
                          double beta, const void *plan_device, const int64_t *plan_layout_host,
                          void *vals, int64_t nnz, void *stream);
/* The P2 load vector in ROW form over the same plan (replaces integrate_linear_form of f v for
 * ElementTri(2, .): abstract_basis.py:95-112, element_tri.py:43-70, dx of basis.py:93-96):
 *   out[r] = sum over the triangles T of DoF r of det_T * sum_q fq[T][q] phi_loc(q) w_q / 2
 * fq (n_elems, Q) source values at the integration points of the elements in their stored frame,
 * out (n_dofs) written exactly once per DoF (launches: vertex rows, long vertex rows if any, edge
 * rows); no atomics, no element vectors.  The plan's layout[19], [20], [21]: byte offsets of the
 * element codes (element * 4 + local index of the DoF among the three of its kind) of the vertex
 * rows (8 dwords per row), the edge rows (2 dwords) and the long rows (16 dwords). */
int tfem_p2_load_rows(const void *coords, int real_bytes, int quad_order, const void *plan_device,
                      const int64_t *plan_layout_host, const void *fq, int64_t n_elems, void *out,
                      int64_t n_dofs, void *stream);
/* y[n_dofs] = (alpha * stiffness + beta * mass) u for ElementTri(2, .) over the same plan, without
 * the CSR values (abstract_basis.py:74-93 with element_tri.py:43-70: the operator the reference
 * assembles, applied instead of stored).  The rows are formed as tfem_p2_assemble_rows forms them;
 * every entry is multiplied by u of its column and the row's sum is written: one number per DoF,
 * every entry of y written once (0 for a vertex without elements).  The plan's records hold CSR
 * positions, so the launch reads colind (nnz int32, the pattern the plan was created from) for the
 * columns; the row starts come from the plan's descriptors and records, rowptr is not an argument.
 * u and y (n_dofs reals each, the plan's DoF numbering) must not overlap.  u == NULL: y = diag(K)
 * (colind is not read then, but is still required).  All pointers DEVICE except plan_layout_host.
 * Launches: vertex rows, long vertex rows if any, edge rows.  No allocation, no synchronisation.
 * TFEM_ERR_INVALID_ARGUMENT: real_bytes not 4 or 8, NULL plan_layout_host, negative sizes, n_dofs
 * != layout[2] + layout[3], u overlapping y, a NULL array or capacities beyond the kernels' on a
 * non-empty plan; TFEM_ERR_INDEX_RANGE: an array of 4 GiB or more; TFEM_ERR_UNSUPPORTED: an unknown
 * quadrature order.  Nothing is launched after a refusal. */
int tfem_p2_apply_rows(const void *coords, int real_bytes, int quad_order, double alpha, double beta,
                       const void *plan_device, const int64_t *plan_layout_host,
                       const int32_t *colind, int64_t nnz, const void *u, void *y, int64_t n_dofs,
                       void *stream);
/* Y = (alpha * stiffness + beta * mass) U of the same operator for n_vec vectors at once: U and Y
 * (DEVICE, n_dofs x n_vec reals each, ROW-major: the n_vec values of a DoF are consecutive, the
 * layout of tfem_p1_apply_rings_multi; the plan's DoF numbering) must not overlap; every entry of Y
 * is written once.  The records, colind, the coordinates and the entries of a row are read and
 * formed once per pass of up to 4 columns, a larger n_vec is served in several passes over column
 * ranges; the long vertex rows take every column in one launch.  real_bytes 4: one launch per kind
 * of row reads them once and forms the row once per column (what the bits below need in fp32).
 * Column c of Y has the bits that tfem_p2_apply_rows gives for column c.  n_vec >= 1 (n_vec = 1 IS the tfem_p2_apply_rows launch);
 * u == NULL on a non-empty plan is an error here (the diagonal has one column: tfem_p2_apply_rows).
 * Everything tfem_p2_apply_rows refuses is refused in the same way; in addition n_vec < 1 and U
 * overlapping Y anywhere in n_dofs * n_vec * real_bytes give TFEM_ERR_INVALID_ARGUMENT, and that
 * extent reaching 0xFFFFFF00 bytes gives TFEM_ERR_INDEX_RANGE.  Nothing is launched and Y is not
 * touched after a refusal; an empty plan launches nothing.  No allocation, no synchronisation. */
int tfem_p2_apply_rows_multi(const void *coords, int real_bytes, int quad_order, double alpha,
                             double beta, const void *plan_device, const int64_t *plan_layout_host,
                             const int32_t *colind, int64_t nnz, const void *u, void *y,
                             int64_t n_dofs, int64_t n_vec, void *stream);

/* ------------------------------------------------------------------------- *
 * The vector part of the Jacobi-preconditioned CG loop around any of the applies above (the loop
 * that stands where the reference's dense reduce + torch.linalg.solve stops being possible,
 * abstract_basis.py:114-117,177-195): per iteration
 *   AP = K P (an apply), tfem_cg_dot, tfem_cg_update, tfem_cg_direction
 * with alpha, beta and every dot product kept on the device.  All vectors DEVICE, n x n_vec reals
 * of real_bytes 4 or 8, ROW-major (the n_vec values of a DoF consecutive: the layout of
 * tfem_p1_apply_rings_multi); n_vec = 1 is the single-vector loop.  Arrays aligned to 16 bytes with
 * n_vec in {1, 2, 4, 8} are moved 16 bytes at a time, everything else by passes over 8 columns.
 *   inv_diag (n reals): mask / diag(K).  It doubles as the mask: inv_diag[i] == 0 marks a HELD DoF
 *            (outside `free`).  A held row is never written by update / direction and takes no part
 *            in any sum (it is skipped, not multiplied by 0: its Ap may be anything, NaN included).
 *   active   (n_vec int32): 0 freezes a column -- alpha = beta = 0 and nothing of it is written.
 *   ws       the caller's workspace of tfem_cg_workspace_bytes(n, n_vec) bytes, need not be
 *            initialised: 5 buffers of G x n_vec doubles [workgroup][column], G = bytes / (40 n_vec)
 *            a function of n alone: p.Ap | r.z parity 0 | r.r parity 0 | r.z parity 1 | r.r parity 1.
 *            Every launch writes one partial sum per workgroup and column (double, also for float
 *            vectors); a later launch sums the G partials of a column itself, every workgroup in the
 *            same order -- no atomics, the same bits in every run.  sum over axis 0 of the r.r buffer
 *            of parity step & 1 is |r|^2 per column after tfem_cg_update(step).
 *   step     iteration number >= 0; its parity picks the buffers: update(step) reads r.z of parity
 *            (step - 1) & 1 and writes parity step & 1, direction(step) reads both.
 * start:     p = inv_diag * r (0 on held rows); partials of r.(inv_diag * r) and r.r into parity 1,
 *            the one step 0 reads as "previous".
 * dot:       partials of sum p * ap per column over the rows that are not held.
 * update:    alpha_j = active[j] ? r.z_j / p.Ap_j : 0; x += alpha p, r -= alpha ap on the rows that
 *            are not held; partials of r.(inv_diag * r) and r.r (all columns) into parity step & 1.
 * direction: beta_j = r.z_j(step) / r.z_j(step - 1); p = inv_diag * r + beta p for active columns
 *            on the rows that are not held.
 * One launch each; no allocation, no synchronisation.  TFEM_ERR_INVALID_ARGUMENT: real_bytes not 4
 * or 8, a negative size or step, a NULL array with n > 0 and n_vec > 0; TFEM_ERR_INDEX_RANGE: a
 * vector of 4 GiB or more (rows and entries are counted in 32 bits).  Nothing is launched after a
 * refusal; n == 0 or n_vec == 0 succeeds and launches nothing.
 * tfem_cg_workspace_bytes (HOST): > 0 for n >= 0, n_vec >= 1; -1 for a negative argument or for
 * vectors the launches refuse (so the size always fits the int it is returned in).
 * tfem_cg_constant (HOST): what = 0 lanes per workgroup, 1 the cap of G, 2 columns per pass.
 * ------------------------------------------------------------------------- */
int tfem_cg_workspace_bytes(int64_t n, int64_t n_vec);
int tfem_cg_constant(int what);
int tfem_cg_start(const void *r, const void *inv_diag, void *p, int real_bytes, int64_t n,
                  int64_t n_vec, void *ws, void *stream);
int tfem_cg_dot(const void *p, const void *ap, const void *inv_diag, int real_bytes, int64_t n,
                int64_t n_vec, void *ws, void *stream);
int tfem_cg_update(void *x, void *r, const void *p, const void *ap, const void *inv_diag,
                   const int32_t *active, int real_bytes, int64_t n, int64_t n_vec, int64_t step,
                   void *ws, void *stream);
int tfem_cg_direction(void *p, const void *r, const void *inv_diag, const int32_t *active,
                      int real_bytes, int64_t n, int64_t n_vec, int64_t step, const void *ws,
                      void *stream);

/* ------------------------------------------------------------------------- *
 * The same loop around a preconditioner that hands z = M^-1 r over as a VECTOR (the V-cycle of the
 * multigrid hierarchies): per iteration
 *   AP = K P (an apply), tfem_cg_dot, tfem_pcg_update, [the preconditioner: r -> z], tfem_pcg_rz,
 *   tfem_pcg_direction
 * Vectors, widths, `active`, `step` and the workspace are those of tfem_cg_* above (the workspace
 * of tfem_cg_workspace_bytes with the same five buffers), and so are the reductions: per-workgroup
 * partial sums, finished by every workgroup of a later launch in one fixed order.
 *   mask (n reals) stands where inv_diag stands above: mask[i] == 0 marks a HELD DoF, any other
 *        value a free one (no mask: a vector of ones).  A held row is never written by update /
 *        direction and takes no part in any sum (it is skipped, not multiplied by 0: its ap and z
 *        may be anything, NaN included).  tfem_cg_dot takes the mask as its inv_diag.
 * start:     p = z on the rows that are not held, 0 on the held ones; partials of r.z into parity 1,
 *            the one step 0 reads as "previous".
 * update:    alpha_j = active[j] ? r.z_j(parity (step - 1) & 1) / p.Ap_j : 0; x += alpha p,
 *            r -= alpha ap on the rows that are not held of the active columns; partials of r.r
 *            (every column, the frozen ones included) into parity step & 1.  Writes no r.z.
 * rz:        partials of r.z over the rows that are not held into parity step & 1.
 * direction: beta_j = r.z_j(step & 1) / r.z_j((step - 1) & 1); p = z + beta p on the rows that are
 *            not held of the active columns; nothing of a frozen column is written.
 * One launch each; no allocation, no synchronisation.  The refusals are those of tfem_cg_*:
 * TFEM_ERR_INVALID_ARGUMENT for real_bytes not 4 or 8, a negative size or step, a NULL array with
 * n > 0 and n_vec > 0; TFEM_ERR_INDEX_RANGE for a vector of 4 GiB or more.  Nothing is launched
 * after a refusal; n == 0 or n_vec == 0 succeeds and launches nothing.
 * ------------------------------------------------------------------------- */
int tfem_pcg_start(const void *r, const void *z, const void *mask, void *p, int real_bytes,
                   int64_t n, int64_t n_vec, void *ws, void *stream);
int tfem_pcg_update(void *x, void *r, const void *p, const void *ap, const void *mask,
                    const int32_t *active, int real_bytes, int64_t n, int64_t n_vec, int64_t step,
                    void *ws, void *stream);
int tfem_pcg_rz(const void *r, const void *z, const void *mask, int real_bytes, int64_t n,
                int64_t n_vec, int64_t step, void *ws, void *stream);
int tfem_pcg_direction(void *p, const void *z, const void *mask, const int32_t *active,
                       int real_bytes, int64_t n, int64_t n_vec, int64_t step, const void *ws,
                       void *stream);

/* ------------------------------------------------------------------------- *
 * The vector part of a geometric multigrid V-cycle on nested P1 spaces (a mesh and its red
 * refinement; the reference has no multigrid, this stands where its dense solve stops being
 * possible, abstract_basis.py:114-117,177-195).  All arrays DEVICE; vectors of reals of real_bytes
 * 4 or 8.  Masks are arrays of reals holding 0 or 1, NULL = all ones.  One launch each, no
 * allocation, no synchronisation, no atomics: two calls on the same data give the same bits.
 * smooth:   first != 0: x = w * b (a sweep from the zero guess; ax is not read and may be NULL);
 *           first == 0: x = x + w * (b - ax), ax = K x from an apply.  w = omega * mask / diag(K),
 *           prepared by the caller.  n entries each.
 * restrict_residual: r_c[v] = mask_c[v] * 0.5 * sum_j mask_f[i_j] * (b_f[i_j] - ax_f[i_j]) over
 *           i_j = idx[ptr[v]] .. idx[ptr[v + 1] - 1], the transposed parent table of the
 *           refinement: ptr (n_c + 1 int32), idx (2 n_f int32) lists for coarse vertex v the fine
 *           vertices that name v as a parent, ascending, a vertex kept from the coarse mesh TWICE
 *           (so every weight of P^T is 0.5).  Eight lanes per row: lane s sums entries s, s + 8, ...
 *           in order, then the partial sums are added pairwise at distances 4, 2, 1.
 * prolong_add: x_f[i] = x_f[i] + mask_f[i] * 0.5 * (e_c[parents[2 i]] + e_c[parents[2 i + 1]]),
 *           parents (n_f x 2 int32) coarse vertex ids.
 * A product and a sum are rounded separately (no fma).  idx, parents and what they index are read
 * through bounds-checked buffer accesses: an index outside its array reads 0.
 * TFEM_ERR_INVALID_ARGUMENT: real_bytes not 4 or 8, a negative size, a NULL array that would be
 * read or written, the output overlapping an input; TFEM_ERR_INDEX_RANGE: an array of 4 GiB or
 * more.  Nothing is launched after a refusal; n == 0 (smooth), n_c == 0 (restrict), n_f == 0
 * (prolong) succeed and launch nothing.
 * ------------------------------------------------------------------------- */
int tfem_mg_smooth(void *x, const void *b, const void *ax, const void *w, int real_bytes, int64_t n,
                   int first, void *stream);
int tfem_mg_restrict_residual(const int32_t *ptr, const int32_t *idx, const void *mask_c,
                              const void *mask_f, const void *b_f, const void *ax_f, void *r_c,
                              int real_bytes, int64_t n_c, int64_t n_f, void *stream);
int tfem_mg_prolong_add(const int32_t *parents, const void *mask_f, const void *e_c, void *x_f,
                        int real_bytes, int64_t n_f, int64_t n_c, void *stream);

/* The same three on a block of n_vec >= 1 vectors (csrc/tfem_mg.hip).  x, b, ax, b_f, ax_f,
 * r_c, e_c, x_f are n x n_vec reals, ROW-major: the n_vec values of a DoF are consecutive (the
 * layout of tfem_p1_apply_rings_multi, tfem_csr_spmm and tfem_cg_*); w, the masks, ptr, idx and
 * parents keep one entry per DoF.  One launch for any n_vec; n_vec == 1 IS the single launch above.
 * smooth:   x[i][c] = w[i] * b[i][c], or x[i][c] = x[i][c] + w[i] * (b[i][c] - ax[i][c]); 16 bytes
 *           per lane when x, b and ax are aligned to 16 bytes, whatever n_vec (w is read per value).
 * restrict_residual: r_c[v][c] = mask_c[v] * 0.5 * sum_j mask_f[i_j] * (b_f[i_j][c] - ax_f[i_j][c]):
 *           the eight lanes per row and the order of the single launch for every column; idx and
 *           mask_f are read once per entry, one accumulator per column, at most 8 columns per pass.
 * prolong_add: x_f[i][c] = x_f[i][c] + mask_f[i] * 0.5 * (e_c[a][c] + e_c[b][c]), (a, b) =
 *           parents[i] read once per fine DoF.
 * With n_vec 2, 4 or 8 and the blocks aligned to min(16, n_vec * real_bytes) bytes the rows move
 * in accesses of that width, otherwise value by value.  Column c of every result is bit for bit
 * what the single launch gives for the contiguous copy of column c; no fma, no atomics, two calls
 * give the same bits.  An index of idx or parents outside its array reads 0 and touches nothing.
 * Refusals as above, with the extents of the blocks n * n_vec * real_bytes (4 GiB or more:
 * TFEM_ERR_INDEX_RANGE; the output overlapping an input anywhere in that extent:
 * TFEM_ERR_INVALID_ARGUMENT), and n_vec < 1: TFEM_ERR_INVALID_ARGUMENT.  A size of 0 (n, n_c for
 * restrict, n_f for prolong) succeeds and launches nothing. */
int tfem_mg_smooth_multi(void *x, const void *b, const void *ax, const void *w, int real_bytes,
                         int64_t n, int64_t n_vec, int first, void *stream);
int tfem_mg_restrict_residual_multi(const int32_t *ptr, const int32_t *idx, const void *mask_c,
                                    const void *mask_f, const void *b_f, const void *ax_f, void *r_c,
                                    int real_bytes, int64_t n_c, int64_t n_f, int64_t n_vec,
                                    void *stream);
int tfem_mg_prolong_add_multi(const int32_t *parents, const void *mask_f, const void *e_c, void *x_f,
                              int real_bytes, int64_t n_f, int64_t n_c, int64_t n_vec, void *stream);

/* The transfers between the P2 space and the P1 space of ONE mesh (csrc/tfem_mg.hip): the step
 * from a P2 level down to the P1 hierarchy above.  The P2 level has n_f = n_v + n_e DoFs, vertices
 * first, then edges; edge DoF n_v + j has the endpoints edge_vertices[2 j], edge_vertices[2 j + 1]
 * (n_e x 2 int32, vertex ids in either order).  P is the identity on the vertex rows and 0.5 / 0.5
 * on an edge row.  Vectors, masks (NULL = all ones), real_bytes and stream as above; one launch
 * each, no allocation, no synchronisation, no atomics, no fma: two calls give the same bits.
 * restrict_residual: with d(j) = mask_f[j] * (b_f[j] - ax_f[j]),
 *           r_c[v] = mask_c[v] * (d(v) + 0.5 * sum_{p in [ptr[v], ptr[v + 1])} d(idx[p])).
 *           ptr (n_v + 1 int32), idx (2 n_e int32): row v lists the edge DoF ids (n_v already added)
 *           of the edges at vertex v, ascending; a vertex without edges has an empty row.  Eight
 *           lanes per row: lane s sums entries s, s + 8, ... in order, the partial sums are added
 *           pairwise at distances 4, 2, 1, then d(v) is added to 0.5 x the sum.
 * prolong_add: x_f[i] = x_f[i] + mask_f[i] * e_c[i] for i < n_v,
 *           x_f[i] = x_f[i] + mask_f[i] * (0.5 * (e_c[a] + e_c[b])), (a, b) = edge_vertices[i - n_v],
 *           for n_v <= i < n_f.  One lane per fine DoF.
 * idx, edge_vertices and what they index are read through bounds-checked buffer accesses: an entry
 * of idx >= n_f or an endpoint >= n_v counts as 0 and touches nothing.
 * TFEM_ERR_INVALID_ARGUMENT: real_bytes not 4 or 8, a negative size, n_f < n_v, a NULL array that
 * would be read or written, the output overlapping an input; TFEM_ERR_INDEX_RANGE: an array of
 * 4 GiB or more.  Nothing is launched after a refusal; n_v == 0 succeeds and launches nothing. */
int tfem_mg_p2_restrict_residual(const int32_t *ptr, const int32_t *idx, const void *mask_c,
                                 const void *mask_f, const void *b_f, const void *ax_f, void *r_c,
                                 int real_bytes, int64_t n_v, int64_t n_f, void *stream);
int tfem_mg_p2_prolong_add(const int32_t *edge_vertices, const void *mask_f, const void *e_c, void *x_f,
                           int real_bytes, int64_t n_v, int64_t n_f, void *stream);

/* The same two on a block of n_vec >= 1 vectors (csrc/tfem_mg.hip).  b_f, ax_f, r_c, e_c,
 * x_f are n x n_vec reals, ROW-major (the layout of tfem_mg_*_multi and tfem_p2_apply_rows_multi);
 * the masks, ptr, idx and edge_vertices keep one entry per DoF.  One launch for any n_vec;
 * n_vec == 1 IS the single launch above.
 * restrict_residual: r_c[v][c] = mask_c[v] * (d(v)[c] + 0.5 * sum_p d(idx[p])[c]) with
 *           d(j)[c] = mask_f[j] * (b_f[j][c] - ax_f[j][c]): the eight lanes per row and the order of
 *           the single launch for every column; idx and mask_f are read once per entry, one
 *           accumulator per column, at most 8 columns per pass.
 * prolong_add: x_f[i][c] = x_f[i][c] + mask_f[i] * e_c[i][c] for i < n_v,
 *           x_f[i][c] = x_f[i][c] + mask_f[i] * (0.5 * (e_c[a][c] + e_c[b][c])) for n_v <= i < n_f;
 *           one lane per fine DoF, which reads its endpoints and mask_f once.
 * With n_vec 2, 4 or 8 and the blocks aligned to min(16, n_vec * real_bytes) bytes the rows move
 * in accesses of that width, otherwise value by value.  Column c of every result is bit for bit
 * what the single launch gives for the contiguous copy of column c; no fma, no atomics, two calls
 * give the same bits.  An entry of idx >= n_f or an endpoint >= n_v counts as 0 and touches nothing.
 * Refusals as above, with the extents of the blocks n * n_vec * real_bytes (4 GiB or more:
 * TFEM_ERR_INDEX_RANGE; the output overlapping an input anywhere in that extent:
 * TFEM_ERR_INVALID_ARGUMENT), and n_vec < 1: TFEM_ERR_INVALID_ARGUMENT.  n_v == 0 succeeds and
 * launches nothing. */
int tfem_mg_p2_restrict_residual_multi(const int32_t *ptr, const int32_t *idx, const void *mask_c,
                                       const void *mask_f, const void *b_f, const void *ax_f, void *r_c,
                                       int real_bytes, int64_t n_v, int64_t n_f, int64_t n_vec,
                                       void *stream);
int tfem_mg_p2_prolong_add_multi(const int32_t *edge_vertices, const void *mask_f, const void *e_c,
                                 void *x_f, int real_bytes, int64_t n_v, int64_t n_f, int64_t n_vec,
                                 void *stream);

/* ------------------------------------------------------------------------- *
 * Interface exchange of the multi-GPU sharding (DEVICE; the path shards by element
 * range, DoFs on an inter-rank interface are summed with one all-reduce of a packed
 * buffer: SURVEY 8(e); the reference is single-process).  pack: buf (nbuf) is zeroed,
 * then buf[k_pos[i]] = vals[k_idx[i]] (i < nk) and buf[f_pos[i]] = f[f_idx[i]] (i < nf);
 * unpack: the reverse copies.  vals / f may be NULL (that part is skipped); index arrays
 * are int64 device arrays.  One kernel launch each.
 * ------------------------------------------------------------------------- */
int tfem_interface_pack(const void *vals, const void *f, int real_bytes, const int64_t *k_idx,
                        const int64_t *k_pos, int64_t nk, const int64_t *f_idx, const int64_t *f_pos,
                        int64_t nf, void *buf, int64_t nbuf, void *stream);
int tfem_interface_unpack(void *vals, void *f, int real_bytes, const int64_t *k_idx,
                          const int64_t *k_pos, int64_t nk, const int64_t *f_idx,
                          const int64_t *f_pos, int64_t nf, const void *buf, void *stream);
/* pack in ONE launch, for the repeated step of a sharded run (the exchange chain -- zero, pack,
 * all-reduce, unpack, each behind the other -- is what bounds such a step at 1e6 elements per rank):
 * src (nbuf, int64 device array): >= 0 an entry of vals, <= -2 entry -src - 2 of f, -1 a position
 * other ranks own (written as zero).  buf[p] for every p < nbuf. */
int tfem_interface_pack_dense(const void *vals, const void *f, int real_bytes, const int64_t *src,
                              int64_t nbuf, void *buf, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TFEM_ASSEMBLY_H */
