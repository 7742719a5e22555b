// The transfers between the P2 space and the P1 space of ONE mesh (p-coarsening; multigrid.py,
// P2Multigrid): the step that puts a P2 level on top of the P1 hierarchy of tfem_mg.hip.
//
//   restrict : r_c = m_c P^T (m_f (b_f - ax_f))    the residual and P^T in ONE pass: the fine
//              residual is never stored
//   prolong  : x_f += m_f P e_c
//
// The P2 level has n_f = n_v + n_e DoFs, "vertices, then edges"; edge DoF n_v + j has the endpoints
// edge_vertices[j].  P1 is a subspace of P2 on the same mesh: P is the identity on the vertex rows
// and 0.5 / 0.5 on an edge row, so neither P nor P^T stores a value.  P^T is the identity plus the
// table (ptr, idx): row v lists the edge DoF ids (in the level's numbering, n_v already added) of
// the edges at vertex v, in ascending order.
//
// No atomics and no reduction across workgroups: a row of the table is summed by the eight lanes of
// its group, lane `sub` taking entries sub, sub + 8, ... in order, then a butterfly over 4, 2, 1
// (the arrangement of k_mg_restrict), then the vertex's own residual is added to 0.5 x the sum.
// The order depends on the table alone, so two runs give the same bits.  A product and a sum are
// never contracted into an fma.
//
// Every gathered array (b_f, ax_f, m_f, idx, e_c, edge_vertices) is read through a buffer resource
// of its own extent: an index outside the array reads 0 and touches no memory.  Offsets are 32-bit,
// the entry points refuse arrays of 4 GiB or more (check_extents).
#include <hip/hip_runtime.h>

#include "tfem_mg.hpp"  // the launch shape, mg_load / mg_store, the host checks

#pragma clang fp contract(off)

namespace tfem {

template <typename T>
struct MgP2RestrictArgs {
  const int32_t *ptr, *idx;
  const T *mask_c, *mask_f, *b_f, *ax_f;
  T *r_c;
  unsigned n_v, n_f;
};

template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_p2_restrict(const MgP2RestrictArgs<T> a) {
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * (a.n_f - a.n_v) * 4u);
  const ring_rsrc_t r_b = ring_rsrc(a.b_f, a.n_f * unsigned(sizeof(T)));
  const ring_rsrc_t r_ax = ring_rsrc(a.ax_f, a.n_f * unsigned(sizeof(T)));
  const ring_rsrc_t r_mf = ring_rsrc(a.mask_f, a.mask_f ? a.n_f * unsigned(sizeof(T)) : 0u);
  const bool masked_f = a.mask_f != nullptr;
  const unsigned gid = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned row = gid / unsigned(kMgRowLanes);
  const unsigned sub = gid % unsigned(kMgRowLanes);
  T acc = T(0);
  if (row < a.n_v) {
    const unsigned end = unsigned(a.ptr[row + 1]);
    for (unsigned p = unsigned(a.ptr[row]) + sub; p < end; p += unsigned(kMgRowLanes)) {
      const unsigned j = __builtin_amdgcn_raw_buffer_load_b32(r_idx, p * 4u, 0, 0);
      T d = mg_load<T>(r_b, j) - mg_load<T>(r_ax, j);
      if (masked_f) d = mg_load<T>(r_mf, j) * d;
      // j * sizeof(T) wraps for an id of 2^32 / sizeof(T) or more: such an entry counts as 0 too
      acc = acc + (j < a.n_f ? d : T(0));
    }
  }
  // the same bits in the eight lanes of the row (x + y == y + x)
  acc = acc + __shfl_xor(acc, 4, 64);
  acc = acc + __shfl_xor(acc, 2, 64);
  acc = acc + __shfl_xor(acc, 1, 64);
  if (row < a.n_v && sub == 0) {
    T own = mg_load<T>(r_b, row) - mg_load<T>(r_ax, row);  // row < n_v <= n_f
    if (masked_f) own = mg_load<T>(r_mf, row) * own;
    T v = own + T(0.5) * acc;
    if (a.mask_c) v = a.mask_c[row] * v;
    a.r_c[row] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_p2_prolong(const int32_t *__restrict__ edge_vertices,
                                                            const T *__restrict__ mask_f, const T *__restrict__ e_c,
                                                            T *__restrict__ x_f, unsigned n_v, unsigned n_f) {
  const ring_rsrc_t r_ev = ring_rsrc(edge_vertices, 2u * (n_f - n_v) * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_v * unsigned(sizeof(T)));
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * unsigned(sizeof(T)));
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  T v;
  if (i < n_v) {
    v = mg_load<T>(r_e, i);
  } else {
    const unsigned e = i - n_v;
    const unsigned pa = __builtin_amdgcn_raw_buffer_load_b32(r_ev, e * 8u, 0, 0);
    const unsigned pb = __builtin_amdgcn_raw_buffer_load_b32(r_ev, e * 8u + 4u, 0, 0);
    // an endpoint outside the coarse vector counts as 0, also where pa * sizeof(T) wraps
    const T ea = pa < n_v ? mg_load<T>(r_e, pa) : T(0);
    const T eb = pb < n_v ? mg_load<T>(r_e, pb) : T(0);
    v = T(0.5) * (ea + eb);
  }
  if (mask_f) v = mask_f[i] * v;
  mg_store<T>(r_x, i, mg_load<T>(r_x, i) + v);
}

}  // namespace tfem

extern "C" {

int tfem_mg_p2_restrict_residual(const int32_t *ptr, const int32_t *idx, const void *mask_c, const void *mask_f,
                                 const void *b_f, const void *ax_f, void *r_c, int real_bytes, int64_t n_v,
                                 int64_t n_f, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_p2_restrict_residual";
  int st = mg_sizes(name, real_bytes, n_v, n_f);
  if (st != TFEM_OK) return st;
  if (n_f < n_v) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: n_f < n_v (the level holds the vertex DoFs)", name);
  if (n_v == 0) return TFEM_OK;
  const int64_t n_e = n_f - n_v;
  if (!ptr || !r_c || !b_f || !ax_f || (n_e > 0 && !idx))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = n_v < kMgCountLimit ? n_v : kMgCountLimit, f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  const int64_t e = f - c;
  // coarse vector, fine vectors, ptr, idx (two entries per edge), the eight lanes per row
  const int64_t bytes[5] = {c * real_bytes, f * real_bytes, (c + 1) * 4, 2 * e * 4, c * kMgRowLanes};
  st = check_extents("multigrid kernels", bytes, 5);
  if (st != TFEM_OK) return st;
  const struct {
    const void *p;
    int64_t bytes;
  } inputs[6] = {{ptr, bytes[2]}, {idx, bytes[3]}, {mask_c, bytes[0]}, {mask_f, bytes[1]}, {b_f, bytes[1]}, {ax_f, bytes[1]}};
  for (const auto &in : inputs)
    if (mg_overlap(r_c, bytes[0], in.p, in.bytes))
      return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: r_c overlaps an input", name);
  const dim3 grid(unsigned((n_v * kMgRowLanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_P2_RESTRICT(T)                                                                                    \
  {                                                                                                               \
    const MgP2RestrictArgs<T> a{ptr, idx, static_cast<const T *>(mask_c), static_cast<const T *>(mask_f),         \
                                static_cast<const T *>(b_f), static_cast<const T *>(ax_f), static_cast<T *>(r_c), \
                                unsigned(n_v), unsigned(n_f)};                                                    \
    k_mg_p2_restrict<T><<<grid, block, 0, s>>>(a);                                                                \
  }
  if (real_bytes == 8) {
    TFEM_MG_P2_RESTRICT(double)
  } else {
    TFEM_MG_P2_RESTRICT(float)
  }
#undef TFEM_MG_P2_RESTRICT
  return mg_launched(name);
}

int tfem_mg_p2_prolong_add(const int32_t *edge_vertices, const void *mask_f, const void *e_c, void *x_f,
                           int real_bytes, int64_t n_v, int64_t n_f, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_p2_prolong_add";
  int st = mg_sizes(name, real_bytes, n_v, n_f);
  if (st != TFEM_OK) return st;
  if (n_f < n_v) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: n_f < n_v (the level holds the vertex DoFs)", name);
  if (n_v == 0) return TFEM_OK;  // no coarse space: nothing to add (an edge needs two vertices)
  const int64_t n_e = n_f - n_v;
  if (!e_c || !x_f || (n_e > 0 && !edge_vertices)) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = n_v < kMgCountLimit ? n_v : kMgCountLimit, f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  const int64_t bytes[3] = {f * real_bytes, c * real_bytes, 2 * (f - c) * 4};
  st = check_extents("multigrid kernels", bytes, 3);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x_f, bytes[0], e_c, bytes[1]) || mg_overlap(x_f, bytes[0], mask_f, bytes[0]) ||
      mg_overlap(x_f, bytes[0], edge_vertices, bytes[2]))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x_f overlaps an input", name);
  const dim3 grid(unsigned((n_f + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (real_bytes == 8)
    k_mg_p2_prolong<double><<<grid, block, 0, s>>>(edge_vertices, static_cast<const double *>(mask_f),
                                                   static_cast<const double *>(e_c), static_cast<double *>(x_f),
                                                   unsigned(n_v), unsigned(n_f));
  else
    k_mg_p2_prolong<float><<<grid, block, 0, s>>>(edge_vertices, static_cast<const float *>(mask_f),
                                                  static_cast<const float *>(e_c), static_cast<float *>(x_f),
                                                  unsigned(n_v), unsigned(n_f));
  return mg_launched(name);
}

}  // extern "C"
