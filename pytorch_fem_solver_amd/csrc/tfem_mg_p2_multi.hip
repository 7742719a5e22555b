// The transfers between the P2 space and the P1 space of one mesh (tfem_mg_p2.hip) on a block of
// n_vec vectors: every block is n x n_vec reals, ROW-major (the layout of tfem_mg_multi.hip and
// tfem_p2_apply_rows_multi); the masks, ptr, idx and edge_vertices keep one entry per DoF.  One
// launch for any n_vec; n_vec = 1 IS the launch of tfem_mg_p2.hip.
//
//   restrict : r_c[v][c] = m_c[v] ( m_f[v] (b_f[v][c] - ax_f[v][c])
//                                   + 0.5 sum_j m_f[i_j] (b_f[i_j][c] - ax_f[i_j][c]) )
//   prolong  : x_f[i][c] += m_f[i] ( i < n_v ? e_c[i][c] : 0.5 (e_c[a][c] + e_c[b][c]) )
//
// Per column this is the arithmetic of k_mg_p2_restrict and k_mg_p2_prolong in the same order with
// the same roundings (a product and a sum, never an fma), so column c of every result is bit for bit
// what the single kernel gives for the contiguous copy of column c, whatever n_vec and the alignment
// are.  No atomics, no reduction across workgroups, no LDS.
//
// restrict keeps the eight lanes per vertex row: lane `sub` takes entries sub, sub + 8, ... in order,
// reads idx[p] and m_f[idx[p]] ONCE and then the values of that fine row, one accumulator per column
// in registers; the butterfly over 4, 2, 1 sums every column; then own + 0.5 * sum and the coarse
// mask, by the lanes that store.  prolong has one lane per fine DoF, which reads its two endpoints
// and m_f once; a vertex DoF is its own two endpoints and takes e_c[i] as it is.
// n_vec in {2, 4, 8} with the blocks aligned to the access width min(16, n_vec * sizeof(T)): the
// rows are read and written in accesses of that width.  Any other width or alignment: passes over
// at most 8 columns (restrict) or a loop over the columns (prolong) with one access per value.
//
// Kernels and their instances: k_mg_p2_restrict_multi<T, NV> and k_mg_p2_prolong_multi<T, NV>, two
// types x NV in {2, 4, 8}: 6 each; k_mg_p2_restrict_multi_any<T> and k_mg_p2_prolong_multi_any<T>:
// 2 each; 16 in all.
//
// Everything indexed by data goes through buffer resources of the array's own extent (idx,
// edge_vertices, and the rows of b_f, ax_f, m_f, e_c they select; x_f too).  A row index is clamped
// to the number of rows first: the row behind the last one starts at the extent, so an index outside
// the array -- however large, the 32-bit product with the row size does not wrap -- reads 0 and
// touches nothing.  Offsets are 32-bit, the entry points refuse blocks of 4 GiB or more
// (check_extents).
#include <hip/hip_runtime.h>

#include "tfem_mg.hpp"

#pragma clang fp contract(off)

namespace tfem {

// ----------------------------------------------------------------------------------- restrict
template <typename T>
struct MgP2RestrictMultiArgs {
  const int32_t *ptr, *idx;
  const T *mask_c, *mask_f, *b_f, *ax_f;
  T *r_c;
  unsigned n_v, n_f, n_vec;
};

// b_f, ax_f and r_c aligned to the access width of the row shape.
template <typename T, int NV>
__global__ __launch_bounds__(kMgBlock) void k_mg_p2_restrict_multi(const MgP2RestrictMultiArgs<T> a) {
  using S = MgRowShape<T, NV>;
  using V = mg_vec<T, S::kE>;
  static_assert(S::kAccesses <= kMgRowLanes, "one access per lane of the row's group");
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * (a.n_f - a.n_v) * 4u);
  const ring_rsrc_t r_b = ring_rsrc(a.b_f, a.n_f * S::kRowBytes);
  const ring_rsrc_t r_ax = ring_rsrc(a.ax_f, a.n_f * S::kRowBytes);
  const ring_rsrc_t r_mf = ring_rsrc(a.mask_f, a.mask_f ? a.n_f * unsigned(sizeof(T)) : 0u);
  const bool masked_f = a.mask_f != nullptr;
  const unsigned gid = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned row = gid / unsigned(kMgRowLanes);
  const unsigned sub = gid % unsigned(kMgRowLanes);
  T acc[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c] = T(0);
  if (row < a.n_v) {
    const unsigned end = unsigned(a.ptr[row + 1]);
    for (unsigned p = unsigned(a.ptr[row]) + sub; p < end; p += unsigned(kMgRowLanes)) {
      const unsigned j = min(__builtin_amdgcn_raw_buffer_load_b32(r_idx, p * 4u, 0, 0), a.n_f);
      const T m = masked_f ? mg_load<T>(r_mf, j) : T(1);
#pragma unroll
      for (int l = 0; l < S::kAccesses; ++l) {
        T bv[S::kE], av[S::kE];
        mg_load_chunk<T, S::kE>(r_b, j * S::kRowBytes + unsigned(l) * S::kAccessBytes, bv);
        mg_load_chunk<T, S::kE>(r_ax, j * S::kRowBytes + unsigned(l) * S::kAccessBytes, av);
#pragma unroll
        for (int e = 0; e < S::kE; ++e) {
          T d = bv[e] - av[e];
          if (masked_f) d = m * d;
          acc[l * S::kE + e] = acc[l * S::kE + e] + d;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c] = mg_row_sum(acc[c]);
  // every lane of the group holds every sum: lane `sub` finishes and stores access `sub` of the row
  if (row < a.n_v && sub < unsigned(S::kAccesses)) {
    T sum[S::kE];
#pragma unroll
    for (int e = 0; e < S::kE; ++e) sum[e] = acc[e];
#pragma unroll
    for (int l = 1; l < S::kAccesses; ++l) {
#pragma unroll
      for (int e = 0; e < S::kE; ++e) sum[e] = sub == unsigned(l) ? acc[l * S::kE + e] : sum[e];
    }
    T bv[S::kE], av[S::kE];  // the vertex's own residual: row < n_v <= n_f
    mg_load_chunk<T, S::kE>(r_b, row * S::kRowBytes + sub * S::kAccessBytes, bv);
    mg_load_chunk<T, S::kE>(r_ax, row * S::kRowBytes + sub * S::kAccessBytes, av);
    const T m = masked_f ? mg_load<T>(r_mf, row) : T(1);
    const T mc = a.mask_c ? a.mask_c[row] : T(1);
    V out;
#pragma unroll
    for (int e = 0; e < S::kE; ++e) {
      T own = bv[e] - av[e];
      if (masked_f) own = m * own;
      T v = own + T(0.5) * sum[e];
      if (a.mask_c) v = mc * v;
      out[e] = v;
    }
    reinterpret_cast<V *>(a.r_c + size_t(row) * NV)[sub] = out;
  }
}

// Any width and alignment: columns c0 .. c0 + 8 per pass, one access per value.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_p2_restrict_multi_any(const MgP2RestrictMultiArgs<T> a) {
  const unsigned block_bytes = a.n_f * a.n_vec * unsigned(sizeof(T));
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * (a.n_f - a.n_v) * 4u);
  const ring_rsrc_t r_b = ring_rsrc(a.b_f, block_bytes);
  const ring_rsrc_t r_ax = ring_rsrc(a.ax_f, block_bytes);
  const ring_rsrc_t r_mf = ring_rsrc(a.mask_f, a.mask_f ? a.n_f * unsigned(sizeof(T)) : 0u);
  const bool masked_f = a.mask_f != nullptr;
  const unsigned gid = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned row = gid / unsigned(kMgRowLanes);
  const unsigned sub = gid % unsigned(kMgRowLanes);
  unsigned start = 0, end = 0;
  T mc = T(1), m_own = T(1);
  if (row < a.n_v) {
    start = unsigned(a.ptr[row]) + sub;
    end = unsigned(a.ptr[row + 1]);
    if (a.mask_c) mc = a.mask_c[row];
    if (masked_f) m_own = mg_load<T>(r_mf, row);
  }
  for (unsigned c0 = 0; c0 < a.n_vec; c0 += unsigned(kMgPass)) {
    const unsigned nc = min(unsigned(kMgPass), a.n_vec - c0);  // the same in every lane
    T acc[kMgPass];
#pragma unroll
    for (int c = 0; c < kMgPass; ++c) acc[c] = T(0);
    for (unsigned p = start; p < end; p += unsigned(kMgRowLanes)) {
      const unsigned j = min(__builtin_amdgcn_raw_buffer_load_b32(r_idx, p * 4u, 0, 0), a.n_f);
      const T m = masked_f ? mg_load<T>(r_mf, j) : T(1);
      const unsigned first = j * a.n_vec + c0;  // row n_f starts at the extent: 0 from there on
#pragma unroll
      for (int c = 0; c < kMgPass; ++c)
        if (unsigned(c) < nc) {
          T d = mg_load<T>(r_b, first + unsigned(c)) - mg_load<T>(r_ax, first + unsigned(c));
          if (masked_f) d = m * d;
          acc[c] = acc[c] + d;
        }
    }
    T mine = T(0);
#pragma unroll
    for (int c = 0; c < kMgPass; ++c) {
      const T sum = mg_row_sum(acc[c]);
      mine = sub == unsigned(c) ? sum : mine;
    }
    if (row < a.n_v && sub < nc) {  // lane `sub` finishes and stores column c0 + sub
      const unsigned at = row * a.n_vec + c0 + sub;  // row < n_v <= n_f: inside the fine blocks
      T own = mg_load<T>(r_b, at) - mg_load<T>(r_ax, at);
      if (masked_f) own = m_own * own;
      T v = own + T(0.5) * mine;
      if (a.mask_c) v = mc * v;
      a.r_c[size_t(row) * a.n_vec + c0 + sub] = v;
    }
  }
}

// ------------------------------------------------------------------------------------ prolong
// One lane per fine DoF; e_c and x_f aligned to the access width of the row shape.
template <typename T, int NV>
__global__ __launch_bounds__(kMgBlock) void k_mg_p2_prolong_multi(const int32_t *__restrict__ edge_vertices,
                                                                  const T *__restrict__ mask_f,
                                                                  const T *__restrict__ e_c, T *__restrict__ x_f,
                                                                  unsigned n_v, unsigned n_f) {
  using S = MgRowShape<T, NV>;
  const ring_rsrc_t r_ev = ring_rsrc(edge_vertices, 2u * (n_f - n_v) * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_v * S::kRowBytes);
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * S::kRowBytes);
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  const bool vertex = i < n_v;
  unsigned pa = i, pb = i;  // a vertex DoF: its own row of e_c
  if (!vertex) {
    const unsigned e = i - n_v;
    pa = min(__builtin_amdgcn_raw_buffer_load_b32(r_ev, e * 8u, 0, 0), n_v);
    pb = min(__builtin_amdgcn_raw_buffer_load_b32(r_ev, e * 8u + 4u, 0, 0), n_v);
  }
  const bool masked = mask_f != nullptr;
  const T m = masked ? mask_f[i] : T(1);
#pragma unroll
  for (int l = 0; l < S::kAccesses; ++l) {
    const unsigned at = unsigned(l) * S::kAccessBytes;
    T ea[S::kE], eb[S::kE], xv[S::kE];
    mg_load_chunk<T, S::kE>(r_e, pa * S::kRowBytes + at, ea);
    mg_load_chunk<T, S::kE>(r_e, pb * S::kRowBytes + at, eb);
    mg_load_chunk<T, S::kE>(r_x, i * S::kRowBytes + at, xv);
#pragma unroll
    for (int e = 0; e < S::kE; ++e) {
      T v = vertex ? ea[e] : T(0.5) * (ea[e] + eb[e]);
      if (masked) v = m * v;
      xv[e] = xv[e] + v;
    }
    mg_store_chunk<T, S::kE>(r_x, i * S::kRowBytes + at, xv);
  }
}

// Any width and alignment: the columns of the row one by one.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_p2_prolong_multi_any(const int32_t *__restrict__ edge_vertices,
                                                                      const T *__restrict__ mask_f,
                                                                      const T *__restrict__ e_c,
                                                                      T *__restrict__ x_f, unsigned n_v,
                                                                      unsigned n_f, unsigned n_vec) {
  const ring_rsrc_t r_ev = ring_rsrc(edge_vertices, 2u * (n_f - n_v) * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_v * n_vec * unsigned(sizeof(T)));
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * n_vec * unsigned(sizeof(T)));
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  const bool vertex = i < n_v;
  unsigned pa = i, pb = i;
  if (!vertex) {
    const unsigned e = i - n_v;
    pa = min(__builtin_amdgcn_raw_buffer_load_b32(r_ev, e * 8u, 0, 0), n_v);
    pb = min(__builtin_amdgcn_raw_buffer_load_b32(r_ev, e * 8u + 4u, 0, 0), n_v);
  }
  const bool masked = mask_f != nullptr;
  const T m = masked ? mask_f[i] : T(1);
  for (unsigned c = 0; c < n_vec; ++c) {  // row n_v starts at the extent: 0 from there on
    const T ea = mg_load<T>(r_e, pa * n_vec + c), eb = mg_load<T>(r_e, pb * n_vec + c);
    T v = vertex ? ea : T(0.5) * (ea + eb);
    if (masked) v = m * v;
    mg_store<T>(r_x, i * n_vec + c, mg_load<T>(r_x, i * n_vec + c) + v);
  }
}

}  // namespace tfem

extern "C" {

int tfem_mg_p2_restrict_residual_multi(const int32_t *ptr, const int32_t *idx, const void *mask_c,
                                       const void *mask_f, const void *b_f, const void *ax_f, void *r_c,
                                       int real_bytes, int64_t n_v, int64_t n_f, int64_t n_vec, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_p2_restrict_residual_multi";
  int st = mg_sizes_multi(name, real_bytes, n_v, n_f, n_vec);
  if (st != TFEM_OK) return st;
  if (n_vec == 1)
    return tfem_mg_p2_restrict_residual(ptr, idx, mask_c, mask_f, b_f, ax_f, r_c, real_bytes, n_v, n_f, stream);
  if (n_f < n_v) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: n_f < n_v (the level holds the vertex DoFs)", name);
  if (n_v == 0) return TFEM_OK;
  const int64_t n_e = n_f - n_v;
  if (!ptr || !r_c || !b_f || !ax_f || (n_e > 0 && !idx))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = n_v < kMgCountLimit ? n_v : kMgCountLimit, f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  // coarse block, fine blocks, ptr, idx (two entries per edge), the eight lanes per row, the masks
  // (one entry per DoF)
  const int64_t bytes[7] = {mg_block_bytes(n_v, n_vec, real_bytes), mg_block_bytes(n_f, n_vec, real_bytes),
                            (c + 1) * 4, 2 * (f - c) * 4, c * kMgRowLanes, c * real_bytes, f * real_bytes};
  st = check_extents("multigrid kernels", bytes, 7);
  if (st != TFEM_OK) return st;
  const struct {
    const void *p;
    int64_t bytes;
  } inputs[6] = {{ptr, bytes[2]}, {idx, bytes[3]}, {mask_c, bytes[5]}, {mask_f, bytes[6]}, {b_f, bytes[1]}, {ax_f, bytes[1]}};
  for (const auto &in : inputs)
    if (mg_overlap(r_c, bytes[0], in.p, in.bytes))
      return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: r_c overlaps an input", name);
  const int nv = mg_row_width(n_vec, real_bytes, {b_f, ax_f, r_c});
  const dim3 grid(unsigned((n_v * kMgRowLanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_P2_RESTRICT(T)                                                                                  \
  {                                                                                                             \
    const MgP2RestrictMultiArgs<T> a{ptr, idx, static_cast<const T *>(mask_c), static_cast<const T *>(mask_f),  \
                                     static_cast<const T *>(b_f), static_cast<const T *>(ax_f),                 \
                                     static_cast<T *>(r_c), unsigned(n_v), unsigned(n_f), unsigned(n_vec)};     \
    switch (nv) {                                                                                               \
      case 2: k_mg_p2_restrict_multi<T, 2><<<grid, block, 0, s>>>(a); break;                                    \
      case 4: k_mg_p2_restrict_multi<T, 4><<<grid, block, 0, s>>>(a); break;                                    \
      case 8: k_mg_p2_restrict_multi<T, 8><<<grid, block, 0, s>>>(a); break;                                    \
      default: k_mg_p2_restrict_multi_any<T><<<grid, block, 0, s>>>(a);                                         \
    }                                                                                                           \
  }
  if (real_bytes == 8) {
    TFEM_MG_P2_RESTRICT(double)
  } else {
    TFEM_MG_P2_RESTRICT(float)
  }
#undef TFEM_MG_P2_RESTRICT
  return mg_launched(name);
}

int tfem_mg_p2_prolong_add_multi(const int32_t *edge_vertices, const void *mask_f, const void *e_c, void *x_f,
                                 int real_bytes, int64_t n_v, int64_t n_f, int64_t n_vec, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_p2_prolong_add_multi";
  int st = mg_sizes_multi(name, real_bytes, n_v, n_f, n_vec);
  if (st != TFEM_OK) return st;
  if (n_vec == 1) return tfem_mg_p2_prolong_add(edge_vertices, mask_f, e_c, x_f, real_bytes, n_v, n_f, stream);
  if (n_f < n_v) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: n_f < n_v (the level holds the vertex DoFs)", name);
  if (n_v == 0) return TFEM_OK;  // no coarse space: nothing to add (an edge needs two vertices)
  const int64_t n_e = n_f - n_v;
  if (!e_c || !x_f || (n_e > 0 && !edge_vertices)) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = n_v < kMgCountLimit ? n_v : kMgCountLimit, f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  // fine block, coarse block, edge_vertices, the mask (one entry per DoF)
  const int64_t bytes[4] = {mg_block_bytes(n_f, n_vec, real_bytes), mg_block_bytes(n_v, n_vec, real_bytes),
                            2 * (f - c) * 4, f * real_bytes};
  st = check_extents("multigrid kernels", bytes, 4);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x_f, bytes[0], e_c, bytes[1]) || mg_overlap(x_f, bytes[0], mask_f, bytes[3]) ||
      mg_overlap(x_f, bytes[0], edge_vertices, bytes[2]))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x_f overlaps an input", name);
  const int nv = mg_row_width(n_vec, real_bytes, {e_c, static_cast<const void *>(x_f)});
  const dim3 grid(unsigned((n_f + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_P2_PROLONG(T)                                                                                        \
  {                                                                                                                  \
    const T *m = static_cast<const T *>(mask_f), *e = static_cast<const T *>(e_c);                                   \
    T *xf = static_cast<T *>(x_f);                                                                                   \
    const unsigned nv_ = unsigned(n_v), nf_ = unsigned(n_f);                                                         \
    switch (nv) {                                                                                                    \
      case 2: k_mg_p2_prolong_multi<T, 2><<<grid, block, 0, s>>>(edge_vertices, m, e, xf, nv_, nf_); break;          \
      case 4: k_mg_p2_prolong_multi<T, 4><<<grid, block, 0, s>>>(edge_vertices, m, e, xf, nv_, nf_); break;          \
      case 8: k_mg_p2_prolong_multi<T, 8><<<grid, block, 0, s>>>(edge_vertices, m, e, xf, nv_, nf_); break;          \
      default: k_mg_p2_prolong_multi_any<T><<<grid, block, 0, s>>>(edge_vertices, m, e, xf, nv_, nf_, unsigned(n_vec)); \
    }                                                                                                                \
  }
  if (real_bytes == 8) {
    TFEM_MG_P2_PROLONG(double)
  } else {
    TFEM_MG_P2_PROLONG(float)
  }
#undef TFEM_MG_P2_PROLONG
  return mg_launched(name);
}

}  // extern "C"
