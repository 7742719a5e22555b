// The vector part of the multigrid V-cycle (tfem_mg.hip) on a block of n_vec vectors: every block is
// n x n_vec reals, ROW-major (the n_vec values of a DoF are consecutive: the layout of
// tfem_p1_apply_rings_multi, tfem_csr_spmm and the tfem_cg_* launches); w, the masks, ptr, idx and
// parents keep one entry per DoF.  One launch for any n_vec; n_vec = 1 IS the launch of tfem_mg.hip.
//
//   smooth   : x[i][c] = w[i] b[i][c]                        (first)
//              x[i][c] = x[i][c] + w[i] (b[i][c] - ax[i][c])
//   restrict : r_c[v][c] = m_c[v] 0.5 sum_j m_f[i_j] (b_f[i_j][c] - ax_f[i_j][c])
//   prolong  : x_f[i][c] += m_f[i] 0.5 (e_c[a][c] + e_c[b][c])
//
// Per column this is the arithmetic of the single kernels in the same order with the same roundings
// (a product and a sum, never an fma), so column c of every result is bit for bit what the single
// kernel gives for the contiguous copy of column c, whatever n_vec is.  No atomics, no reduction
// across workgroups.
//
// smooth streams the flat block: 16 bytes per lane when x, b and ax are aligned to 16 bytes, the
// tail one by one.  A group of 2 doubles or 4 floats may lie across rows (an odd n_vec; n_vec = 2
// or 3 with floats), so every value of the group takes the w of its own row: row(e0 + t) = row(e0)
// + [r >= n_vec] + [r >= 2 n_vec] with r = e0 mod n_vec + t <= n_vec + 2, one division per lane.
//
// restrict keeps the eight lanes per coarse row of k_mg_restrict: lane `sub` takes entries sub,
// sub + 8, ... in order, reads idx[p] and m_f[idx[p]] ONCE and then the values of that fine row, one
// accumulator per column in registers, and the butterfly over 4, 2, 1 sums every column.  prolong
// has one lane per fine DoF, which reads its two parents and m_f once.
// n_vec in {2, 4, 8} with the blocks aligned to the access width min(16, n_vec * sizeof(T)): the
// rows are read and written in accesses of that width.  Any other width or alignment: passes over
// at most 8 columns (restrict) or a loop over the columns (prolong) with one access per value.
//
// Everything indexed by data goes through buffer resources of the array's own extent (idx, parents,
// and the rows of b_f, ax_f, m_f, e_c, x_f they select).  A row index is clamped to the number of
// rows first: the row behind the last one starts at the extent, so an index outside the array --
// however large, the 32-bit product with the row size does not wrap -- reads 0 and touches nothing.
// Offsets are 32-bit, the entry points refuse blocks of 4 GiB or more (check_extents).
#include <hip/hip_runtime.h>

#include "tfem_mg.hpp"

#pragma clang fp contract(off)

namespace tfem {

// ------------------------------------------------------------------------------------- smooth
// total = n * n_vec values.  VEC: x, b and ax are aligned to 16 bytes; w has one entry per row and
// is read entry by entry.
template <typename T, bool VEC, bool FIRST>
__global__ __launch_bounds__(kMgBlock) void k_mg_smooth_multi(T *__restrict__ x, const T *__restrict__ b,
                                                              const T *__restrict__ ax,
                                                              const T *__restrict__ w, unsigned total,
                                                              unsigned n_vec) {
  constexpr int kE = VEC ? 16 / int(sizeof(T)) : 1;
  using V = mg_vec<T, kE>;
  const unsigned g = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned n_groups = total / unsigned(kE);
  if (g < n_groups) {
    const unsigned e0 = g * unsigned(kE);
    const unsigned row = e0 / n_vec;
    const unsigned rem = e0 - row * n_vec;
    V wv;
#pragma unroll
    for (int t = 0; t < kE; ++t) {
      const unsigned r = rem + unsigned(t);  // < n_vec + 3 <= 3 n_vec for n_vec >= 2
      wv[t] = w[row + (r >= n_vec ? 1u : 0u) + (r >= 2u * n_vec ? 1u : 0u)];
    }
    const V bv = reinterpret_cast<const V *>(b)[g];
    V xv;
    if constexpr (FIRST) {
      xv = wv * bv;
    } else {
      const V av = reinterpret_cast<const V *>(ax)[g];
      xv = reinterpret_cast<const V *>(x)[g];
      xv = xv + wv * (bv - av);
    }
    reinterpret_cast<V *>(x)[g] = xv;
  } else if constexpr (VEC) {
    const unsigned i = n_groups * unsigned(kE) + (g - n_groups);
    if (i < total) {
      const T wi = w[i / n_vec];
      if constexpr (FIRST)
        x[i] = wi * b[i];
      else
        x[i] = x[i] + wi * (b[i] - ax[i]);
    }
  }
}

// ----------------------------------------------------------------------------------- restrict
template <typename T>
struct MgRestrictMultiArgs {
  const int32_t *ptr, *idx;
  const T *mask_c, *mask_f, *b_f, *ax_f;
  T *r_c;
  unsigned n_c, n_f, n_vec;
};

// b_f, ax_f and r_c aligned to the access width of the row shape.
template <typename T, int NV>
__global__ __launch_bounds__(kMgBlock) void k_mg_restrict_multi(const MgRestrictMultiArgs<T> a) {
  using S = MgRowShape<T, NV>;
  using V = mg_vec<T, S::kE>;
  static_assert(S::kAccesses <= kMgRowLanes, "one access per lane of the row's group");
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * a.n_f * 4u);
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
  if (row < a.n_c) {
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
  // every lane of the group holds every sum: lane `sub` stores access `sub` of the row
  if (row < a.n_c && sub < unsigned(S::kAccesses)) {
    V out;
#pragma unroll
    for (int e = 0; e < S::kE; ++e) out[e] = acc[e];
#pragma unroll
    for (int l = 1; l < S::kAccesses; ++l) {
#pragma unroll
      for (int e = 0; e < S::kE; ++e) out[e] = sub == unsigned(l) ? acc[l * S::kE + e] : out[e];
    }
#pragma unroll
    for (int e = 0; e < S::kE; ++e) out[e] = T(0.5) * out[e];
    if (a.mask_c) {
      const T mc = a.mask_c[row];
#pragma unroll
      for (int e = 0; e < S::kE; ++e) out[e] = mc * out[e];
    }
    reinterpret_cast<V *>(a.r_c + size_t(row) * NV)[sub] = out;
  }
}

// Any width and alignment: columns c0 .. c0 + 8 per pass, one access per value.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_restrict_multi_any(const MgRestrictMultiArgs<T> a) {
  const unsigned block_bytes = a.n_f * a.n_vec * unsigned(sizeof(T));
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * a.n_f * 4u);
  const ring_rsrc_t r_b = ring_rsrc(a.b_f, block_bytes);
  const ring_rsrc_t r_ax = ring_rsrc(a.ax_f, block_bytes);
  const ring_rsrc_t r_mf = ring_rsrc(a.mask_f, a.mask_f ? a.n_f * unsigned(sizeof(T)) : 0u);
  const bool masked_f = a.mask_f != nullptr;
  const unsigned gid = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned row = gid / unsigned(kMgRowLanes);
  const unsigned sub = gid % unsigned(kMgRowLanes);
  unsigned start = 0, end = 0;
  T mc = T(1);
  if (row < a.n_c) {
    start = unsigned(a.ptr[row]) + sub;
    end = unsigned(a.ptr[row + 1]);
    if (a.mask_c) mc = a.mask_c[row];
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
    if (row < a.n_c && sub < nc) {
      T v = T(0.5) * mine;
      if (a.mask_c) v = mc * v;
      a.r_c[size_t(row) * a.n_vec + c0 + sub] = v;
    }
  }
}

// ------------------------------------------------------------------------------------ prolong
// One lane per fine DoF; e_c and x_f aligned to the access width of the row shape.
template <typename T, int NV>
__global__ __launch_bounds__(kMgBlock) void k_mg_prolong_multi(const int32_t *__restrict__ parents,
                                                               const T *__restrict__ mask_f,
                                                               const T *__restrict__ e_c, T *__restrict__ x_f,
                                                               unsigned n_f, unsigned n_c) {
  using S = MgRowShape<T, NV>;
  const ring_rsrc_t r_par = ring_rsrc(parents, 2u * n_f * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_c * S::kRowBytes);
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * S::kRowBytes);
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  const unsigned pa = min(__builtin_amdgcn_raw_buffer_load_b32(r_par, i * 8u, 0, 0), n_c);
  const unsigned pb = min(__builtin_amdgcn_raw_buffer_load_b32(r_par, i * 8u + 4u, 0, 0), n_c);
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
      T v = T(0.5) * (ea[e] + eb[e]);
      if (masked) v = m * v;
      xv[e] = xv[e] + v;
    }
    mg_store_chunk<T, S::kE>(r_x, i * S::kRowBytes + at, xv);
  }
}

// Any width and alignment: the columns of the row one by one.
template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_prolong_multi_any(const int32_t *__restrict__ parents,
                                                                   const T *__restrict__ mask_f,
                                                                   const T *__restrict__ e_c,
                                                                   T *__restrict__ x_f, unsigned n_f,
                                                                   unsigned n_c, unsigned n_vec) {
  const ring_rsrc_t r_par = ring_rsrc(parents, 2u * n_f * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_c * n_vec * unsigned(sizeof(T)));
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * n_vec * unsigned(sizeof(T)));
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  const unsigned pa = min(__builtin_amdgcn_raw_buffer_load_b32(r_par, i * 8u, 0, 0), n_c);
  const unsigned pb = min(__builtin_amdgcn_raw_buffer_load_b32(r_par, i * 8u + 4u, 0, 0), n_c);
  const bool masked = mask_f != nullptr;
  const T m = masked ? mask_f[i] : T(1);
  for (unsigned c = 0; c < n_vec; ++c) {  // row n_c starts at the extent: 0 from there on
    T v = T(0.5) * (mg_load<T>(r_e, pa * n_vec + c) + mg_load<T>(r_e, pb * n_vec + c));
    if (masked) v = m * v;
    mg_store<T>(r_x, i * n_vec + c, mg_load<T>(r_x, i * n_vec + c) + v);
  }
}

}  // namespace tfem

extern "C" {

int tfem_mg_smooth_multi(void *x, const void *b, const void *ax, const void *w, int real_bytes, int64_t n,
                         int64_t n_vec, int first, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_smooth_multi";
  int st = mg_sizes_multi(name, real_bytes, n, 0, n_vec);
  if (st != TFEM_OK) return st;
  if (n_vec == 1) return tfem_mg_smooth(x, b, ax, w, real_bytes, n, first, stream);
  if (n == 0) return TFEM_OK;
  if (!x || !b || !w || (!first && !ax)) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t bytes = mg_block_bytes(n, n_vec, real_bytes);
  st = check_extents("multigrid kernels", &bytes, 1);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x, bytes, b, bytes) || mg_overlap(x, bytes, w, n * real_bytes) ||
      (!first && mg_overlap(x, bytes, ax, bytes)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x overlaps an input", name);
  bool vec = true;
  for (const void *p : {static_cast<const void *>(x), b, first ? b : ax})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) vec = false;
  const int per_lane = vec ? 16 / real_bytes : 1;
  const int64_t total = n * n_vec;
  const int64_t lanes = total / per_lane + (vec ? total % per_lane : 0);
  const dim3 grid(unsigned((lanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_SMOOTH(T, VEC, FIRST)                                                                     \
  k_mg_smooth_multi<T, VEC, FIRST><<<grid, block, 0, s>>>(static_cast<T *>(x), static_cast<const T *>(b), \
                                                          static_cast<const T *>(ax),                     \
                                                          static_cast<const T *>(w), unsigned(total),     \
                                                          unsigned(n_vec))
#define TFEM_MG_SMOOTH_TYPE(T)       \
  if (vec && first) {                \
    TFEM_MG_SMOOTH(T, true, true);   \
  } else if (vec) {                  \
    TFEM_MG_SMOOTH(T, true, false);  \
  } else if (first) {                \
    TFEM_MG_SMOOTH(T, false, true);  \
  } else {                           \
    TFEM_MG_SMOOTH(T, false, false); \
  }
  if (real_bytes == 8) {
    TFEM_MG_SMOOTH_TYPE(double)
  } else {
    TFEM_MG_SMOOTH_TYPE(float)
  }
#undef TFEM_MG_SMOOTH_TYPE
#undef TFEM_MG_SMOOTH
  return mg_launched(name);
}

int tfem_mg_restrict_residual_multi(const int32_t *ptr, const int32_t *idx, const void *mask_c, const void *mask_f,
                                    const void *b_f, const void *ax_f, void *r_c, int real_bytes, int64_t n_c,
                                    int64_t n_f, int64_t n_vec, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_restrict_residual_multi";
  int st = mg_sizes_multi(name, real_bytes, n_c, n_f, n_vec);
  if (st != TFEM_OK) return st;
  if (n_vec == 1)
    return tfem_mg_restrict_residual(ptr, idx, mask_c, mask_f, b_f, ax_f, r_c, real_bytes, n_c, n_f, stream);
  if (n_c == 0) return TFEM_OK;
  if (!ptr || !r_c || (n_f > 0 && (!idx || !b_f || !ax_f)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = n_c < kMgCountLimit ? n_c : kMgCountLimit, f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  // coarse block, fine blocks, ptr, idx (two entries per fine vertex), the eight lanes per row,
  // the masks (one entry per DoF)
  const int64_t bytes[7] = {mg_block_bytes(n_c, n_vec, real_bytes), mg_block_bytes(n_f, n_vec, real_bytes),
                            (c + 1) * 4, 2 * f * 4, c * kMgRowLanes, c * real_bytes, f * real_bytes};
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
  const dim3 grid(unsigned((n_c * kMgRowLanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_RESTRICT(T)                                                                                     \
  {                                                                                                             \
    const MgRestrictMultiArgs<T> a{ptr, idx, static_cast<const T *>(mask_c), static_cast<const T *>(mask_f),    \
                                   static_cast<const T *>(b_f), static_cast<const T *>(ax_f),                   \
                                   static_cast<T *>(r_c), unsigned(n_c), unsigned(n_f), unsigned(n_vec)};       \
    switch (nv) {                                                                                               \
      case 2: k_mg_restrict_multi<T, 2><<<grid, block, 0, s>>>(a); break;                                       \
      case 4: k_mg_restrict_multi<T, 4><<<grid, block, 0, s>>>(a); break;                                       \
      case 8: k_mg_restrict_multi<T, 8><<<grid, block, 0, s>>>(a); break;                                       \
      default: k_mg_restrict_multi_any<T><<<grid, block, 0, s>>>(a);                                            \
    }                                                                                                           \
  }
  if (real_bytes == 8) {
    TFEM_MG_RESTRICT(double)
  } else {
    TFEM_MG_RESTRICT(float)
  }
#undef TFEM_MG_RESTRICT
  return mg_launched(name);
}

int tfem_mg_prolong_add_multi(const int32_t *parents, const void *mask_f, const void *e_c, void *x_f, int real_bytes,
                              int64_t n_f, int64_t n_c, int64_t n_vec, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_prolong_add_multi";
  int st = mg_sizes_multi(name, real_bytes, n_f, n_c, n_vec);
  if (st != TFEM_OK) return st;
  if (n_vec == 1) return tfem_mg_prolong_add(parents, mask_f, e_c, x_f, real_bytes, n_f, n_c, stream);
  if (n_f == 0) return TFEM_OK;
  if (!parents || !e_c || !x_f) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  // fine block, coarse block, parents, the mask (one entry per DoF)
  const int64_t bytes[4] = {mg_block_bytes(n_f, n_vec, real_bytes), mg_block_bytes(n_c, n_vec, real_bytes), 2 * f * 4,
                            f * real_bytes};
  st = check_extents("multigrid kernels", bytes, 4);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x_f, bytes[0], e_c, bytes[1]) || mg_overlap(x_f, bytes[0], mask_f, bytes[3]) ||
      mg_overlap(x_f, bytes[0], parents, bytes[2]))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x_f overlaps an input", name);
  const int nv = mg_row_width(n_vec, real_bytes, {e_c, static_cast<const void *>(x_f)});
  const dim3 grid(unsigned((n_f + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_PROLONG(T)                                                                                          \
  {                                                                                                                 \
    const T *m = static_cast<const T *>(mask_f), *e = static_cast<const T *>(e_c);                                  \
    T *xf = static_cast<T *>(x_f);                                                                                  \
    switch (nv) {                                                                                                   \
      case 2: k_mg_prolong_multi<T, 2><<<grid, block, 0, s>>>(parents, m, e, xf, unsigned(n_f), unsigned(n_c)); break; \
      case 4: k_mg_prolong_multi<T, 4><<<grid, block, 0, s>>>(parents, m, e, xf, unsigned(n_f), unsigned(n_c)); break; \
      case 8: k_mg_prolong_multi<T, 8><<<grid, block, 0, s>>>(parents, m, e, xf, unsigned(n_f), unsigned(n_c)); break; \
      default:                                                                                                      \
        k_mg_prolong_multi_any<T><<<grid, block, 0, s>>>(parents, m, e, xf, unsigned(n_f), unsigned(n_c),           \
                                                         unsigned(n_vec));                                          \
    }                                                                                                               \
  }
  if (real_bytes == 8) {
    TFEM_MG_PROLONG(double)
  } else {
    TFEM_MG_PROLONG(float)
  }
#undef TFEM_MG_PROLONG
  return mg_launched(name);
}

}  // extern "C"
