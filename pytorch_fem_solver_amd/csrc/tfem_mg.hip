// The vector part of a geometric multigrid V-cycle on nested P1 spaces (multigrid.py): the damped
// Jacobi sweep around an operator apply, and the two transfers between a mesh and its red
// refinement (meshgen.refine_uniform).
//
//   smooth   : x = w b                (first sweep on a zero guess, no apply needed)
//              x += w (b - ax)        (ax = K x from an apply launch)
//   restrict : r_c = m_c P^T (m_f (b_f - ax_f))   the residual and P^T in ONE pass: the fine
//              residual is never stored
//   prolong  : x_f += m_f P e_c
//
// P is the P1 prolongation of a red refinement: fine vertex i is the mean of its two `parents`
// (a kept vertex names itself twice), so every weight of P is 0.5 and neither P nor P^T stores a
// value.  P^T is the transposed parent table (ptr, idx): row v lists the fine vertices that name v
// as a parent, in ascending order, a vertex kept from the coarse mesh twice.
//
// No atomics and no reduction across workgroups: a row of P^T is summed by the eight lanes of its
// group, lane `sub` taking entries sub, sub + 8, ... in order, then a butterfly over 4, 2, 1 (the
// arrangement of k_csr_spmv).  The order depends on the table alone, so two runs give the same
// bits.  A product and a sum are never contracted into an fma: the roundings are those of the
// formulas above, evaluated left to right.
//
// Every gathered array (b_f, ax_f, m_f, idx, e_c, parents) is read through a buffer resource of
// its own extent: an index outside the array reads 0 and touches no memory.  Offsets are 32-bit,
// the entry points refuse arrays of 4 GiB or more (check_extents).
#include <hip/hip_runtime.h>

#include "tfem_mg.hpp"  // the launch shape, mg_load / mg_store, the host checks (shared with tfem_mg_multi.hip)

#pragma clang fp contract(off)

namespace tfem {

// VEC: the four arrays are aligned to 16 bytes; a lane moves 16 bytes of each (2 doubles or 4
// floats), the lanes behind the last whole group take the 1 .. 3 entries of the tail one by one.
template <typename T, bool VEC, bool FIRST>
__global__ __launch_bounds__(kMgBlock) void k_mg_smooth(T *__restrict__ x, const T *__restrict__ b,
                                                        const T *__restrict__ ax, const T *__restrict__ w,
                                                        unsigned n) {
  constexpr int kE = VEC ? 16 / int(sizeof(T)) : 1;
  using V = mg_vec<T, kE>;
  const unsigned g = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned n_groups = n / unsigned(kE);
  if (g < n_groups) {
    const V wv = reinterpret_cast<const V *>(w)[g];
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
    if (i < n) {
      if constexpr (FIRST)
        x[i] = w[i] * b[i];
      else
        x[i] = x[i] + w[i] * (b[i] - ax[i]);
    }
  }
}

template <typename T>
struct MgRestrictArgs {
  const int32_t *ptr, *idx;
  const T *mask_c, *mask_f, *b_f, *ax_f;
  T *r_c;
  unsigned n_c, n_f;
};

template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_restrict(const MgRestrictArgs<T> a) {
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * a.n_f * 4u);
  const ring_rsrc_t r_b = ring_rsrc(a.b_f, a.n_f * unsigned(sizeof(T)));
  const ring_rsrc_t r_ax = ring_rsrc(a.ax_f, a.n_f * unsigned(sizeof(T)));
  const ring_rsrc_t r_mf = ring_rsrc(a.mask_f, a.mask_f ? a.n_f * unsigned(sizeof(T)) : 0u);
  const bool masked_f = a.mask_f != nullptr;
  const unsigned gid = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned row = gid / unsigned(kMgRowLanes);
  const unsigned sub = gid % unsigned(kMgRowLanes);
  T acc = T(0);
  if (row < a.n_c) {
    const unsigned end = unsigned(a.ptr[row + 1]);
    for (unsigned p = unsigned(a.ptr[row]) + sub; p < end; p += unsigned(kMgRowLanes)) {
      const unsigned j = __builtin_amdgcn_raw_buffer_load_b32(r_idx, p * 4u, 0, 0);
      T d = mg_load<T>(r_b, j) - mg_load<T>(r_ax, j);
      if (masked_f) d = mg_load<T>(r_mf, j) * d;
      acc = acc + d;
    }
  }
  // the same bits in the eight lanes of the row (x + y == y + x)
  acc = acc + __shfl_xor(acc, 4, 64);
  acc = acc + __shfl_xor(acc, 2, 64);
  acc = acc + __shfl_xor(acc, 1, 64);
  if (row < a.n_c && sub == 0) {
    T v = T(0.5) * acc;
    if (a.mask_c) v = a.mask_c[row] * v;
    a.r_c[row] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(kMgBlock) void k_mg_prolong(const int32_t *__restrict__ parents,
                                                         const T *__restrict__ mask_f, const T *__restrict__ e_c,
                                                         T *__restrict__ x_f, unsigned n_f, unsigned n_c) {
  const ring_rsrc_t r_par = ring_rsrc(parents, 2u * n_f * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_c * unsigned(sizeof(T)));
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * unsigned(sizeof(T)));
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  const unsigned pa = __builtin_amdgcn_raw_buffer_load_b32(r_par, i * 8u, 0, 0);
  const unsigned pb = __builtin_amdgcn_raw_buffer_load_b32(r_par, i * 8u + 4u, 0, 0);
  T v = T(0.5) * (mg_load<T>(r_e, pa) + mg_load<T>(r_e, pb));
  if (mask_f) v = mask_f[i] * v;
  mg_store<T>(r_x, i, mg_load<T>(r_x, i) + v);
}

}  // namespace tfem

extern "C" {

int tfem_mg_smooth(void *x, const void *b, const void *ax, const void *w, int real_bytes, int64_t n, int first,
                   void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_smooth";
  int st = mg_sizes(name, real_bytes, n, 0);
  if (st != TFEM_OK) return st;
  if (n == 0) return TFEM_OK;
  if (!x || !b || !w || (!first && !ax)) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t bytes = (n < kMgCountLimit ? n : kMgCountLimit) * real_bytes;
  st = check_extents("multigrid kernels", &bytes, 1);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x, bytes, b, bytes) || mg_overlap(x, bytes, w, bytes) || (!first && mg_overlap(x, bytes, ax, bytes)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x overlaps an input", name);
  bool vec = true;
  for (const void *p : {static_cast<const void *>(x), b, w, first ? b : ax})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) vec = false;
  const int per_lane = vec ? 16 / real_bytes : 1;
  const int64_t lanes = n / per_lane + (vec ? n % per_lane : 0);
  const dim3 grid(unsigned((lanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_SMOOTH(T, VEC, FIRST)                                                                       \
  k_mg_smooth<T, VEC, FIRST><<<grid, block, 0, s>>>(static_cast<T *>(x), static_cast<const T *>(b),       \
                                                    static_cast<const T *>(ax), static_cast<const T *>(w), \
                                                    unsigned(n))
#define TFEM_MG_SMOOTH_TYPE(T)      \
  if (vec && first) {               \
    TFEM_MG_SMOOTH(T, true, true);  \
  } else if (vec) {                 \
    TFEM_MG_SMOOTH(T, true, false); \
  } else if (first) {               \
    TFEM_MG_SMOOTH(T, false, true); \
  } else {                          \
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

int tfem_mg_restrict_residual(const int32_t *ptr, const int32_t *idx, const void *mask_c, const void *mask_f,
                              const void *b_f, const void *ax_f, void *r_c, int real_bytes, int64_t n_c,
                              int64_t n_f, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_restrict_residual";
  int st = mg_sizes(name, real_bytes, n_c, n_f);
  if (st != TFEM_OK) return st;
  if (n_c == 0) return TFEM_OK;
  if (!ptr || !r_c || (n_f > 0 && (!idx || !b_f || !ax_f)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = n_c < kMgCountLimit ? n_c : kMgCountLimit, f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  // coarse vector, fine vectors, ptr, idx (two entries per fine vertex), the eight lanes per row
  const int64_t bytes[5] = {c * real_bytes, f * real_bytes, (c + 1) * 4, 2 * f * 4, c * kMgRowLanes};
  st = check_extents("multigrid kernels", bytes, 5);
  if (st != TFEM_OK) return st;
  const struct {
    const void *p;
    int64_t bytes;
  } inputs[6] = {{ptr, bytes[2]}, {idx, bytes[3]}, {mask_c, bytes[0]}, {mask_f, bytes[1]}, {b_f, bytes[1]}, {ax_f, bytes[1]}};
  for (const auto &in : inputs)
    if (mg_overlap(r_c, bytes[0], in.p, in.bytes))
      return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: r_c overlaps an input", name);
  const dim3 grid(unsigned((n_c * kMgRowLanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_RESTRICT(T)                                                                                      \
  {                                                                                                              \
    const MgRestrictArgs<T> a{ptr, idx, static_cast<const T *>(mask_c), static_cast<const T *>(mask_f),          \
                              static_cast<const T *>(b_f), static_cast<const T *>(ax_f), static_cast<T *>(r_c),  \
                              unsigned(n_c), unsigned(n_f)};                                                     \
    k_mg_restrict<T><<<grid, block, 0, s>>>(a);                                                                  \
  }
  if (real_bytes == 8) {
    TFEM_MG_RESTRICT(double)
  } else {
    TFEM_MG_RESTRICT(float)
  }
#undef TFEM_MG_RESTRICT
  return mg_launched(name);
}

int tfem_mg_prolong_add(const int32_t *parents, const void *mask_f, const void *e_c, void *x_f, int real_bytes,
                        int64_t n_f, int64_t n_c, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_mg_prolong_add";
  int st = mg_sizes(name, real_bytes, n_f, n_c);
  if (st != TFEM_OK) return st;
  if (n_f == 0) return TFEM_OK;
  if (!parents || !e_c || !x_f) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = n_c < kMgCountLimit ? n_c : kMgCountLimit, f = n_f < kMgCountLimit ? n_f : kMgCountLimit;
  const int64_t bytes[3] = {f * real_bytes, c * real_bytes, 2 * f * 4};
  st = check_extents("multigrid kernels", bytes, 3);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x_f, bytes[0], e_c, bytes[1]) || mg_overlap(x_f, bytes[0], mask_f, bytes[0]) ||
      mg_overlap(x_f, bytes[0], parents, bytes[2]))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x_f overlaps an input", name);
  const dim3 grid(unsigned((n_f + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (real_bytes == 8)
    k_mg_prolong<double><<<grid, block, 0, s>>>(parents, static_cast<const double *>(mask_f),
                                                static_cast<const double *>(e_c), static_cast<double *>(x_f),
                                                unsigned(n_f), unsigned(n_c));
  else
    k_mg_prolong<float><<<grid, block, 0, s>>>(parents, static_cast<const float *>(mask_f),
                                               static_cast<const float *>(e_c), static_cast<float *>(x_f),
                                               unsigned(n_f), unsigned(n_c));
  return mg_launched(name);
}

}  // extern "C"
