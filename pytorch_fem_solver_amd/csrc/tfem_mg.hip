// The vector part of a multigrid V-cycle (multigrid.py): the damped Jacobi sweep around an operator
// apply, and the two transfers between a level and the one below it, on one vector or on a block of
// n_vec vectors.  A block is n x n_vec reals, ROW-major (the n_vec values of a DoF are consecutive:
// the layout of tfem_p1_apply_rings_multi, tfem_csr_spmm and the tfem_cg_* launches); w, the masks,
// ptr, idx and the table of P keep one entry per DoF.
//
//   smooth   : x = w b                (first sweep on a zero guess, no apply needed)
//              x += w (b - ax)        (ax = K x from an apply launch)
//   restrict : r_c = m_c P^T (m_f (b_f - ax_f))   the residual and P^T in ONE pass: the fine
//              residual is never stored
//   prolong  : x_f += m_f P e_c
//
// The transfers come in two kinds (tfem_mg.hpp), the red refinement of a P1 mesh (MgRefine,
// tfem_mg_*) and the step from P1 to P2 on one mesh (MgP2, tfem_mg_p2_*), with every weight 0.5 or
// 1: neither P nor P^T stores a value.
//
//   MgRefine : r_c[v] = m_c[v] 0.5 sum_j m_f[i_j] (b_f - ax_f)[i_j]
//              x_f[i] += m_f[i] 0.5 (e_c[a] + e_c[b])                 (a, b) = parents[i]
//   MgP2     : r_c[v] = m_c[v] ( m_f[v] (b_f - ax_f)[v] + 0.5 sum_j m_f[i_j] (b_f - ax_f)[i_j] )
//              x_f[i] += m_f[i] ( i < n_v ? e_c[i] : 0.5 (e_c[a] + e_c[b]) )   (a, b) = edge_vertices[i - n_v]
//
// with i_j the entries of row v of (ptr, idx), the transposed table.  No atomics and no reduction
// across workgroups: a row of P^T is summed by the eight lanes of its group, lane `sub` taking
// entries sub, sub + 8, ... in order and reading idx[p] and m_f[idx[p]] ONCE, one accumulator per
// column in registers, then a butterfly over 4, 2, 1 (the arrangement of k_csr_spmv).  prolong has
// one lane per fine DoF, which reads its two table entries and m_f once.  The order depends on the
// table alone, so two runs give the same bits; a product and a sum are never contracted into an
// fma, and the roundings are those of the formulas above, evaluated left to right -- per column, so
// column c of a block result is bit for bit the single-vector result for the contiguous copy of
// column c, whatever n_vec and the alignment are.
//
// Row shapes: n_vec = 1 (a single vector), and n_vec in {2, 4, 8} with the blocks aligned to the
// access width min(16, n_vec * sizeof(T)), are the instances <T, Kind, NV>, which read and write a
// row in accesses of that width.  Any other width or alignment: the _any instances, passes over at
// most 8 columns (restrict) or a loop over the columns (prolong) with one access per value.
// Instances: smooth 2 types x aligned or not x first or not, single and block: 16; restrict and
// prolong 2 types x 2 kinds x (4 shapes + any): 20 each; 56 in all.
//
// Everything indexed by data goes through buffer resources of the array's own extent (idx, the table
// of P, and the rows of b_f, ax_f, m_f, e_c, x_f they select), row indices clamped to the number of
// rows: an index outside the array reads 0 and touches no memory (tfem_mg.hpp).  Offsets are
// 32-bit, the entry points refuse blocks of 4 GiB or more (check_extents).
#include <hip/hip_runtime.h>

#include "tfem_mg.hpp"

#pragma clang fp contract(off)

namespace tfem {

// ------------------------------------------------------------------------------------- smooth
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

// A block of total = n * n_vec values, n_vec >= 2, streamed flat.  VEC: x, b and ax are aligned to 16
// bytes; w has one entry per row and is read entry by entry.  A group of 2 doubles or 4 floats may
// lie across rows (an odd n_vec; n_vec = 2 or 3 with floats), so every value of the group takes the
// w of its own row: row(e0 + t) = row(e0) + [r >= n_vec] + [r >= 2 n_vec] with r = e0 mod n_vec + t
// <= n_vec + 2, one division per lane.
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
struct MgRestrictArgs {
  const int32_t *ptr, *idx;
  const T *mask_c, *mask_f, *b_f, *ax_f;
  T *r_c;
  unsigned n_c, n_f, n_vec;
};

// b_f, ax_f and r_c aligned to the access width of the row shape.
template <typename T, typename Kind, int NV>
__global__ __launch_bounds__(kMgBlock) void k_mg_restrict(const MgRestrictArgs<T> a) {
  using S = MgRowShape<T, NV>;
  using V = mg_vec<T, S::kE>;
  static_assert(S::kAccesses <= kMgRowLanes, "one access per lane of the row's group");
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * Kind::table_rows(a.n_c, a.n_f) * 4u);
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
  // every lane of the group holds every sum: lane `sub` finishes and stores access `sub` of the row
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
    if constexpr (Kind::kOwn) {  // the row's own residual: row < n_c <= n_f
      T bv[S::kE], av[S::kE];
      mg_load_chunk<T, S::kE>(r_b, row * S::kRowBytes + sub * S::kAccessBytes, bv);
      mg_load_chunk<T, S::kE>(r_ax, row * S::kRowBytes + sub * S::kAccessBytes, av);
      const T m = masked_f ? mg_load<T>(r_mf, row) : T(1);
#pragma unroll
      for (int e = 0; e < S::kE; ++e) {
        T own = bv[e] - av[e];
        if (masked_f) own = m * own;
        out[e] = own + out[e];
      }
    }
    if (a.mask_c) {
      const T mc = a.mask_c[row];
#pragma unroll
      for (int e = 0; e < S::kE; ++e) out[e] = mc * out[e];
    }
    reinterpret_cast<V *>(a.r_c + size_t(row) * NV)[sub] = out;
  }
}

// Any width and alignment: columns c0 .. c0 + 8 per pass, one access per value.
template <typename T, typename Kind>
__global__ __launch_bounds__(kMgBlock) void k_mg_restrict_any(const MgRestrictArgs<T> a) {
  const unsigned block_bytes = a.n_f * a.n_vec * unsigned(sizeof(T));
  const ring_rsrc_t r_idx = ring_rsrc(a.idx, 2u * Kind::table_rows(a.n_c, a.n_f) * 4u);
  const ring_rsrc_t r_b = ring_rsrc(a.b_f, block_bytes);
  const ring_rsrc_t r_ax = ring_rsrc(a.ax_f, block_bytes);
  const ring_rsrc_t r_mf = ring_rsrc(a.mask_f, a.mask_f ? a.n_f * unsigned(sizeof(T)) : 0u);
  const bool masked_f = a.mask_f != nullptr;
  const unsigned gid = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  const unsigned row = gid / unsigned(kMgRowLanes);
  const unsigned sub = gid % unsigned(kMgRowLanes);
  unsigned start = 0, end = 0;
  T mc = T(1), m_own = T(1);
  if (row < a.n_c) {
    start = unsigned(a.ptr[row]) + sub;
    end = unsigned(a.ptr[row + 1]);
    if (a.mask_c) mc = a.mask_c[row];
    if constexpr (Kind::kOwn)
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
    if (row < a.n_c && sub < nc) {  // lane `sub` finishes and stores column c0 + sub
      T v = T(0.5) * mine;
      if constexpr (Kind::kOwn) {
        const unsigned at = row * a.n_vec + c0 + sub;  // row < n_c <= n_f: inside the fine blocks
        T own = mg_load<T>(r_b, at) - mg_load<T>(r_ax, at);
        if (masked_f) own = m_own * own;
        v = own + v;
      }
      if (a.mask_c) v = mc * v;
      a.r_c[size_t(row) * a.n_vec + c0 + sub] = v;
    }
  }
}

// ------------------------------------------------------------------------------------ prolong
// The two coarse rows of fine DoF i, clamped to n_c, and whether it is its own coarse row.
template <typename Kind>
__device__ __forceinline__ bool mg_coarse_rows(ring_rsrc_t r_table, unsigned i, unsigned n_c, unsigned &pa,
                                               unsigned &pb) {
  bool own = false;
  if constexpr (Kind::kOwn) own = i < n_c;
  pa = i, pb = i;  // its own coarse row
  if (!own) {
    const unsigned t = Kind::table_row(i, n_c);
    pa = min(__builtin_amdgcn_raw_buffer_load_b32(r_table, t * 8u, 0, 0), n_c);
    pb = min(__builtin_amdgcn_raw_buffer_load_b32(r_table, t * 8u + 4u, 0, 0), n_c);
  }
  return own;
}

// One lane per fine DoF; e_c and x_f aligned to the access width of the row shape.
template <typename T, typename Kind, int NV>
__global__ __launch_bounds__(kMgBlock) void k_mg_prolong(const int32_t *__restrict__ table,
                                                         const T *__restrict__ mask_f, const T *__restrict__ e_c,
                                                         T *__restrict__ x_f, unsigned n_c, unsigned n_f) {
  using S = MgRowShape<T, NV>;
  const ring_rsrc_t r_table = ring_rsrc(table, 2u * Kind::table_rows(n_c, n_f) * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_c * S::kRowBytes);
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * S::kRowBytes);
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  unsigned pa, pb;
  const bool own = mg_coarse_rows<Kind>(r_table, i, n_c, pa, pb);
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
      T v = own ? ea[e] : T(0.5) * (ea[e] + eb[e]);
      if (masked) v = m * v;
      xv[e] = xv[e] + v;
    }
    mg_store_chunk<T, S::kE>(r_x, i * S::kRowBytes + at, xv);
  }
}

// Any width and alignment: the columns of the row one by one.
template <typename T, typename Kind>
__global__ __launch_bounds__(kMgBlock) void k_mg_prolong_any(const int32_t *__restrict__ table,
                                                             const T *__restrict__ mask_f,
                                                             const T *__restrict__ e_c, T *__restrict__ x_f,
                                                             unsigned n_c, unsigned n_f, unsigned n_vec) {
  const ring_rsrc_t r_table = ring_rsrc(table, 2u * Kind::table_rows(n_c, n_f) * 4u);
  const ring_rsrc_t r_e = ring_rsrc(e_c, n_c * n_vec * unsigned(sizeof(T)));
  const ring_rsrc_t r_x = ring_rsrc(x_f, n_f * n_vec * unsigned(sizeof(T)));
  const unsigned i = blockIdx.x * unsigned(kMgBlock) + threadIdx.x;
  if (i >= n_f) return;
  unsigned pa, pb;
  const bool own = mg_coarse_rows<Kind>(r_table, i, n_c, pa, pb);
  const bool masked = mask_f != nullptr;
  const T m = masked ? mask_f[i] : T(1);
  for (unsigned c = 0; c < n_vec; ++c) {  // row n_c starts at the extent: 0 from there on
    const T ea = mg_load<T>(r_e, pa * n_vec + c), eb = mg_load<T>(r_e, pb * n_vec + c);
    T v = own ? ea : T(0.5) * (ea + eb);
    if (masked) v = m * v;
    mg_store<T>(r_x, i * n_vec + c, mg_load<T>(r_x, i * n_vec + c) + v);
  }
}

// ---------------------------------------------------------------------------------------- host
// One function per operation: the checks of its single and its block entry point, of both kinds.
// `name` is the entry point the messages speak of; a single entry point passes n_vec = 1.

static int mg_smooth(const char *name, void *x, const void *b, const void *ax, const void *w, int real_bytes,
                     int64_t n, int64_t n_vec, int first, void *stream) {
  int st = mg_sizes(name, real_bytes, n, 0, n_vec);
  if (st != TFEM_OK) return st;
  if (n == 0) return TFEM_OK;
  if (!x || !b || !w || (!first && !ax)) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t bytes = mg_block_bytes(n, n_vec, real_bytes);
  st = check_extents("multigrid kernels", &bytes, 1);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x, bytes, b, bytes) || mg_overlap(x, bytes, w, n * real_bytes) ||
      (!first && mg_overlap(x, bytes, ax, bytes)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x overlaps an input", name);
  const bool single = n_vec == 1;  // k_mg_smooth reads w in groups as well
  bool vec = true;
  for (const void *p : {static_cast<const void *>(x), b, first ? b : ax, single ? w : b})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) vec = false;
  const int per_lane = vec ? 16 / real_bytes : 1;
  const int64_t total = n * n_vec;
  const int64_t lanes = total / per_lane + (vec ? total % per_lane : 0);
  const dim3 grid(unsigned((lanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_MG_SMOOTH(T, VEC, FIRST)                                                                          \
  if (single)                                                                                                  \
    k_mg_smooth<T, VEC, FIRST><<<grid, block, 0, s>>>(static_cast<T *>(x), static_cast<const T *>(b),          \
                                                      static_cast<const T *>(ax), static_cast<const T *>(w),   \
                                                      unsigned(n));                                            \
  else                                                                                                         \
    k_mg_smooth_multi<T, VEC, FIRST><<<grid, block, 0, s>>>(static_cast<T *>(x), static_cast<const T *>(b),    \
                                                            static_cast<const T *>(ax),                        \
                                                            static_cast<const T *>(w), unsigned(total),        \
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

template <typename Kind>
static int mg_restrict(const char *name, const int32_t *ptr, const int32_t *idx, const void *mask_c,
                       const void *mask_f, const void *b_f, const void *ax_f, void *r_c, int real_bytes, int64_t n_c,
                       int64_t n_f, int64_t n_vec, void *stream) {
  int st = mg_sizes(name, real_bytes, n_c, n_f, n_vec);
  if (st != TFEM_OK) return st;
  if (Kind::kOwn && n_f < n_c)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: n_f < n_v (the level holds the vertex DoFs)", name);
  if (n_c == 0) return TFEM_OK;
  // with rows of their own, n_f >= n_c > 0: the fine blocks are read whatever the table holds
  if (!ptr || !r_c || (Kind::table_rows(n_c, n_f) > 0 && !idx) || (n_f > 0 && (!b_f || !ax_f)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = mg_count(n_c), f = mg_count(n_f);
  // coarse block, fine blocks, ptr, idx (two entries per row of the table), the eight lanes per
  // row, the masks (one entry per DoF)
  const int64_t bytes[7] = {mg_block_bytes(n_c, n_vec, real_bytes), mg_block_bytes(n_f, n_vec, real_bytes),
                            (c + 1) * 4, 2 * Kind::table_rows(c, f) * 4, c * kMgRowLanes, c * real_bytes,
                            f * real_bytes};
  st = check_extents("multigrid kernels", bytes, 7);
  if (st != TFEM_OK) return st;
  const struct {
    const void *p;
    int64_t bytes;
  } inputs[6] = {{ptr, bytes[2]}, {idx, bytes[3]}, {mask_c, bytes[5]}, {mask_f, bytes[6]}, {b_f, bytes[1]}, {ax_f, bytes[1]}};
  for (const auto &in : inputs)
    if (mg_overlap(r_c, bytes[0], in.p, in.bytes))
      return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: r_c overlaps an input", name);
  const dim3 grid(unsigned((n_c * kMgRowLanes + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  mg_dispatch(real_bytes, mg_row_width(n_vec, real_bytes, {b_f, ax_f, r_c}), [&](auto t, auto width) {
    using T = decltype(t);
    constexpr int NV = decltype(width)::value;
    const MgRestrictArgs<T> a{ptr, idx, static_cast<const T *>(mask_c), static_cast<const T *>(mask_f),
                              static_cast<const T *>(b_f), static_cast<const T *>(ax_f), static_cast<T *>(r_c),
                              unsigned(n_c), unsigned(n_f), unsigned(n_vec)};
    if constexpr (NV == 0)
      k_mg_restrict_any<T, Kind><<<grid, block, 0, s>>>(a);
    else
      k_mg_restrict<T, Kind, NV><<<grid, block, 0, s>>>(a);
  });
  return mg_launched(name);
}

template <typename Kind>
static int mg_prolong(const char *name, const int32_t *table, const void *mask_f, const void *e_c, void *x_f,
                      int real_bytes, int64_t n_c, int64_t n_f, int64_t n_vec, void *stream) {
  int st = mg_sizes(name, real_bytes, n_c, n_f, n_vec);
  if (st != TFEM_OK) return st;
  if (Kind::kOwn && n_f < n_c)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: n_f < n_v (the level holds the vertex DoFs)", name);
  // with rows of their own and no coarse space there is nothing to add (an edge needs two vertices)
  if (n_f == 0 || (Kind::kOwn && n_c == 0)) return TFEM_OK;
  if (!e_c || !x_f || (Kind::table_rows(n_c, n_f) > 0 && !table))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  const int64_t c = mg_count(n_c), f = mg_count(n_f);
  // fine block, coarse block, the table, the mask (one entry per DoF)
  const int64_t bytes[4] = {mg_block_bytes(n_f, n_vec, real_bytes), mg_block_bytes(n_c, n_vec, real_bytes),
                            2 * Kind::table_rows(c, f) * 4, f * real_bytes};
  st = check_extents("multigrid kernels", bytes, 4);
  if (st != TFEM_OK) return st;
  if (mg_overlap(x_f, bytes[0], e_c, bytes[1]) || mg_overlap(x_f, bytes[0], mask_f, bytes[3]) ||
      mg_overlap(x_f, bytes[0], table, bytes[2]))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x_f overlaps an input", name);
  const dim3 grid(unsigned((n_f + kMgBlock - 1) / kMgBlock)), block(kMgBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  mg_dispatch(real_bytes, mg_row_width(n_vec, real_bytes, {e_c, static_cast<const void *>(x_f)}),
              [&](auto t, auto width) {
                using T = decltype(t);
                constexpr int NV = decltype(width)::value;
                const T *m = static_cast<const T *>(mask_f), *e = static_cast<const T *>(e_c);
                T *xf = static_cast<T *>(x_f);
                if constexpr (NV == 0)
                  k_mg_prolong_any<T, Kind><<<grid, block, 0, s>>>(table, m, e, xf, unsigned(n_c), unsigned(n_f),
                                                                   unsigned(n_vec));
                else
                  k_mg_prolong<T, Kind, NV><<<grid, block, 0, s>>>(table, m, e, xf, unsigned(n_c), unsigned(n_f));
              });
  return mg_launched(name);
}

}  // namespace tfem

using namespace tfem;

extern "C" {

int tfem_mg_smooth(void *x, const void *b, const void *ax, const void *w, int real_bytes, int64_t n, int first,
                   void *stream) {
  return mg_smooth("tfem_mg_smooth", x, b, ax, w, real_bytes, n, 1, first, stream);
}

int tfem_mg_smooth_multi(void *x, const void *b, const void *ax, const void *w, int real_bytes, int64_t n,
                         int64_t n_vec, int first, void *stream) {
  const char *const name = mg_multi_name("tfem_mg_smooth_multi", "tfem_mg_smooth", real_bytes, n, 0, n_vec);
  return mg_smooth(name, x, b, ax, w, real_bytes, n, n_vec, first, stream);
}

int tfem_mg_restrict_residual(const int32_t *ptr, const int32_t *idx, const void *mask_c, const void *mask_f,
                              const void *b_f, const void *ax_f, void *r_c, int real_bytes, int64_t n_c,
                              int64_t n_f, void *stream) {
  return mg_restrict<MgRefine>("tfem_mg_restrict_residual", ptr, idx, mask_c, mask_f, b_f, ax_f, r_c, real_bytes, n_c,
                               n_f, 1, stream);
}

int tfem_mg_restrict_residual_multi(const int32_t *ptr, const int32_t *idx, const void *mask_c, const void *mask_f,
                                    const void *b_f, const void *ax_f, void *r_c, int real_bytes, int64_t n_c,
                                    int64_t n_f, int64_t n_vec, void *stream) {
  const char *const name =
      mg_multi_name("tfem_mg_restrict_residual_multi", "tfem_mg_restrict_residual", real_bytes, n_c, n_f, n_vec);
  return mg_restrict<MgRefine>(name, ptr, idx, mask_c, mask_f, b_f, ax_f, r_c, real_bytes, n_c, n_f, n_vec, stream);
}

int tfem_mg_prolong_add(const int32_t *parents, const void *mask_f, const void *e_c, void *x_f, int real_bytes,
                        int64_t n_f, int64_t n_c, void *stream) {
  return mg_prolong<MgRefine>("tfem_mg_prolong_add", parents, mask_f, e_c, x_f, real_bytes, n_c, n_f, 1, stream);
}

int tfem_mg_prolong_add_multi(const int32_t *parents, const void *mask_f, const void *e_c, void *x_f, int real_bytes,
                              int64_t n_f, int64_t n_c, int64_t n_vec, void *stream) {
  const char *const name =
      mg_multi_name("tfem_mg_prolong_add_multi", "tfem_mg_prolong_add", real_bytes, n_c, n_f, n_vec);
  return mg_prolong<MgRefine>(name, parents, mask_f, e_c, x_f, real_bytes, n_c, n_f, n_vec, stream);
}

int tfem_mg_p2_restrict_residual(const int32_t *ptr, const int32_t *idx, const void *mask_c, const void *mask_f,
                                 const void *b_f, const void *ax_f, void *r_c, int real_bytes, int64_t n_v,
                                 int64_t n_f, void *stream) {
  return mg_restrict<MgP2>("tfem_mg_p2_restrict_residual", ptr, idx, mask_c, mask_f, b_f, ax_f, r_c, real_bytes, n_v,
                           n_f, 1, stream);
}

int tfem_mg_p2_restrict_residual_multi(const int32_t *ptr, const int32_t *idx, const void *mask_c,
                                       const void *mask_f, const void *b_f, const void *ax_f, void *r_c,
                                       int real_bytes, int64_t n_v, int64_t n_f, int64_t n_vec, void *stream) {
  const char *const name = mg_multi_name("tfem_mg_p2_restrict_residual_multi", "tfem_mg_p2_restrict_residual",
                                         real_bytes, n_v, n_f, n_vec);
  return mg_restrict<MgP2>(name, ptr, idx, mask_c, mask_f, b_f, ax_f, r_c, real_bytes, n_v, n_f, n_vec, stream);
}

int tfem_mg_p2_prolong_add(const int32_t *edge_vertices, const void *mask_f, const void *e_c, void *x_f,
                           int real_bytes, int64_t n_v, int64_t n_f, void *stream) {
  return mg_prolong<MgP2>("tfem_mg_p2_prolong_add", edge_vertices, mask_f, e_c, x_f, real_bytes, n_v, n_f, 1, stream);
}

int tfem_mg_p2_prolong_add_multi(const int32_t *edge_vertices, const void *mask_f, const void *e_c, void *x_f,
                                 int real_bytes, int64_t n_v, int64_t n_f, int64_t n_vec, void *stream) {
  const char *const name =
      mg_multi_name("tfem_mg_p2_prolong_add_multi", "tfem_mg_p2_prolong_add", real_bytes, n_v, n_f, n_vec);
  return mg_prolong<MgP2>(name, edge_vertices, mask_f, e_c, x_f, real_bytes, n_v, n_f, n_vec, stream);
}

}  // extern "C"
