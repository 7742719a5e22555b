// What the multigrid kernels of tfem_mg.hip share: the launch shape, the transfer kinds, the
// bounds-checked accesses, the accesses to the rows of a row-major block, and the host checks of the
// entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>

#include "tfem_common.hpp"
#include "tfem_rowkit.hpp"

namespace tfem {

constexpr int kMgBlock = 256;  // lanes per workgroup
constexpr int kMgRowLanes = 8;  // lanes per row of P^T

template <typename T, int N>
using mg_vec = T __attribute__((ext_vector_type(N)));

// ------------------------------------------------------------------------------ transfer kinds
// A transfer between a fine space of n_f DoFs and a coarse space of n_c DoFs whose weights are all
// 0.5: P is a table of two coarse ids per row, P^T its transpose (ptr, idx).  The two kinds differ
// in the extent of the table, in the DoFs that are their own coarse row, and in the table row of a
// fine DoF; the kernels and the host checks ask the kind and share everything else.

// The red refinement of a P1 mesh: every fine vertex has a row of `parents` (a kept vertex names
// itself twice), so the table is all of P.
struct MgRefine {
  static constexpr bool kOwn = false;  // no DoF is its own coarse row
  template <typename I>
  __host__ __device__ static constexpr I table_rows(I, I n_f) {
    return n_f;
  }
  __device__ static unsigned table_row(unsigned i, unsigned) { return i; }
};

// The step from P1 to P2 on one mesh (n_c = n_v): the P2 DoFs are "vertices, then edges", a vertex
// DoF is its own coarse row with the weight 1, and edge DoF n_v + j has row j of `edge_vertices`.
struct MgP2 {
  static constexpr bool kOwn = true;  // fine DoF i < n_c is coarse row i
  template <typename I>
  __host__ __device__ static constexpr I table_rows(I n_c, I n_f) {
    return n_f - n_c;
  }
  __device__ static unsigned table_row(unsigned i, unsigned n_c) { return i - n_c; }
};

// ---------------------------------------------------------------------- bounds-checked accesses
// A gathered array is read through a buffer resource of its own extent.  A row index that comes from
// data is clamped to the number of rows first (min(j, rows)): the row behind the last one starts at
// the extent, so an index outside the array -- however large, the 32-bit product with the row size
// does not wrap -- reads 0 and touches no memory.

// The T at byte offset `byte` of an array behind a buffer resource; 0 outside it.
template <typename T>
__device__ __forceinline__ T mg_load_at(ring_rsrc_t r, unsigned byte) {
  if constexpr (sizeof(T) == 8) {
    // two dword loads: raw_buffer_load_b64 is miscompiled by this hipcc (tfem_tiles.hip)
    const ru32x2 v{__builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0),
                   __builtin_amdgcn_raw_buffer_load_b32(r, byte + 4u, 0, 0)};
    return __builtin_bit_cast(double, v);
  } else {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0));
  }
}

// Entry i of an array of T behind a buffer resource; 0 outside it.
template <typename T>
__device__ __forceinline__ T mg_load(ring_rsrc_t r, unsigned i) {
  return mg_load_at<T>(r, i * unsigned(sizeof(T)));
}

template <typename T>
__device__ __forceinline__ void mg_store(ring_rsrc_t r, unsigned i, T v) {
  if constexpr (sizeof(T) == 8)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, v), r, i * 8u, 0, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, i * 4u, 0, 0);
}

// ------------------------------------------------------------- rows of a row-major block

constexpr int kMgPass = 8;  // columns per pass of the generic restriction

// KE consecutive values from byte offset `byte` (a multiple of KE * sizeof(T)) of a block behind a
// buffer resource; 0 outside it.  16 bytes in one access; one value, or two floats, value by value.
template <typename T, int KE>
__device__ __forceinline__ void mg_load_chunk(ring_rsrc_t r, unsigned byte, T (&v)[KE]) {
  static_assert(KE * sizeof(T) == 16 || KE == 1 || (KE == 2 && sizeof(T) == 4), "16 bytes, one value or two floats");
  if constexpr (KE * sizeof(T) == 16) {
    const ru32x4 q = __builtin_amdgcn_raw_buffer_load_b128(r, byte, 0, 0);
    if constexpr (sizeof(T) == 8) {
      v[0] = __builtin_bit_cast(double, ru32x2{q.x, q.y});
      v[1] = __builtin_bit_cast(double, ru32x2{q.z, q.w});
    } else {
      // the words by value first: a bit_cast straight from a vector element reads element 0
      const unsigned q0 = q.x, q1 = q.y, q2 = q.z, q3 = q.w;
      v[0] = __builtin_bit_cast(float, q0);
      v[1] = __builtin_bit_cast(float, q1);
      v[2] = __builtin_bit_cast(float, q2);
      v[3] = __builtin_bit_cast(float, q3);
    }
  } else {  // dword loads: raw_buffer_load_b64 is miscompiled by this hipcc (tfem_tiles.hip)
#pragma unroll
    for (int e = 0; e < KE; ++e) v[e] = mg_load_at<T>(r, byte + unsigned(e * sizeof(T)));
  }
}

template <typename T, int KE>
__device__ __forceinline__ void mg_store_chunk(ring_rsrc_t r, unsigned byte, const T (&v)[KE]) {
  if constexpr (KE * sizeof(T) == 16) {
    ru32x4 q;
    if constexpr (sizeof(T) == 8) {
      const ru32x2 lo = __builtin_bit_cast(ru32x2, v[0]), hi = __builtin_bit_cast(ru32x2, v[1]);
      q = ru32x4{lo.x, lo.y, hi.x, hi.y};
    } else {
      q = ru32x4{__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]),
                 __builtin_bit_cast(unsigned, v[2]), __builtin_bit_cast(unsigned, v[3])};
    }
    __builtin_amdgcn_raw_buffer_store_b128(q, r, byte, 0, 0);
  } else if constexpr (KE * sizeof(T) == 8) {  // one double or two floats
    ru32x2 q;
    if constexpr (KE == 1)
      q = __builtin_bit_cast(ru32x2, v[0]);
    else
      q = ru32x2{__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1])};
    __builtin_amdgcn_raw_buffer_store_b64(q, r, byte, 0, 0);
  } else {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[0]), r, byte, 0, 0);
  }
}

// Row width NV in {1, 2, 4, 8}: kE values per access, kAccesses accesses per row (SpmmShape).  NV = 1
// is a single vector: one value per access.
template <typename T, int NV>
struct MgRowShape {
  static constexpr int kE = NV * int(sizeof(T)) >= 16 ? 16 / int(sizeof(T)) : NV;
  static constexpr int kAccesses = NV / kE;
  static constexpr unsigned kAccessBytes = unsigned(kE * sizeof(T));
  static constexpr unsigned kRowBytes = unsigned(NV * sizeof(T));
};

// The sum over the eight lanes of a row, the same bits in every one of them (x + y == y + x).
template <typename T>
__device__ __forceinline__ T mg_row_sum(T acc) {
  acc = acc + __shfl_xor(acc, 4, 64);
  acc = acc + __shfl_xor(acc, 2, 64);
  acc = acc + __shfl_xor(acc, 1, 64);
  return acc;
}

// ---------------------------------------------------------------------------------------- host

static inline bool mg_overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes) {
  if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + uintptr_t(b_bytes) && pb < pa + uintptr_t(a_bytes);
}

// A single entry point passes n_vec = 1.
static inline int mg_sizes(const char *name, int real_bytes, int64_t n_a, int64_t n_b, int64_t n_vec) {
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: real_bytes must be 4 or 8", name);
  if (n_a < 0 || n_b < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: negative size", name);
  if (n_vec < 1) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: n_vec must be at least 1", name);
  return TFEM_OK;
}

// The name a block entry point goes on under: with n_vec == 1 it IS the single entry point once its
// sizes are accepted, and every later refusal carries that name; its sizes are refused under its own.
static inline const char *mg_multi_name(const char *multi, const char *single, int real_bytes, int64_t n_a,
                                        int64_t n_b, int64_t n_vec) {
  return n_vec == 1 && mg_sizes(multi, real_bytes, n_a, n_b, n_vec) == TFEM_OK ? single : multi;
}

static inline int mg_launched(const char *name) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "%s launch: %s", name, hipGetErrorString(e));
  return TFEM_OK;
}

// the largest n an extent check can be asked about without overflowing its own arithmetic
constexpr int64_t kMgCountLimit = int64_t(1) << 40;

static inline int64_t mg_count(int64_t n) { return n < kMgCountLimit ? n : kMgCountLimit; }

// n * n_vec * real_bytes, or a value >= 4 GiB where that would overflow.
static inline int64_t mg_block_bytes(int64_t n, int64_t n_vec, int real_bytes) {
  const int64_t rows = mg_count(n), cols = mg_count(n_vec);
  if (rows == 0) return 0;
  if (cols > kMgCountLimit / rows) return kMgCountLimit * real_bytes;
  return rows * cols * real_bytes;
}

// The row shape of a transfer launch: 1 for a single vector; n_vec if it is 2, 4 or 8 and every
// block is aligned to the access width; else 0 (the instance for any width).
static inline int mg_row_width(int64_t n_vec, int real_bytes, std::initializer_list<const void *> blocks) {
  if (n_vec == 1) return 1;
  if (n_vec != 2 && n_vec != 4 && n_vec != 8) return 0;
  const uintptr_t width = uintptr_t(n_vec * real_bytes < 16 ? n_vec * real_bytes : 16);
  for (const void *p : blocks)
    if (reinterpret_cast<uintptr_t>(p) % width != 0) return 0;
  return int(n_vec);
}

// launch(T(), width) with T the type of real_bytes and width the integral constant of nv, 0 .. 8.
template <typename F>
static inline void mg_dispatch(int real_bytes, int nv, F &&launch) {
  const auto widths = [&](auto t) {
    switch (nv) {
      case 1: launch(t, std::integral_constant<int, 1>()); break;
      case 2: launch(t, std::integral_constant<int, 2>()); break;
      case 4: launch(t, std::integral_constant<int, 4>()); break;
      case 8: launch(t, std::integral_constant<int, 8>()); break;
      default: launch(t, std::integral_constant<int, 0>());
    }
  };
  if (real_bytes == 8)
    widths(double());
  else
    widths(float());
}

}  // namespace tfem

