// What the multigrid kernels of tfem_mg.hip (one vector) and tfem_mg_multi.hip (a row-major block
// of vectors) share: the launch shape, the bounds-checked accesses, and the host checks of the entry
// points.
#pragma once

#include <hip/hip_runtime.h>

#include "tfem_common.hpp"
#include "tfem_rowkit.hpp"

namespace tfem {

constexpr int kMgBlock = 256;  // lanes per workgroup
constexpr int kMgRowLanes = 8;  // lanes per row of P^T

template <typename T, int N>
using mg_vec = T __attribute__((ext_vector_type(N)));

// Entry i of an array of T behind a buffer resource; 0 outside it.
template <typename T>
__device__ __forceinline__ T mg_load(ring_rsrc_t r, unsigned i) {
  if constexpr (sizeof(T) == 8) {
    // two dword loads: raw_buffer_load_b64 is miscompiled by this hipcc (tfem_tiles.hip)
    const ru32x2 v{__builtin_amdgcn_raw_buffer_load_b32(r, i * 8u, 0, 0),
                   __builtin_amdgcn_raw_buffer_load_b32(r, i * 8u + 4u, 0, 0)};
    return __builtin_bit_cast(double, v);
  } else {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, i * 4u, 0, 0));
  }
}

template <typename T>
__device__ __forceinline__ void mg_store(ring_rsrc_t r, unsigned i, T v) {
  if constexpr (sizeof(T) == 8)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, v), r, i * 8u, 0, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, i * 4u, 0, 0);
}

// ---------------------------------------------------------------------------------------- host

static inline bool mg_overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes) {
  if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + uintptr_t(b_bytes) && pb < pa + uintptr_t(a_bytes);
}

static inline int mg_sizes(const char *name, int real_bytes, int64_t n_a, int64_t n_b) {
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: real_bytes must be 4 or 8", name);
  if (n_a < 0 || n_b < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: negative size", name);
  return TFEM_OK;
}

static inline int mg_launched(const char *name) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "%s launch: %s", name, hipGetErrorString(e));
  return TFEM_OK;
}

// the largest n an extent check can be asked about without overflowing its own arithmetic
constexpr int64_t kMgCountLimit = int64_t(1) << 40;

}  // namespace tfem
