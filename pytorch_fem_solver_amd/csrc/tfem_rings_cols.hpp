// Column staging of the block launches over a ring plan (k_p1_apply_rows_multi in
// tfem_rings_apply.hip, k_p1_coef_rows_multi in tfem_rings_coef_multi.hip): U and Y are
// (n_verts, n_vec) row-major, a pass of a launch takes NV consecutive columns of every row.
#pragma once

#include "tfem_rings_kernel.hpp"

namespace tfem {

template <typename T>
struct ApplyMultiArgs {
  const T *u;
  T *y;
  unsigned u_bytes, y_bytes;
  unsigned n_vec;  // row stride of u and y (reals)
  unsigned col0;   // first column of this pass
  unsigned n_col;  // columns of this pass, 1 .. NV (the last pass of a launch may be narrower)
};

// NV consecutive reals of one row.  All NV are fetched whatever n_col is: behind the pass's last
// column they are the head of the next row (or the zeros behind the array); those sums are formed
// and dropped.  Doubles by 16-byte loads at 8-byte alignment (as ring_load_fq).
template <typename T, int NV>
__device__ __forceinline__ void apply_load_cols(ring_rsrc_t r, unsigned byte, T (&v)[NV]) {
#pragma unroll
  for (int c = 0; c < NV; c += 2) {
    if constexpr (sizeof(T) == 8) {
      const ru32x4 x = __builtin_amdgcn_raw_buffer_load_b128(r, byte + unsigned(c) * 8u, 0, 0);
      v[c] = __builtin_bit_cast(double, ru32x2{x.x, x.y});
      v[c + 1] = __builtin_bit_cast(double, ru32x2{x.z, x.w});
    } else {
      v[c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte + unsigned(c) * 4u, 0, 0));
      v[c + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte + unsigned(c) * 4u + 4u, 0, 0));
    }
  }
}

// The first n_col of NV sums -> one row of Y (n_col is uniform: scalar branches).
template <typename T, int NV>
__device__ __forceinline__ void apply_store_cols(ring_rsrc_t r, unsigned byte, const T (&v)[NV], unsigned n_col) {
#pragma unroll
  for (int c = 0; c < NV; c += 2) {
    if constexpr (sizeof(T) == 8) {
      const ru32x2 x = __builtin_bit_cast(ru32x2, v[c]), y = __builtin_bit_cast(ru32x2, v[c + 1]);
      if (unsigned(c + 1) < n_col)
        __builtin_amdgcn_raw_buffer_store_b128(ru32x4{x.x, x.y, y.x, y.y}, r, byte + unsigned(c) * 8u, 0, 0);
      else if (unsigned(c) < n_col)
        __builtin_amdgcn_raw_buffer_store_b64(x, r, byte + unsigned(c) * 8u, 0, 0);
    } else {
      if (unsigned(c) < n_col)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[c]), r, byte + unsigned(c) * 4u, 0, 0);
      if (unsigned(c + 1) < n_col)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[c + 1]), r, byte + unsigned(c) * 4u + 4u, 0, 0);
    }
  }
}

}  // namespace tfem
