// What the P2 row launches share (tfem_p2rows.hip: the rows stored, tfem_p2apply.hip: the rows
// applied to a vector): the launch constants, the kernel arguments and the row of the element block.
#pragma once

#include <hip/hip_runtime.h>

#include "tfem_common.hpp"
#include "tfem_rowkit.hpp"

#pragma clang fp contract(fast)

namespace tfem {

constexpr int kP2Block = 256;
constexpr int kP2Waves = kP2Block / 64;
constexpr int kP2VertexRowMax = 22;  // 1 + 3 * 7
constexpr int kP2EdgeRowMax = 9;

template <typename T>
struct P2RowArgs {
  const T *coords;
  const unsigned char *plan;
  T *vals;
  unsigned coords_bytes, plan_bytes, vals_bytes;
  unsigned off_desc, off_rows, off_gid;
  int n_tiles;
  int lds_vert;
  int xcd_ranges;  // 1: every XCD works on one contiguous range of the tile list, 0: tile = workgroup
  // row 0 (vertex kinds) or row 3 (edge kind) of the constant maps, alpha / beta folded in
  T ca[6], cb[6], cd[6], cm[6];
};

// entries r[0..6) of one row of the element block in the frame whose edge vectors are e1, e2
template <typename T, bool MASS>
__device__ __forceinline__ void p2_block_row(const T (&ca)[6], const T (&cb)[6], const T (&cd)[6], const T (&cm)[6],
                                             T q1, T q2, T p, T cross, uint32_t flag, T (&r)[6]);

template <typename T, bool MASS>
__device__ __forceinline__ void p2_block_row(const P2RowArgs<T> &a, T q1, T q2, T p, T cross,
                                             uint32_t flag, T (&r)[6]) {
  p2_block_row<T, MASS>(a.ca, a.cb, a.cd, a.cm, q1, q2, p, cross, flag, r);
}

template <typename T, bool MASS>
__device__ __forceinline__ void p2_block_row(const T (&ca)[6], const T (&cb)[6], const T (&cd)[6], const T (&cm)[6],
                                             T q1, T q2, T p, T cross, uint32_t flag, T (&r)[6]) {
  // flag: 0 no triangle (all zero), 1 frame = (e1, e2) as given, 2 frame = (e2, e1)
  const T c = flag_weight<T>(T(1), flag) * fast_rcp<T>(flag ? cross : T(1));  // 1 / det or 0
  const T g11 = c * (flag == 2u ? q1 : q2);
  const T g12 = -(c * p);
  const T g22 = c * (flag == 2u ? q2 : q1);
  const T det = flag_weight<T>(T(1), flag) * cross;
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    T v = ca[m] * g11 + cb[m] * g12 + cd[m] * g22;
    if (MASS) v = v + cm[m] * det;
    r[m] = v;
  }
}

}  // namespace tfem
