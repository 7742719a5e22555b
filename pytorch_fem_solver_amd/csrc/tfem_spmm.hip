// Y = A X for the assembled CSR operator and a block of n_vec vectors (tfem_csr_spmm): the block
// form of k_csr_spmv (tfem_kernels.hip), one launch for any n_vec.
//
// X is n_cols x n_vec and Y n_rows x n_vec, ROW-major (the layout of tfem_cg.hip and of the
// matrix-free block applies).  Eight lanes per row, as in k_csr_spmv: lane `sub` of a row's group
// takes the entries start + sub, start + sub + 8, ... in order, reads vals[p] and colind[p] ONCE and
// then the n_vec consecutive values of row colind[p] of X; the butterfly over 4, 2, 1 sums the eight
// partial sums of every column.  Per column this is the arithmetic of k_csr_spmv on that column, in
// the same order with the same roundings (a product and a sum, never an fma), so column c of Y is
// bit for bit what tfem_csr_spmv gives for the contiguous copy of column c, whatever n_vec is.
//
// n_vec in {2, 4, 8} with X and Y aligned to the access width min(16, n_vec * sizeof(T)) bytes: a
// row of X is read and a row of Y written in accesses of that width.  After the butterfly every
// lane of the group holds every sum, so lane `sub` stores access `sub` of the row: one store
// instruction per row.  Any other width, and any other alignment: passes over at most 8 columns
// with scalar accesses inside the one launch; lane `sub` stores column c0 + sub.  Plain loads and
// stores: the vectors are meant to stay in cache between the launches of a CG iteration.
#include <hip/hip_runtime.h>

#include "tfem_common.hpp"

// a product and a sum per entry, as in k_csr_spmv: the bits of the two kernels must agree
#pragma clang fp contract(off)

namespace tfem {

constexpr int kSpmmBlock = 256;  // lanes per workgroup: 32 rows
constexpr int kSpmmPass = 8;     // columns per pass of the generic instance

template <typename T, int N>
using spmm_vec = T __attribute__((ext_vector_type(N)));

// Row width NV: kE values per access, kAccesses accesses per row.
template <typename T, int NV>
struct SpmmShape {
  static constexpr int kE = NV * int(sizeof(T)) >= 16 ? 16 / int(sizeof(T)) : NV;
  static constexpr int kAccesses = NV / kE;
  static constexpr int kBytes = kE * int(sizeof(T));
};

// The sum over the eight lanes of a row, the same bits in every one of them (x + y == y + x): the
// steps of k_csr_spmv.
template <typename T>
__device__ __forceinline__ T spmm_row_sum(T acc) {
  acc = acc + __shfl_xor(acc, 4, 64);
  acc = acc + __shfl_xor(acc, 2, 64);
  acc = acc + __shfl_xor(acc, 1, 64);
  return acc;
}

template <typename T, int NV>
__global__ __launch_bounds__(kSpmmBlock) void k_csr_spmm(const int64_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ colind,
                                                         const T *__restrict__ vals, const T *__restrict__ x,
                                                         T *__restrict__ y, int64_t n_rows) {
  using S = SpmmShape<T, NV>;
  using V = spmm_vec<T, S::kE>;
  static_assert(S::kAccesses <= 8, "one access per lane of the row's group");
  const int64_t gid = int64_t(blockIdx.x) * kSpmmBlock + threadIdx.x;
  const int64_t row = gid >> 3;
  const int sub = int(gid & 7);
  T acc[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c] = T(0);
  if (row < n_rows) {
    const int64_t end = rowptr[row + 1];
    for (int64_t p = rowptr[row] + sub; p < end; p += 8) {
      const T v = vals[p];
      const V *xr = reinterpret_cast<const V *>(x + int64_t(colind[p]) * NV);
#pragma unroll
      for (int l = 0; l < S::kAccesses; ++l) {
        const V w = xr[l];
#pragma unroll
        for (int e = 0; e < S::kE; ++e) acc[l * S::kE + e] = acc[l * S::kE + e] + v * w[e];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c] = spmm_row_sum(acc[c]);
  if (row < n_rows && sub < S::kAccesses) {
    V w;
#pragma unroll
    for (int e = 0; e < S::kE; ++e) w[e] = acc[e];
#pragma unroll
    for (int l = 1; l < S::kAccesses; ++l) {
#pragma unroll
      for (int e = 0; e < S::kE; ++e) w[e] = sub == l ? acc[l * S::kE + e] : w[e];
    }
    reinterpret_cast<V *>(y + row * NV)[sub] = w;
  }
}

// Any width and alignment: columns c0 .. c0 + 8 per pass.
template <typename T>
__global__ __launch_bounds__(kSpmmBlock) void k_csr_spmm_any(const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ colind,
                                                             const T *__restrict__ vals, const T *__restrict__ x,
                                                             T *__restrict__ y, int64_t n_rows, int n_vec) {
  const int64_t gid = int64_t(blockIdx.x) * kSpmmBlock + threadIdx.x;
  const int64_t row = gid >> 3;
  const int sub = int(gid & 7);
  int64_t start = 0, end = 0;
  if (row < n_rows) {
    start = rowptr[row] + sub;
    end = rowptr[row + 1];
  }
  for (int c0 = 0; c0 < n_vec; c0 += kSpmmPass) {
    const int nc = min(kSpmmPass, n_vec - c0);  // the same in every lane
    T acc[kSpmmPass];
#pragma unroll
    for (int c = 0; c < kSpmmPass; ++c) acc[c] = T(0);
    for (int64_t p = start; p < end; p += 8) {
      const T v = vals[p];
      const T *xr = x + int64_t(colind[p]) * n_vec + c0;
#pragma unroll
      for (int c = 0; c < kSpmmPass; ++c)
        if (c < nc) acc[c] = acc[c] + v * xr[c];
    }
    T mine = T(0);
#pragma unroll
    for (int c = 0; c < kSpmmPass; ++c) {
      const T sum = spmm_row_sum(acc[c]);
      mine = sub == c ? sum : mine;
    }
    if (row < n_rows && sub < nc) y[row * n_vec + c0 + sub] = mine;
  }
}

}  // namespace tfem

extern "C" int tfem_csr_spmm(const int64_t *rowptr, const int32_t *colind, const void *vals, int real_bytes,
                             int64_t n_rows, int64_t n_cols, int n_vec, const void *x, void *y, void *stream) {
  using namespace tfem;
  const char *const name = "tfem_csr_spmm";
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: real_bytes must be 4 or 8", name);
  if (n_rows < 0 || n_cols < 0 || n_vec < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: negative size", name);
  if (n_rows == 0 || n_vec == 0) return TFEM_OK;
  if (!rowptr || !y || (n_cols > 0 && !x)) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", name);
  // 8 lanes per row in a 32-bit grid, and extents that can be compared as byte addresses
  const int64_t most = n_rows > n_cols ? n_rows : n_cols;
  if (n_rows >= (int64_t(1) << 36) || most > (int64_t(1) << 59) / n_vec)
    return fail(TFEM_ERR_INDEX_RANGE, "%s: %lld x %lld by %d vectors is beyond the launch's extent", name,
                (long long)n_rows, (long long)n_cols, n_vec);
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
  const uintptr_t xb = uintptr_t(n_cols) * uintptr_t(n_vec) * uintptr_t(real_bytes);
  const uintptr_t yb = uintptr_t(n_rows) * uintptr_t(n_vec) * uintptr_t(real_bytes);
  if (xa < ya + yb && ya < xa + xb) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: x and y overlap", name);
  // the width instance: both base pointers on the access width (the row stride is a multiple of it)
  int nv = 0;
  if (n_vec == 2 || n_vec == 4 || n_vec == 8) {
    const uintptr_t width = uintptr_t(n_vec * real_bytes < 16 ? n_vec * real_bytes : 16);
    if (xa % width == 0 && ya % width == 0) nv = n_vec;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned((8 * n_rows + kSpmmBlock - 1) / kSpmmBlock)), block(kSpmmBlock);
#define TFEM_SPMM_WIDTH(T, NV)                                                                                   \
  k_csr_spmm<T, NV><<<grid, block, 0, s>>>(rowptr, colind, static_cast<const T *>(vals), static_cast<const T *>(x), \
                                           static_cast<T *>(y), n_rows)
#define TFEM_SPMM_TYPE(T)                                                                                            \
  switch (nv) {                                                                                                      \
    case 2: TFEM_SPMM_WIDTH(T, 2); break;                                                                            \
    case 4: TFEM_SPMM_WIDTH(T, 4); break;                                                                            \
    case 8: TFEM_SPMM_WIDTH(T, 8); break;                                                                            \
    default:                                                                                                         \
      k_csr_spmm_any<T><<<grid, block, 0, s>>>(rowptr, colind, static_cast<const T *>(vals),                         \
                                               static_cast<const T *>(x), static_cast<T *>(y), n_rows, n_vec);       \
  }
  if (real_bytes == 8) {
    TFEM_SPMM_TYPE(double)
  } else {
    TFEM_SPMM_TYPE(float)
  }
#undef TFEM_SPMM_TYPE
#undef TFEM_SPMM_WIDTH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "%s launch: %s", name, hipGetErrorString(e));
  return TFEM_OK;
}
