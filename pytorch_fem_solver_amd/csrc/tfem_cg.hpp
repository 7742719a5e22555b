// What the fused CG loops share (csrc/tfem_cg.hip: the Jacobi-preconditioned loop with z = D^-1 r
// formed inline; csrc/tfem_pcg.hip: the loop around a preconditioner whose z arrives as a vector):
// the shape of a lane's group of rows, its loads and stores, the per-workgroup partial sums in the
// caller's workspace and their fixed-order read, the grid, the host checks and the width dispatch.
//
// A reduction is never finished by the launch that starts it.  Every workgroup writes its own
// partial sum (double, also for float vectors) to the slot [workgroup][column] of a buffer in the
// caller's workspace, and every workgroup of a LATER launch sums the G slots of a column itself, in
// one fixed order (lane t takes slots t, t + 256, ...; butterfly over the wave; the four waves in
// order).  So there is no atomic, no fence, no counter of finished workgroups and no scalar that
// one workgroup writes while another reads it; all workgroups get the same bits, and two runs give
// the same bits, because G depends on n alone.
//
// Vectors are n x n_vec ROW-major.  A lane owns whole rows: with n_vec in {1, 2, 4, 8} and 16-byte
// aligned arrays it moves 16 bytes at a time (one row, or the 2 / 4 rows that fill 16 bytes); any
// other width goes through passes over at most 8 columns with scalar accesses, inside the one
// launch.  Plain loads and stores: the vectors are meant to stay in cache from launch to launch.
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>

#include "tfem_common.hpp"

namespace tfem {

constexpr int kCgBlock = 256;     // lanes per workgroup (tfem_cg_constant(0))
constexpr int kCgMaxGrid = 1024;  // workgroups at most: 4 per CU of 256 (tfem_cg_constant(1))
constexpr int kCgPass = 8;        // columns per pass of the generic instance

// Workgroups of every launch for n rows: a function of n alone, never of the device's state.
static int64_t cg_grid(int64_t n) {
  const int64_t g = (n + kCgBlock - 1) / kCgBlock;
  return g < 1 ? 1 : (g > kCgMaxGrid ? kCgMaxGrid : g);
}

// NV > 0: the row width is NV, a lane's group is kRows rows = kVals values = kLoads 16-byte
// accesses.  NV == 0: one row per group, up to kCgPass of its columns per pass.
template <typename T, int NV>
struct CgShape {
  static constexpr int kE = 16 / int(sizeof(T));
  static constexpr int kRows = NV >= kE ? 1 : kE / NV;
  static constexpr int kCols = NV;
  static constexpr int kVals = kRows * NV;
  static constexpr int kLoads = kVals / kE;
};
template <typename T>
struct CgShape<T, 0> {
  static constexpr int kE = 1;
  static constexpr int kRows = 1;
  static constexpr int kCols = kCgPass;
  static constexpr int kVals = kCgPass;
  static constexpr int kLoads = 0;
};

template <typename T, int N>
using cg_vec = T __attribute__((ext_vector_type(N)));

// What every kernel knows about the vectors.  n_groups = ceil(n / kRows).
struct CgDims {
  unsigned n, n_vec, n_groups, grid;
};

// The values of group g of one vector (columns c0 .. c0 + nc of its row for NV == 0); 0 past the end.
template <typename T, int NV>
__device__ __forceinline__ void cg_load(const T *a, unsigned g, const CgDims &d, unsigned c0, unsigned nc,
                                        T (&v)[CgShape<T, NV>::kVals]) {
  using S = CgShape<T, NV>;
  if constexpr (NV > 0) {
    const T *base = a + size_t(g) * S::kVals;
    if ((g + 1) * S::kRows <= d.n) {
#pragma unroll
      for (int l = 0; l < S::kLoads; ++l) {
        const cg_vec<T, S::kE> w = reinterpret_cast<const cg_vec<T, S::kE> *>(base)[l];
#pragma unroll
        for (int e = 0; e < S::kE; ++e) v[l * S::kE + e] = w[e];
      }
    } else {
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) v[i] = (g * S::kRows + i / NV < d.n) ? base[i] : T(0);
    }
  } else {
    const T *base = a + size_t(g) * d.n_vec + c0;
#pragma unroll
    for (int i = 0; i < S::kVals; ++i) v[i] = unsigned(i) < nc ? base[i] : T(0);
  }
}

// Stores the values whose bit of `mask` is set, and no other: 16 bytes at a time where all of
// them are, one by one otherwise (held rows, inactive columns, the ragged last group).
template <typename T, int NV>
__device__ __forceinline__ void cg_store(T *a, unsigned g, const CgDims &d, unsigned c0, unsigned mask,
                                         const T (&v)[CgShape<T, NV>::kVals]) {
  using S = CgShape<T, NV>;
  if constexpr (NV > 0) {
    T *base = a + size_t(g) * S::kVals;
#pragma unroll
    for (int l = 0; l < S::kLoads; ++l) {
      const unsigned all = ((1u << S::kE) - 1u) << (l * S::kE);
      if ((mask & all) == all) {
        cg_vec<T, S::kE> w;
#pragma unroll
        for (int e = 0; e < S::kE; ++e) w[e] = v[l * S::kE + e];
        reinterpret_cast<cg_vec<T, S::kE> *>(base)[l] = w;
      } else {
#pragma unroll
        for (int e = 0; e < S::kE; ++e)
          if (mask >> (l * S::kE + e) & 1u) base[l * S::kE + e] = v[l * S::kE + e];
      }
    }
  } else {
    T *base = a + size_t(g) * d.n_vec + c0;
#pragma unroll
    for (int i = 0; i < S::kVals; ++i)
      if (mask >> i & 1u) base[i] = v[i];
  }
}

// inv_diag of the rows of group g, 0 past the end (a row past the end is a held row).
template <typename T, int NV>
__device__ __forceinline__ void cg_load_diag(const T *inv_diag, unsigned g, const CgDims &d,
                                             T (&w)[CgShape<T, NV>::kRows]) {
  using S = CgShape<T, NV>;
  if constexpr (S::kRows > 1) {
    if ((g + 1) * S::kRows <= d.n) {
      const cg_vec<T, S::kRows> q = reinterpret_cast<const cg_vec<T, S::kRows> *>(inv_diag)[g];
#pragma unroll
      for (int j = 0; j < S::kRows; ++j) w[j] = q[j];
    } else {
#pragma unroll
      for (int j = 0; j < S::kRows; ++j) w[j] = (g * S::kRows + j < d.n) ? inv_diag[g * S::kRows + j] : T(0);
    }
  } else {
    w[0] = inv_diag[g];
  }
}

// Bit k: column c0 + k exists and is active (active == nullptr: exists).
template <int NC>
__device__ __forceinline__ unsigned cg_columns(const int *active, unsigned c0, unsigned nc) {
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < NC; ++k)
    if (unsigned(k) < nc && (!active || active[c0 + k] != 0)) bits |= 1u << k;
  return bits;
}

// Sum of a[k] over the wave, the same bits in every lane (x + y == y + x, so both partners of a
// butterfly step hold the same value).
template <int NA>
__device__ __forceinline__ void cg_wave_sum(double (&a)[NA]) {
#pragma unroll
  for (int k = 0; k < NA; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a[k] += __shfl_xor(a[k], off, 64);
  }
}

// Sum over the workgroup, in every lane.  lds: 4 * NA doubles.
template <int NA>
__device__ __forceinline__ void cg_block_sum(double (&a)[NA], double *lds) {
  cg_wave_sum<NA>(a);
  __syncthreads();  // the previous use of lds is over
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int k = 0; k < NA; ++k) lds[(threadIdx.x >> 6) * NA + k] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NA; ++k) a[k] = ((lds[k] + lds[NA + k]) + lds[2 * NA + k]) + lds[3 * NA + k];
}

// The workgroup's partial sums of NQ quantities x NC columns (a[q * NC + k]) to slot
// [workgroup][c0 + k] of the NQ buffers out[q].
template <int NQ, int NC>
__device__ __forceinline__ void cg_write_partials(double (&a)[NQ * NC], double *lds, double *const (&out)[NQ],
                                                  const CgDims &d, unsigned c0, unsigned nc) {
  constexpr int NA = NQ * NC;
  cg_wave_sum<NA>(a);
  __syncthreads();
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int k = 0; k < NA; ++k) lds[(threadIdx.x >> 6) * NA + k] = a[k];
  }
  __syncthreads();
  const unsigned t = threadIdx.x;
  if (t < unsigned(NA) && t % NC < nc) {
    const double s = ((lds[t] + lds[NA + t]) + lds[2 * NA + t]) + lds[3 * NA + t];
    double *buf = out[0];
#pragma unroll
    for (int q = 1; q < NQ; ++q)
      if (t / NC == unsigned(q)) buf = out[q];
    buf[size_t(blockIdx.x) * d.n_vec + c0 + t % NC] = s;
  }
}

// s[q * NC + k] = sum over the d.grid slots of column c0 + k of buffer in[q]: the same order in
// every workgroup of every launch.
template <int NQ, int NC>
__device__ __forceinline__ void cg_read_partials(double (&s)[NQ * NC], double *lds, const double *const (&in)[NQ],
                                                 const CgDims &d, unsigned c0, unsigned nc) {
#pragma unroll
  for (int i = 0; i < NQ * NC; ++i) s[i] = 0.0;
  for (unsigned g = threadIdx.x; g < d.grid; g += kCgBlock) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (unsigned(k) < nc) s[q * NC + k] += in[q][size_t(g) * d.n_vec + c0 + k];
    }
  }
  cg_block_sum<NQ * NC>(s, lds);
}

// The buffers of the workspace: p.Ap, then (r.z, r.r) of parity 0, then of parity 1; each
// grid x n_vec doubles.
__device__ __forceinline__ double *cg_buffer(double *ws, const CgDims &d, int which) {
  return ws + size_t(which) * d.grid * d.n_vec;
}

// ---------------------------------------------------------------------------------------- host

// The width instance: n_vec itself for 1, 2, 4, 8 when every array can be moved 16 bytes at a
// time, the generic passes otherwise.
static int cg_instance(int64_t n_vec, std::initializer_list<const void *> arrays) {
  if (n_vec != 1 && n_vec != 2 && n_vec != 4 && n_vec != 8) return 0;
  for (const void *a : arrays)
    if (reinterpret_cast<uintptr_t>(a) % 16 != 0) return 0;
  return int(n_vec);
}

static CgDims cg_dims(int64_t n, int64_t n_vec, int rows_per_group) {
  CgDims d;
  d.n = unsigned(n);
  d.n_vec = unsigned(n_vec);
  d.n_groups = unsigned((n + rows_per_group - 1) / rows_per_group);
  d.grid = unsigned(cg_grid(n));
  return d;
}

// The checks shared by the launches.  *go: something is to be launched.
static int cg_check(const char *what, int real_bytes, int64_t n, int64_t n_vec,
                    std::initializer_list<const void *> arrays, bool *go) {
  *go = false;
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: real_bytes must be 4 or 8", what);
  if (n < 0 || n_vec < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: negative size", what);
  if (n == 0 || n_vec == 0) return TFEM_OK;
  for (const void *a : arrays)
    if (!a) return fail(TFEM_ERR_INVALID_ARGUMENT, "%s: NULL pointer", what);
  // the kernels count rows and entries in 32 bits
  const int64_t limit = (int64_t(1) << 32) / real_bytes;
  if (n >= limit || n_vec >= limit || n * n_vec >= limit)
    return fail(TFEM_ERR_INDEX_RANGE, "%s: a vector of %lld x %lld entries has 4 GiB or more", what, (long long)n,
                (long long)n_vec);
  *go = true;
  return TFEM_OK;
}

static int cg_launched(const char *what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
  return TFEM_OK;
}

#define TFEM_CG_WIDTHS(T, CALL) \
  switch (nv) {                 \
    case 1: CALL(T, 1); break;  \
    case 2: CALL(T, 2); break;  \
    case 4: CALL(T, 4); break;  \
    case 8: CALL(T, 8); break;  \
    default: CALL(T, 0); break; \
  }
#define TFEM_CG_DISPATCH(CALL)    \
  if (real_bytes == 8) {          \
    TFEM_CG_WIDTHS(double, CALL)  \
  } else {                        \
    TFEM_CG_WIDTHS(float, CALL)   \
  }

}  // namespace tfem
