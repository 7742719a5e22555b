// The vector part of the Jacobi-preconditioned CG loop (sparse.fused_conjugate_gradients): three
// streaming launches per iteration around the operator's apply, every scalar on the device.
//
//   start     : p = D^-1 r,                      partials of r.z and r.r  -> parity 1
//   dot       : partials of p.Ap
//   update    : alpha = r.z / p.Ap, x += alpha p, r -= alpha Ap, partials of r.z and r.r -> parity step & 1
//   direction : beta = r.z(new) / r.z(old), p = D^-1 r + beta p
//
// A reduction is never finished by the launch that starts it.  Every workgroup writes its own
// partial sum (double, also for float vectors) to the slot [workgroup][column] of a buffer in the
// caller's workspace, and every workgroup of a LATER launch sums the G slots of a column itself, in
// one fixed order (lane t takes slots t, t + 256, ...; butterfly over the wave; the four waves in
// order).  So there is no atomic, no fence, no counter of finished workgroups and no scalar that
// one workgroup writes while another reads it; all workgroups get the same bits, and two runs give
// the same bits, because G depends on n alone.  r.z and r.r have two buffers each, chosen by the
// parity of the step: update(t) reads r.z of parity (t - 1) & 1 and writes parity t & 1,
// direction(t) reads both and writes none -- no launch reads a buffer its own workgroups write.
//
// Vectors are n x n_vec ROW-major.  A lane owns whole rows: with n_vec in {1, 2, 4, 8} and 16-byte
// aligned arrays it moves 16 bytes at a time (one row, or the 2 / 4 rows that fill 16 bytes); any
// other width goes through passes over at most 8 columns with scalar accesses, inside the one
// launch.  Plain loads and stores: the vectors are meant to stay in cache from launch to launch.
#include <hip/hip_runtime.h>

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

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_cg_start(const T *__restrict__ r, const T *__restrict__ inv_diag,
                                                       T *__restrict__ p, CgDims d, double *__restrict__ ws) {
  using S = CgShape<T, NV>;
  constexpr int NC = S::kCols;
  __shared__ double lds[4 * 2 * NC];
  double *const out[2] = {cg_buffer(ws, d, 3), cg_buffer(ws, d, 4)};
  for (unsigned c0 = 0; c0 < d.n_vec; c0 += NC) {
    const unsigned nc = min(unsigned(NC), d.n_vec - c0);
    double acc[2 * NC];
#pragma unroll
    for (int i = 0; i < 2 * NC; ++i) acc[i] = 0.0;
    for (unsigned g = blockIdx.x * kCgBlock + threadIdx.x; g < d.n_groups; g += d.grid * kCgBlock) {
      T w[S::kRows], rv[S::kVals], pv[S::kVals];
      cg_load_diag<T, NV>(inv_diag, g, d, w);
      cg_load<T, NV>(r, g, d, c0, nc, rv);
      unsigned mask = 0;
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        const bool exists = unsigned(col) < nc && g * S::kRows + row < d.n;
        const bool held = w[row] == T(0);
        const T z = w[row] * rv[i];
        pv[i] = held ? T(0) : z;
        if (exists) mask |= 1u << i;
        if (exists && !held) {
          acc[col] += double(rv[i]) * double(z);
          acc[NC + col] += double(rv[i]) * double(rv[i]);
        }
      }
      cg_store<T, NV>(p, g, d, c0, mask, pv);
    }
    cg_write_partials<2, NC>(acc, lds, out, d, c0, nc);
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_cg_dot(const T *__restrict__ p, const T *__restrict__ ap,
                                                     const T *__restrict__ inv_diag, CgDims d,
                                                     double *__restrict__ ws) {
  using S = CgShape<T, NV>;
  constexpr int NC = S::kCols;
  __shared__ double lds[4 * NC];
  double *const out[1] = {cg_buffer(ws, d, 0)};
  for (unsigned c0 = 0; c0 < d.n_vec; c0 += NC) {
    const unsigned nc = min(unsigned(NC), d.n_vec - c0);
    double acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0;
    for (unsigned g = blockIdx.x * kCgBlock + threadIdx.x; g < d.n_groups; g += d.grid * kCgBlock) {
      T w[S::kRows], pv[S::kVals], av[S::kVals];
      cg_load_diag<T, NV>(inv_diag, g, d, w);
      cg_load<T, NV>(p, g, d, c0, nc, pv);
      cg_load<T, NV>(ap, g, d, c0, nc, av);
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        // a held row is skipped, not multiplied by 0: its Ap may be anything
        if (unsigned(col) < nc && w[row] != T(0)) acc[col] += double(pv[i]) * double(av[i]);
      }
    }
    cg_write_partials<1, NC>(acc, lds, out, d, c0, nc);
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_cg_update(T *__restrict__ x, T *__restrict__ r, const T *__restrict__ p,
                                                        const T *__restrict__ ap, const T *__restrict__ inv_diag,
                                                        const int *__restrict__ active, CgDims d, int parity,
                                                        double *__restrict__ ws) {
  using S = CgShape<T, NV>;
  constexpr int NC = S::kCols;
  __shared__ double lds[4 * 2 * NC];
  const double *const in[2] = {cg_buffer(ws, d, 0), cg_buffer(ws, d, 1 + 2 * (parity ^ 1))};
  double *const out[2] = {cg_buffer(ws, d, 1 + 2 * parity), cg_buffer(ws, d, 2 + 2 * parity)};
  for (unsigned c0 = 0; c0 < d.n_vec; c0 += NC) {
    const unsigned nc = min(unsigned(NC), d.n_vec - c0);
    const unsigned act = cg_columns<NC>(active, c0, nc);
    double s[2 * NC];
    cg_read_partials<2, NC>(s, lds, in, d, c0, nc);
    T alpha[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) alpha[k] = (act >> k & 1u) ? T(s[NC + k] / s[k]) : T(0);
    double acc[2 * NC];
#pragma unroll
    for (int i = 0; i < 2 * NC; ++i) acc[i] = 0.0;
    for (unsigned g = blockIdx.x * kCgBlock + threadIdx.x; g < d.n_groups; g += d.grid * kCgBlock) {
      T w[S::kRows], xv[S::kVals], rv[S::kVals], pv[S::kVals], av[S::kVals];
      cg_load_diag<T, NV>(inv_diag, g, d, w);
      cg_load<T, NV>(x, g, d, c0, nc, xv);
      cg_load<T, NV>(r, g, d, c0, nc, rv);
      cg_load<T, NV>(p, g, d, c0, nc, pv);
      cg_load<T, NV>(ap, g, d, c0, nc, av);
      unsigned mask = 0;
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        const bool free_row = w[row] != T(0);
        if (free_row && (act >> col & 1u)) {
          mask |= 1u << i;
          xv[i] = xv[i] + alpha[col] * pv[i];
          rv[i] = rv[i] - alpha[col] * av[i];
        }
        if (free_row && unsigned(col) < nc) {
          const T z = w[row] * rv[i];
          acc[col] += double(rv[i]) * double(z);
          acc[NC + col] += double(rv[i]) * double(rv[i]);
        }
      }
      cg_store<T, NV>(x, g, d, c0, mask, xv);
      cg_store<T, NV>(r, g, d, c0, mask, rv);
    }
    cg_write_partials<2, NC>(acc, lds, out, d, c0, nc);
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_cg_direction(T *__restrict__ p, const T *__restrict__ r,
                                                           const T *__restrict__ inv_diag,
                                                           const int *__restrict__ active, CgDims d, int parity,
                                                           const double *__restrict__ ws) {
  using S = CgShape<T, NV>;
  constexpr int NC = S::kCols;
  __shared__ double lds[4 * 2 * NC];
  double *base = const_cast<double *>(ws);
  const double *const in[2] = {cg_buffer(base, d, 1 + 2 * parity), cg_buffer(base, d, 1 + 2 * (parity ^ 1))};
  for (unsigned c0 = 0; c0 < d.n_vec; c0 += NC) {
    const unsigned nc = min(unsigned(NC), d.n_vec - c0);
    const unsigned act = cg_columns<NC>(active, c0, nc);
    if (act == 0) continue;  // uniform: nothing of this pass is written
    double s[2 * NC];
    cg_read_partials<2, NC>(s, lds, in, d, c0, nc);
    T beta[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) beta[k] = (act >> k & 1u) ? T(s[k] / s[NC + k]) : T(0);
    for (unsigned g = blockIdx.x * kCgBlock + threadIdx.x; g < d.n_groups; g += d.grid * kCgBlock) {
      T w[S::kRows], rv[S::kVals], pv[S::kVals];
      cg_load_diag<T, NV>(inv_diag, g, d, w);
      cg_load<T, NV>(r, g, d, c0, nc, rv);
      cg_load<T, NV>(p, g, d, c0, nc, pv);
      unsigned mask = 0;
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        if (w[row] != T(0) && (act >> col & 1u)) {
          mask |= 1u << i;
          pv[i] = w[row] * rv[i] + beta[col] * pv[i];
        }
      }
      cg_store<T, NV>(p, g, d, c0, mask, pv);
    }
  }
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

// The checks shared by the four launches.  *go: something is to be launched.
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

extern "C" {

int tfem_cg_constant(int what) {
  return what == 0 ? tfem::kCgBlock : what == 1 ? tfem::kCgMaxGrid : what == 2 ? tfem::kCgPass : -1;
}

int tfem_cg_workspace_bytes(int64_t n, int64_t n_vec) {
  if (n < 0 || n_vec < 0) return -1;
  // vectors the launches refuse (2^30 entries or more) have no workspace either; below that
  // grid * n_vec <= 2^22 + n_vec and the size fits an int
  if (n_vec >= (int64_t(1) << 30) || (n > 0 && n_vec > (int64_t(1) << 30) / n)) return -1;
  const int64_t bytes = 5 * tfem::cg_grid(n) * n_vec * int64_t(sizeof(double));
  return bytes > int64_t(0x7fffffff) ? -1 : int(bytes);
}

int tfem_cg_start(const void *r, const void *inv_diag, void *p, int real_bytes, int64_t n, int64_t n_vec, void *ws,
                  void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_cg_start", real_bytes, n, n_vec, {r, inv_diag, p, ws}, &go);
  if (!go) return st;
  const int nv = cg_instance(n_vec, {r, inv_diag, p});
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                              \
  {                                                                                                      \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                           \
    k_cg_start<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(static_cast<const T *>(r),                 \
                                                             static_cast<const T *>(inv_diag),           \
                                                             static_cast<T *>(p), d, static_cast<double *>(ws)); \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_cg_start");
}

int tfem_cg_dot(const void *p, const void *ap, const void *inv_diag, int real_bytes, int64_t n, int64_t n_vec,
                void *ws, void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_cg_dot", real_bytes, n, n_vec, {p, ap, inv_diag, ws}, &go);
  if (!go) return st;
  const int nv = cg_instance(n_vec, {p, ap, inv_diag});
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                                      \
  {                                                                                                              \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                                   \
    k_cg_dot<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(static_cast<const T *>(p), static_cast<const T *>(ap), \
                                                           static_cast<const T *>(inv_diag), d,                  \
                                                           static_cast<double *>(ws));                           \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_cg_dot");
}

int tfem_cg_update(void *x, void *r, const void *p, const void *ap, const void *inv_diag, const int32_t *active,
                   int real_bytes, int64_t n, int64_t n_vec, int64_t step, void *ws, void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_cg_update", real_bytes, n, n_vec, {x, r, p, ap, inv_diag, active, ws}, &go);
  if (!go) return st;
  if (step < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "tfem_cg_update: negative step");
  const int nv = cg_instance(n_vec, {x, r, p, ap, inv_diag});
  const int parity = int(step & 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                                  \
  {                                                                                                          \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                               \
    k_cg_update<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(                                              \
        static_cast<T *>(x), static_cast<T *>(r), static_cast<const T *>(p), static_cast<const T *>(ap),     \
        static_cast<const T *>(inv_diag), active, d, parity, static_cast<double *>(ws));                     \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_cg_update");
}

int tfem_cg_direction(void *p, const void *r, const void *inv_diag, const int32_t *active, int real_bytes, int64_t n,
                      int64_t n_vec, int64_t step, const void *ws, void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_cg_direction", real_bytes, n, n_vec, {p, r, inv_diag, active, ws}, &go);
  if (!go) return st;
  if (step < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "tfem_cg_direction: negative step");
  const int nv = cg_instance(n_vec, {p, r, inv_diag});
  const int parity = int(step & 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                            \
  {                                                                                                    \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                         \
    k_cg_direction<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(                                     \
        static_cast<T *>(p), static_cast<const T *>(r), static_cast<const T *>(inv_diag), active, d,   \
        parity, static_cast<const double *>(ws));                                                      \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_cg_direction");
}

}  // extern "C"
