// The vector part of the Jacobi-preconditioned CG loop (sparse.fused_conjugate_gradients): three
// streaming launches per iteration around the operator's apply, every scalar on the device.
//
//   start     : p = D^-1 r,                      partials of r.z and r.r  -> parity 1
//   dot       : partials of p.Ap
//   update    : alpha = r.z / p.Ap, x += alpha p, r -= alpha Ap, partials of r.z and r.r -> parity step & 1
//   direction : beta = r.z(new) / r.z(old), p = D^-1 r + beta p
//
// The layout of the vectors, the width instances and the reductions (per-workgroup partial sums in
// the caller's workspace, finished by every workgroup of a LATER launch in one fixed order: no
// atomic, no fence, the same bits from run to run) are those of csrc/tfem_cg.hpp, shared with the
// loop around a vector preconditioner (csrc/tfem_pcg.hip).  r.z and r.r have two buffers each,
// chosen by the parity of the step: update(t) reads r.z of parity (t - 1) & 1 and writes parity
// t & 1, direction(t) reads both and writes none -- no launch reads a buffer its own workgroups
// write.
#include "tfem_cg.hpp"

namespace tfem {

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
