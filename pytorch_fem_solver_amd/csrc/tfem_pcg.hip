// The vector part of a CG loop whose preconditioner hands z = M^-1 r over as a VECTOR (the V-cycle
// of multigrid.py): four streaming launches per iteration around the operator's apply and the
// preconditioner, every scalar on the device.
//
//   start     : p = z,                            partials of r.z -> parity 1
//   dot       : partials of p.Ap                  (tfem_cg_dot of csrc/tfem_cg.hip, the mask as inv_diag)
//   update    : alpha = r.z / p.Ap, x += alpha p, r -= alpha Ap, partials of r.r -> parity step & 1
//     ... the preconditioner turns r into z ...
//   rz        : partials of r.z -> parity step & 1
//   direction : beta = r.z(new) / r.z(old), p = z + beta p
//
// The layout of the vectors, the width instances, the workspace and the reductions are those of
// csrc/tfem_cg.hpp: a reduction is never finished by the launch that starts it, every later
// workgroup sums the G partials in the one fixed order, no atomic, no fence, the same bits from run
// to run.  update(t) reads r.z of parity (t - 1) & 1 and writes r.r of parity t & 1, rz(t) writes
// r.z of parity t & 1, direction(t) reads both r.z and writes none -- no launch reads a buffer its
// own workgroups write.
//
// `mask` (n values of T) stands where inv_diag stands in tfem_cg.hip: mask[i] == 0 marks a held
// row, which is skipped (never multiplied by 0: its ap or z may be NaN).
#include "tfem_cg.hpp"

namespace tfem {

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_pcg_start(const T *__restrict__ r, const T *__restrict__ z,
                                                        const T *__restrict__ mask, T *__restrict__ p, CgDims d,
                                                        double *__restrict__ ws) {
  using S = CgShape<T, NV>;
  constexpr int NC = S::kCols;
  __shared__ double lds[4 * NC];
  double *const out[1] = {cg_buffer(ws, d, 3)};
  for (unsigned c0 = 0; c0 < d.n_vec; c0 += NC) {
    const unsigned nc = min(unsigned(NC), d.n_vec - c0);
    double acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0;
    for (unsigned g = blockIdx.x * kCgBlock + threadIdx.x; g < d.n_groups; g += d.grid * kCgBlock) {
      T w[S::kRows], rv[S::kVals], zv[S::kVals], pv[S::kVals];
      cg_load_diag<T, NV>(mask, g, d, w);
      cg_load<T, NV>(r, g, d, c0, nc, rv);
      cg_load<T, NV>(z, g, d, c0, nc, zv);
      unsigned bits = 0;
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        const bool exists = unsigned(col) < nc && g * S::kRows + row < d.n;
        const bool held = w[row] == T(0);
        pv[i] = held ? T(0) : zv[i];
        if (exists) bits |= 1u << i;
        if (exists && !held) acc[col] += double(rv[i]) * double(zv[i]);
      }
      cg_store<T, NV>(p, g, d, c0, bits, pv);
    }
    cg_write_partials<1, NC>(acc, lds, out, d, c0, nc);
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_pcg_update(T *__restrict__ x, T *__restrict__ r, const T *__restrict__ p,
                                                         const T *__restrict__ ap, const T *__restrict__ mask,
                                                         const int *__restrict__ active, CgDims d, int parity,
                                                         double *__restrict__ ws) {
  using S = CgShape<T, NV>;
  constexpr int NC = S::kCols;
  __shared__ double lds[4 * 2 * NC];
  const double *const in[2] = {cg_buffer(ws, d, 0), cg_buffer(ws, d, 1 + 2 * (parity ^ 1))};
  double *const out[1] = {cg_buffer(ws, d, 2 + 2 * parity)};
  for (unsigned c0 = 0; c0 < d.n_vec; c0 += NC) {
    const unsigned nc = min(unsigned(NC), d.n_vec - c0);
    const unsigned act = cg_columns<NC>(active, c0, nc);
    double s[2 * NC];
    cg_read_partials<2, NC>(s, lds, in, d, c0, nc);
    T alpha[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) alpha[k] = (act >> k & 1u) ? T(s[NC + k] / s[k]) : T(0);
    double acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0;
    for (unsigned g = blockIdx.x * kCgBlock + threadIdx.x; g < d.n_groups; g += d.grid * kCgBlock) {
      T w[S::kRows], xv[S::kVals], rv[S::kVals], pv[S::kVals], av[S::kVals];
      cg_load_diag<T, NV>(mask, g, d, w);
      cg_load<T, NV>(x, g, d, c0, nc, xv);
      cg_load<T, NV>(r, g, d, c0, nc, rv);
      cg_load<T, NV>(p, g, d, c0, nc, pv);
      cg_load<T, NV>(ap, g, d, c0, nc, av);
      unsigned bits = 0;
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        const bool free_row = w[row] != T(0);
        if (free_row && (act >> col & 1u)) {
          bits |= 1u << i;
          xv[i] = xv[i] + alpha[col] * pv[i];
          rv[i] = rv[i] - alpha[col] * av[i];
        }
        // every existing column, the frozen ones included: the host reads |r|^2 of all of them
        if (free_row && unsigned(col) < nc) acc[col] += double(rv[i]) * double(rv[i]);
      }
      cg_store<T, NV>(x, g, d, c0, bits, xv);
      cg_store<T, NV>(r, g, d, c0, bits, rv);
    }
    cg_write_partials<1, NC>(acc, lds, out, d, c0, nc);
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_pcg_rz(const T *__restrict__ r, const T *__restrict__ z,
                                                     const T *__restrict__ mask, CgDims d, int parity,
                                                     double *__restrict__ ws) {
  using S = CgShape<T, NV>;
  constexpr int NC = S::kCols;
  __shared__ double lds[4 * NC];
  double *const out[1] = {cg_buffer(ws, d, 1 + 2 * parity)};
  for (unsigned c0 = 0; c0 < d.n_vec; c0 += NC) {
    const unsigned nc = min(unsigned(NC), d.n_vec - c0);
    double acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0;
    for (unsigned g = blockIdx.x * kCgBlock + threadIdx.x; g < d.n_groups; g += d.grid * kCgBlock) {
      T w[S::kRows], rv[S::kVals], zv[S::kVals];
      cg_load_diag<T, NV>(mask, g, d, w);
      cg_load<T, NV>(r, g, d, c0, nc, rv);
      cg_load<T, NV>(z, g, d, c0, nc, zv);
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        // a held row is skipped, not multiplied by 0: its z may be anything
        if (unsigned(col) < nc && w[row] != T(0)) acc[col] += double(rv[i]) * double(zv[i]);
      }
    }
    cg_write_partials<1, NC>(acc, lds, out, d, c0, nc);
  }
}

template <typename T, int NV>
__global__ __launch_bounds__(kCgBlock) void k_pcg_direction(T *__restrict__ p, const T *__restrict__ z,
                                                            const T *__restrict__ mask,
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
      T w[S::kRows], zv[S::kVals], pv[S::kVals];
      cg_load_diag<T, NV>(mask, g, d, w);
      cg_load<T, NV>(z, g, d, c0, nc, zv);
      cg_load<T, NV>(p, g, d, c0, nc, pv);
      unsigned bits = 0;
#pragma unroll
      for (int i = 0; i < S::kVals; ++i) {
        const int row = i / NC, col = i % NC;
        if (w[row] != T(0) && (act >> col & 1u)) {
          bits |= 1u << i;
          pv[i] = zv[i] + beta[col] * pv[i];
        }
      }
      cg_store<T, NV>(p, g, d, c0, bits, pv);
    }
  }
}

}  // namespace tfem

extern "C" {

int tfem_pcg_start(const void *r, const void *z, const void *mask, void *p, int real_bytes, int64_t n, int64_t n_vec,
                   void *ws, void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_pcg_start", real_bytes, n, n_vec, {r, z, mask, p, ws}, &go);
  if (!go) return st;
  const int nv = cg_instance(n_vec, {r, z, mask, p});
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                                   \
  {                                                                                                           \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                                \
    k_pcg_start<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(static_cast<const T *>(r),                     \
                                                              static_cast<const T *>(z),                      \
                                                              static_cast<const T *>(mask), static_cast<T *>(p), \
                                                              d, static_cast<double *>(ws));                  \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_pcg_start");
}

int tfem_pcg_update(void *x, void *r, const void *p, const void *ap, const void *mask, const int32_t *active,
                    int real_bytes, int64_t n, int64_t n_vec, int64_t step, void *ws, void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_pcg_update", real_bytes, n, n_vec, {x, r, p, ap, mask, active, ws}, &go);
  if (!go) return st;
  if (step < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "tfem_pcg_update: negative step");
  const int nv = cg_instance(n_vec, {x, r, p, ap, mask});
  const int parity = int(step & 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                              \
  {                                                                                                      \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                           \
    k_pcg_update<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(                                         \
        static_cast<T *>(x), static_cast<T *>(r), static_cast<const T *>(p), static_cast<const T *>(ap), \
        static_cast<const T *>(mask), active, d, parity, static_cast<double *>(ws));                     \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_pcg_update");
}

int tfem_pcg_rz(const void *r, const void *z, const void *mask, int real_bytes, int64_t n, int64_t n_vec, int64_t step,
                void *ws, void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_pcg_rz", real_bytes, n, n_vec, {r, z, mask, ws}, &go);
  if (!go) return st;
  if (step < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "tfem_pcg_rz: negative step");
  const int nv = cg_instance(n_vec, {r, z, mask});
  const int parity = int(step & 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                                      \
  {                                                                                                              \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                                   \
    k_pcg_rz<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(static_cast<const T *>(r), static_cast<const T *>(z), \
                                                           static_cast<const T *>(mask), d, parity,              \
                                                           static_cast<double *>(ws));                           \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_pcg_rz");
}

int tfem_pcg_direction(void *p, const void *z, const void *mask, const int32_t *active, int real_bytes, int64_t n,
                       int64_t n_vec, int64_t step, const void *ws, void *stream) {
  using namespace tfem;
  bool go;
  const int st = cg_check("tfem_pcg_direction", real_bytes, n, n_vec, {p, z, mask, active, ws}, &go);
  if (!go) return st;
  if (step < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "tfem_pcg_direction: negative step");
  const int nv = cg_instance(n_vec, {p, z, mask});
  const int parity = int(step & 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define TFEM_CG_CALL(T, NV)                                                                      \
  {                                                                                              \
    const CgDims d = cg_dims(n, n_vec, CgShape<T, NV>::kRows);                                   \
    k_pcg_direction<T, NV><<<dim3(d.grid), dim3(kCgBlock), 0, s>>>(                              \
        static_cast<T *>(p), static_cast<const T *>(z), static_cast<const T *>(mask), active, d, \
        parity, static_cast<const double *>(ws));                                                \
  }
  TFEM_CG_DISPATCH(TFEM_CG_CALL)
#undef TFEM_CG_CALL
  return cg_launched("tfem_pcg_direction");
}

}  // extern "C"
