// What the variable-coefficient launches over a ring plan share (tfem_rings_coef.hip: assembly, K u,
// diag K; tfem_rings_coef_multi.hip: K U): the launch arguments, the cursor over a row record and
// ring_row_coef, the row of K with kappa and c evaluated per triangle.  tfem_rings_coef.hip's header
// says what ring_row_coef computes and why it is shaped as it is.
#pragma once

#include "tfem_rings_kernel.hpp"

namespace tfem {

template <typename T>
struct CoefArgs {
  const T *u;
  T *y;
  unsigned u_bytes, y_bytes;
  int has_kappa, has_c;  // 0: that term keeps its constant (RingArgs::stiff_w, mass_d / mass_o)
  T alpha, beta;
  SrcProgram<T> kappa, c;
};

template <typename T>
struct CoefLaunch {  // the kernel's only parameter (src_in_kernarg addresses the programs in it)
  RingArgs<T> a;
  CoefArgs<T> b;
};

// The fields of a row record in fan order, one slot per pop (RingRec's bit layout).
template <int SLOTS>
struct RecCursor {
  static constexpr int kIdWords = SLOTS == 7 ? 3 : 5;
  uint32_t idw[kIdWords];
  uint32_t flags;
  unsigned long long pos;
  __device__ __forceinline__ explicit RecCursor(const RingRec<SLOTS> &rec) {
#pragma unroll
    for (int j = 0; j < kIdWords; ++j) idw[j] = rec.w[j] & 0x3FFFFFFFu;
    if constexpr (SLOTS == 7) {
      idw[2] &= 0x3FFu;
      flags = (rec.w[2] >> 10) & 0x3FFFu;
      pos = rec.w[3] & 0x1FFFFFu;
    } else {
      flags = rec.w[5] & 0x3FFFFFFFu;
      pos = (unsigned long long)rec.w[6] | ((unsigned long long)rec.w[7] << 32);
    }
  }
  __device__ __forceinline__ uint32_t id() const { return idw[0] & 0x3FFu; }
  __device__ __forceinline__ uint32_t flag() const { return flags & 3u; }
  __device__ __forceinline__ int at() const { return int(pos & (SLOTS == 7 ? 7u : 15u)); }
  __device__ __forceinline__ void next() {
#pragma unroll
    for (int j = 0; j + 1 < kIdWords; ++j) idw[j] = (idw[j] >> 10) | ((idw[j + 1] & 0x3FFu) << 20);
    idw[kIdWords - 1] >>= 10;
    flags >>= 2;
    pos >>= (SLOTS == 7 ? 3 : 4);
  }
};

// The row of local vertex `lv` with coefficients: emit(live, id, pos, value) is called once per slot
// 1 .. kmax - 1 inside the loop and once for slot 0 behind it (live: the slot is one of the row's
// k neighbours; id its tile-local vertex, pos its position in the row's CSR values); the diagonal
// comes back in diag.  kmax: the largest k of the wave (wave-uniform).
template <typename T, int SLOTS, bool MASS, int QL, typename Emit>
__device__ __forceinline__ void ring_row_coef(const RingArgs<T> &a, const CoefArgs<T> &b, const SrcLanes<T> &pk,
                                              const SrcLanes<T> &pc, const RingRec<SLOTS> &rec, uint32_t lv,
                                              const T *xy, int kmax, T &diag, Emit &&emit) {
  const int k = rec.k();
  RecCursor<SLOTS> cur(rec);
  T xv, yv, pcx, pcy;
  lds_xy(xy, lv, xv, yv);
  const uint32_t id0 = cur.id();
  const int pos0 = cur.at();
  lds_xy(xy, id0, pcx, pcy);
  T sum_st = T(0), dmass = T(0), carry = T(0), wrapv = T(0), e0 = T(0);
#pragma unroll 1
  for (int i = 0; i < kmax; ++i) {
    const uint32_t id_i = cur.id();
    const int pos_i = cur.at();
    const uint32_t flag = i < k ? cur.flag() : 0u;
    cur.next();
    // neighbour behind slot i: slot i + 1, or slot 0 where the fan closes
    const uint32_t idn = (i + 1 < SLOTS && i + 1 != k) ? cur.id() : id0;
    T pnx, pny;
    lds_xy(xy, idn, pnx, pny);
    const T ecx = pcx - xv, ecy = pcy - yv, enx = pnx - xv, eny = pny - yv;
    const T qc = ecx * ecx + ecy * ecy, qn = enx * enx + eny * eny;
    const T p = ecx * enx + ecy * eny;
    const T cross = ecx * eny - ecy * enx;  // +- the signed determinant (element_tri.py:139)
    // the triangle's integration points x_q = bar(q)^T X (basis.py:90-91), vertices (v, n_i, n_next);
    // a slot without a triangle evaluates at the row's own vertex
    const T x1 = flag ? pcx : xv, y1 = flag ? pcy : yv, x2 = flag ? pnx : xv, y2 = flag ? pny : yv;
    T xq[QL], yq[QL], fv[QL];
#pragma unroll
    for (int q = 0; q < QL; ++q) {
      xq[q] = (a.lam[0][q] * xv + a.lam[1][q] * x1) + a.lam[2][q] * x2;
      yq[q] = (a.lam[0][q] * yv + a.lam[1][q] * y1) + a.lam[2][q] * y2;
    }
    T wk = a.stiff_w, mvv = a.mass_d, mvi = a.mass_o, mvn = a.mass_o;
    // ONE call site of the interpreter: pass 0 kappa, pass 1 c (both conditions wave-uniform)
#pragma unroll 1
    for (int pass = 0; pass < (MASS ? 2 : 1); ++pass) {
      if (!(pass == 0 ? b.has_kappa : b.has_c)) continue;
      SrcLanes<T> prog;
      prog.op = pass == 0 ? pk.op : pc.op;
      prog.c = pass == 0 ? pk.c : pc.c;
      prog.n_ops = pass == 0 ? pk.n_ops : pc.n_ops;
      src_run<T, QL>(prog, xq, yq, fv);
      if (pass == 0) {
        T w = T(0);
#pragma unroll
        for (int q = 0; q < QL; ++q) w = w + a.hw[q] * fv[q];
        wk = b.alpha * w;
      } else {
        T s00 = T(0), s01 = T(0), s02 = T(0);
#pragma unroll
        for (int q = 0; q < QL; ++q) {
          const T f0 = (a.hw[q] * fv[q]) * a.lam[0][q];
          s00 = s00 + f0 * a.lam[0][q];
          s01 = s01 + f0 * a.lam[1][q];
          s02 = s02 + f0 * a.lam[2][q];
        }
        mvv = b.beta * s00;
        mvi = b.beta * s01;
        mvn = b.beta * s02;
      }
    }
    const T cs = flag_weight<T>(wk, flag) * fast_rcp<T>(flag ? cross : T(1));
    T here = cs * (p - qn), next = cs * (p - qc);  // to column n_i, to column n_next
    sum_st = sum_st + (here + next);
    if (MASS) {
      // selects, not products with a zero determinant: a discarded program value may be anything
      const T sdet = flag_weight<T>(T(1), flag) * cross;
      here = here + (flag ? mvi * sdet : T(0));
      next = next + (flag ? mvn * sdet : T(0));
      dmass = dmass + (flag ? mvv * sdet : T(0));
    }
    const T entry = here + carry;
    carry = next;
    wrapv = i + 1 == k ? next : wrapv;  // the closing triangle's second share belongs to slot 0
    if (i == 0)
      e0 = here;
    else
      emit(i < k, id_i, pos_i, entry);
    pcx = pnx;
    pcy = pny;
  }
  emit(k > 0, id0, pos0, e0 + wrapv);
  diag = dmass - sum_st;
}

// What both coefficient launches prepare alike once the entry point's own refusals are through:
// the quadrature tables, the programs, the plan's arguments.  `tables` comes from build_tri_tables.
template <typename T>
static int coef_launch_init(const TriTables &tables, const void *coords, int64_t n_verts, double alpha, double beta,
                            const tfem_source_program *kappa, const tfem_source_program *c,
                            const unsigned char *plan, const int64_t *z, CoefLaunch<T> &K) {
  int st = ring_args_init<T>(tables, z, coords, plan, n_verts, alpha, beta, K.a);
  if (st != TFEM_OK) return st;
  std::memset(&K.b, 0, sizeof(K.b));
  if (kappa) st = src_convert<T>(kappa, &K.b.kappa);
  if (st == TFEM_OK && c) st = src_convert<T>(c, &K.b.c);
  if (st != TFEM_OK) return st;
  for (int i = 0; i < 3; ++i)
    for (int q = 0; q < tables.nq; ++q) K.a.lam[i][q] = T(tables.lam[q][i]);
  for (int q = 0; q < tables.nq; ++q) K.a.hw[q] = T(tables.hw[q]);
  // a term whose scalar factor is zero takes no program
  K.b.has_kappa = kappa != nullptr && alpha != 0.0;
  K.b.has_c = c != nullptr && beta != 0.0;
  K.b.alpha = T(alpha);
  K.b.beta = T(beta);
  return TFEM_OK;
}

}  // namespace tfem
