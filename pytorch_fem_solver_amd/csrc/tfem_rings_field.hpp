// What the coefficient-data launches over a ring plan share (k_p1_field_rows in
// tfem_rings_field.hip, k_p1_field_rows_multi in tfem_rings_field_multi.hip): the kernel's
// parameter, the slot codes of a row, the row from the tile's element table (ring_row_field), the
// element ids and values of a tile, the fill of the element table and the host's argument set-up.
// The header of tfem_rings_field.hip says what the table holds and how a row reads it.
#pragma once

#include "tfem_rings_coef.hpp"

namespace tfem {

constexpr size_t kFieldLdsLimit = 64 * 1024;

template <typename T>
struct FieldArgs {
  const T *u;
  T *y;
  const T *kappa, *c;  // (n_elems, kappa_nq) / (n_elems, c_nq) values
  unsigned u_bytes, y_bytes, kappa_bytes, c_bytes;
  int kappa_nq, c_nq;  // Q: a value per integration point; 1: one per element; 0: the constant 1
  T alpha, beta;
};

template <typename T>
struct FieldLaunch {  // the kernel's only parameter
  RingArgs<T> a;
  FieldArgs<T> b;
};

// The 12-bit slot codes of a row in fan order, one per pop (packed as the plan packs them).
template <int SLOTS>
struct CodeCursor {
  static constexpr int kWords = (12 * SLOTS + 31) / 32;  // 3 or 6
  uint32_t w[kWords];
  __device__ __forceinline__ uint32_t code() const { return w[0] & 0xFFFu; }
  __device__ __forceinline__ void next() {
#pragma unroll
    for (int j = 0; j + 1 < kWords; ++j) w[j] = (w[j] >> 12) | (w[j + 1] << 20);
    w[kWords - 1] >>= 12;
  }
};

// Reals per staged element: wk, then m00 m01 m02 m11 m12 m22.
template <bool MASS>
constexpr int field_elem_reals() { return MASS ? 7 : 1; }

// The row of local vertex `lv` from the element table `etab`: ring_row_coef with the per-triangle
// numbers read from LDS instead of evaluated.  emit(live, id, pos, value) once per slot, the diagonal
// in diag; kmax: the largest fan of the wave (wave-uniform).
template <typename T, int SLOTS, bool MASS, typename Emit>
__device__ __forceinline__ void ring_row_field(const RingRec<SLOTS> &rec, CodeCursor<SLOTS> &ec, uint32_t lv,
                                               const T *xy, const T *etab, int kmax, T &diag, Emit &&emit) {
  constexpr int ES = field_elem_reals<MASS>();
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
    const uint32_t code = ec.code();
    ec.next();
    // neighbour behind slot i: slot i + 1, or slot 0 where the fan closes
    const uint32_t idn = (i + 1 < SLOTS && i + 1 != k) ? cur.id() : id0;
    T pnx, pny;
    lds_xy(xy, idn, pnx, pny);
    const T ecx = pcx - xv, ecy = pcy - yv, enx = pnx - xv, eny = pny - yv;
    const T qc = ecx * ecx + ecy * ecy, qn = enx * enx + eny * eny;
    const T p = ecx * enx + ecy * eny;
    const T cross = ecx * eny - ecy * enx;  // +- the signed determinant (element_tri.py:139)
    // the slot's element in the tile's table; a slot without a triangle reads entry 0 and discards it
    const bool none = flag == 0u || code == 0xFFFu;
    const uint32_t el = none ? 0u : (code & 0x3FFu);
    const uint32_t loc = none ? 0u : (code >> 10);
    const T *ep = etab + el * unsigned(ES);
    const T wk = ep[0];
    const T cs = flag_weight<T>(wk, flag) * fast_rcp<T>(flag ? cross : T(1));
    T here = cs * (p - qn), next = cs * (p - qc);  // to column n_i, to column n_next
    sum_st = sum_st + (here + next);
    if (MASS) {
      // m[loc][loc], m[loc][loc + 1], m[loc][loc + 2] in the table's order (1 + index of i <= j)
      const T mvv = ep[(0x641u >> (4u * loc)) & 0xFu];
      const T ma = ep[(0x352u >> (4u * loc)) & 0xFu];
      const T mb = ep[(0x523u >> (4u * loc)) & 0xFu];
      // flag 1: the element holds (v, n_i, n_next): n_i is its local vertex loc + 1; flag 2: loc + 2
      const T mvi = (flag & 2u) ? mb : ma, mvn = (flag & 2u) ? ma : mb;
      // selects, not products with a zero determinant: a discarded table entry may be anything
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

constexpr unsigned kFieldNone = 0x3FFFFFFu;      // index behind every array: buffer loads give 0
constexpr unsigned kFieldBehind = 0xFFFFFFF0u;   // byte offset behind every value array

// vertex ids of a tile: the lane's own row and halo vertex number tid (as k_p1_apply_rows)
template <typename T, bool CHUNK>
__device__ __forceinline__ void field_load_ids(const RingArgs<T> &a, ring_rsrc_t r_plan, const RingDesc &d, int tid,
                                               int lane, unsigned &g_own, unsigned &g_halo) {
  const int r = d.row0 + lane;
  if (CHUNK)
    g_own = unsigned(d.gid0 + lane);
  else
    g_own = __builtin_amdgcn_raw_buffer_load_b32(
        r_plan, a.off_gid + (r < d.row1 ? unsigned(d.vert_off + r) : kFieldNone) * 4u, 0, 0);
  const int h = d.n_own + tid;
  g_halo = __builtin_amdgcn_raw_buffer_load_b32(
      r_plan, a.off_gid + (h < d.n_vert ? unsigned(d.vert_off + h) : kFieldNone) * 4u, 0, 0);
}

// element ids of a tile stored as a list (desc[18] = 0): position tid + 256 j of the list
template <typename T>
__device__ __forceinline__ void field_load_eids(const RingArgs<T> &a, ring_rsrc_t r_plan, const RingDesc &d, int tid,
                                                unsigned (&e)[kRingElemPerLane]) {
  if (d.elem_mode) return;  // runs of consecutive ids: nothing to fetch
#pragma unroll
  for (int j = 0; j < kRingElemPerLane; ++j) {
    const int l = tid + j * kRingBlock;
    e[j] = __builtin_amdgcn_raw_buffer_load_b32(
        r_plan, a.off_telems + (l < d.n_elem ? unsigned(d.elem_off + l) : kFieldNone) * 4u, 0, 0);
  }
}

// ... and of a tile stored as runs (desc[18] = 1): from the first ids of the runs and the list
// positions they end at (16 scalars of the plan), as load_fq derives them
template <typename T>
__device__ __forceinline__ void field_run_eids(const RingArgs<T> &a, const RingDesc &d, int tid,
                                               unsigned (&e)[kRingElemPerLane]) {
  if (!d.elem_mode) return;
  ring_const_i32 rg = (ring_const_i32)(uintptr_t)(a.plan + a.off_telems + 4u * unsigned(d.elem_off));
  int first[kRingElemRuns], upto[kRingElemRuns];
#pragma unroll
  for (int r = 0; r < kRingElemRuns; ++r) {
    first[r] = rg[r];
    upto[r] = rg[kRingElemRuns + r];
  }
#pragma unroll
  for (int j = 0; j < kRingElemPerLane; ++j) {
    const int l = tid + j * kRingBlock;
    int id = first[0] + l;
#pragma unroll
    for (int r = 1; r < kRingElemRuns; ++r) id = l >= upto[r - 1] ? first[r] + (l - upto[r - 1]) : id;
    e[j] = unsigned(id);
  }
}

template <typename T>
__device__ __forceinline__ T field_load_real(ring_rsrc_t r, unsigned byte) {
  if constexpr (sizeof(T) == 8) {
    const ru32x2 v{__builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0),
                   __builtin_amdgcn_raw_buffer_load_b32(r, byte + 4u, 0, 0)};
    return __builtin_bit_cast(double, v);
  } else {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0));
  }
}

// the values of one element: Q of them, or the element's one value for every point, or 1
template <typename T, int QL>
__device__ __forceinline__ void field_load_vals(ring_rsrc_t r, int nq, unsigned id, bool live, T (&v)[QL]) {
  if (nq == QL) {
    ring_load_fq<T, QL>(r, live ? id * unsigned(QL * sizeof(T)) : kFieldBehind, v);
  } else {
    const T one = nq == 1 ? field_load_real<T>(r, live ? id * unsigned(sizeof(T)) : kFieldBehind) : T(1);
#pragma unroll
    for (int q = 0; q < QL; ++q) v[q] = one;
  }
}

// wk and m_ij of the elements a lane has loaded (kv, cv: T [kRingElemPerLane][QL], cv one row without
// mass) -> the tile's element table, by their position in the tile's list.  A macro, not a function:
// the statements stand in the kernel's own body.  As a call -- even one that is always inlined --
// kv and cv are passed by address while the kernel's early passes run, which changed the register
// allocation of 22 of the 192 k_p1_field_rows instances (tools/kernel_regs.py); as text the single
// launch's code is what it was before both kernels shared it.
#define TFEM_FIELD_FILL_TABLE(T, MASS, QL, a, b, etab, tid, n_elem, kv, cv)                  \
  _Pragma("unroll") for (int e = 0; e < kRingElemPerLane; ++e) {                             \
    const int l = (tid) + e * kRingBlock;                                                    \
    if (l < (n_elem)) {                                                                      \
      T *ep = (etab) + l * field_elem_reals<MASS>();                                         \
      T w = T(0);                                                                            \
      _Pragma("unroll") for (int q = 0; q < QL; ++q) w = w + (a).hw[q] * (kv)[e][q];         \
      ep[0] = (b).alpha * w;                                                                 \
      if (MASS) {                                                                            \
        T f[QL];                                                                             \
        _Pragma("unroll") for (int q = 0; q < QL; ++q) f[q] = (a).hw[q] * (cv)[MASS ? e : 0][q]; \
        int at = 1;                                                                          \
        _Pragma("unroll") for (int i0 = 0; i0 < 3; ++i0) {                                   \
          _Pragma("unroll") for (int i1 = i0; i1 < 3; ++i1) {                                \
            T s = T(0);                                                                      \
            _Pragma("unroll") for (int q = 0; q < QL; ++q)                                   \
                s = s + (f[q] * (a).lam[i0][q]) * (a).lam[i1][q];                            \
            ep[at++] = (b).beta * s;                                                         \
          }                                                                                  \
        }                                                                                    \
      }                                                                                      \
    }                                                                                        \
  }

// What the launches with coefficient data set alike, after ring_args_init: the quadrature tables in
// T, the extents of the value arrays (checked), the plan's element sections and the fields.  The
// vectors (b.u, b.y and their extents) and a.vals are the caller's; they stay zero.
template <typename T>
static int field_args_init(const TriTables &tables, const void *coords, int64_t n_verts, double alpha, double beta,
                           const void *kappa, int kappa_nq, const void *c, int c_nq, int64_t n_elems,
                           const unsigned char *plan, const int64_t *z, FieldLaunch<T> &K) {
  int st = ring_args_init<T>(tables, z, coords, plan, n_verts, alpha, beta, K.a);
  if (st != TFEM_OK) return st;
  RingArgs<T> &a = K.a;
  FieldArgs<T> &b = K.b;
  std::memset(&b, 0, sizeof(b));
  for (int i = 0; i < 3; ++i)
    for (int q = 0; q < tables.nq; ++q) a.lam[i][q] = T(tables.lam[q][i]);
  for (int q = 0; q < tables.nq; ++q) a.hw[q] = T(tables.hw[q]);
  const int64_t bytes[2] = {kappa ? n_elems * kappa_nq * int64_t(sizeof(T)) : 0,
                            c ? n_elems * c_nq * int64_t(sizeof(T)) : 0};
  st = check_extents("ring kernel", bytes, 2);
  if (st != TFEM_OK) return st;
  a.off_elems = unsigned(z[15]);
  a.off_telems = unsigned(z[16]);
  a.lds_elem = int(std::max<int64_t>(z[17], 1));
  b.kappa = static_cast<const T *>(kappa);
  b.c = static_cast<const T *>(c);
  b.kappa_bytes = unsigned(bytes[0]);
  b.c_bytes = unsigned(bytes[1]);
  b.kappa_nq = kappa ? kappa_nq : 0;
  b.c_nq = c ? c_nq : 0;
  b.alpha = T(alpha);
  b.beta = T(beta);
  return TFEM_OK;
}

}  // namespace tfem
