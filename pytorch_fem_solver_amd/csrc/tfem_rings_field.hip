// P1 forms with coefficient DATA over a ring plan:
//     K = alpha * int kappa grad u . grad v  +  beta * int c u v
// (abstract_basis.py:74-93 applied to a caller's `kq * (v_grad @ v_grad.mT) + cq * (v @ v.mT)`), kappa
// and c given as VALUES at the integration points -- (n_elems, Q) in the caller's element order and
// the element's stored frame, q in the order of tfem_quadrature_rule, or one value per element --
// instead of source programs (tfem_rings_coef.hip): a previous iterate, a material constant per
// element, a network evaluated at basis.integration_points.  Assembled into the CSR values or
// applied matrix-free; nothing per element beyond the caller's values exists in memory.
//
// The lookup is the fused load vector's (load_eids / load_fq / park_g in tfem_rings_kernel.hpp): the
// plan lists every tile's elements ascending (tile_elems, as a list or as runs of consecutive ids,
// desc[18]) and gives every row one 12-bit code per fan slot (row_ecodes: tile-local element |
// local index of the row's vertex in that element << 10).  Per tile, before the rows run, every lane
// takes up to three elements of the list, loads their kappa and c values (coalesced: the list is
// ascending) and parks per tile-local element
//     wk   = alpha * sum_q (w_q / 2) kappa[e][q]
//     m_ij = beta * sum_q (w_q / 2) c[e][q] l_i(q) l_j(q)      (mass only; i <= j, six numbers)
// in LDS, in the ELEMENT's local order.  A row's slot reads wk, m[loc][loc], m[loc][loc + 1] and
// m[loc][loc + 2] (indices mod 3) through its code; the slot's orientation flag says which of the
// two off-diagonal numbers belongs to n_i and which to n_next (flag 1: the element holds
// (v, n_i, n_next) up to rotation, flag 2: (v, n_next, n_i)).  Every element's values are reduced
// once per tile that touches it, not once per row: what a row reads does not depend on the row, only
// the geometric factors do, so K_ij and K_ji still agree to rounding only.
//
// k_p1_field_rows: the tile walk of k_p1_coef_rows (one lane per row, coordinates -- and u for the
// apply mode -- in LDS); MODE = apply (y = K u), diag (y = diag K) or store (the row's CSR values,
// staged per wave and streamed out with ring_store / ring_store_run1).  The fan loop is the one of
// ring_row_coef: slot by slot, not unrolled, the record's fields and the slot codes popped from
// shift registers, a finished entry handed out per slot -- no register array is indexed by the loop
// counter and no kernel here uses scratch memory.  Slots without a triangle (flag 0, code 0xFFF)
// contribute nothing by select: what they read from the element table is discarded.  No atomics.
// Data with one value per element (*_nq == 1) is read once per element and never expanded.
//
// k_p1_field_adjoint: the derivative of g^T K u with respect to the values, element form (modelled on
// k_p1_residual_backward): one lane per element, g and u gathered at its three vertices for every
// column, summed over the columns in registers; every entry written once.
#include "tfem_rings_field.hpp"

namespace tfem {

constexpr int kFieldApply = 0, kFieldDiag = 1, kFieldStore = 2;

template <typename T, int SLOTS, bool MASS, bool CHUNK, int QL, int MODE>
__global__ __launch_bounds__(kRingBlock) void k_p1_field_rows(const FieldLaunch<T> L) {
  const RingArgs<T> &a = L.a;
  const FieldArgs<T> &b = L.b;
  constexpr int kEW = CodeCursor<SLOTS>::kWords;
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_smem[];
  T *xy = reinterpret_cast<T *>(ring_smem);  // [2 * lds_vert]
  T *us = xy + 2 * a.lds_vert;               // [lds_vert] (apply only)
  T *stage = xy + 2 * a.lds_vert;            // [waves][stage entries] (store only)
  // [ES * lds_elem] behind them: what the tile's elements contribute
  T *etab = xy + 2 * a.lds_vert +
            (MODE == kFieldApply ? a.lds_vert : MODE == kFieldStore ? kRingWaves * ring_stage_entries<T, SLOTS>() : 0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  T *my_stage = stage + wave * ring_stage_entries<T, SLOTS>();
  const int per = (a.n_tiles + 7) / 8;
  const int xcd = blockIdx.x & 7;
  const int stride = gridDim.x >> 3;
  const ring_rsrc_t r_coords = ring_rsrc(a.coords, a.coords_bytes);
  const ring_rsrc_t r_plan = ring_rsrc(a.plan, a.plan_bytes);
  const ring_rsrc_t r_u = ring_rsrc(b.u, b.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(b.y, b.y_bytes);
  const ring_rsrc_t r_vals = ring_rsrc(a.vals, a.vals_bytes);
  const ring_rsrc_t r_kappa = ring_rsrc(b.kappa, b.kappa_bytes);
  const ring_rsrc_t r_c = ring_rsrc(b.c, b.c_bytes);
  constexpr unsigned kRecBytes = unsigned(4 * RingRec<SLOTS>::kWords);
  constexpr unsigned kNone = kFieldNone;
  constexpr int kSpare = 64 * (SLOTS + 1);  // the stage's spare entries (ring_stage_entries)

  auto tile_at = [&](int j) { return (j < per && xcd * per + j < a.n_tiles) ? xcd * per + j : -1; };
  // the ids and values of a tile: tfem_rings_field.hpp
  auto load_ids = [&](const RingDesc &d, unsigned &g_own, unsigned &g_halo) {
    field_load_ids<T, CHUNK>(a, r_plan, d, tid, lane, g_own, g_halo);
  };
  auto load_eids = [&](const RingDesc &d, unsigned (&e)[kRingElemPerLane]) { field_load_eids<T>(a, r_plan, d, tid, e); };
  auto run_eids = [&](const RingDesc &d, unsigned (&e)[kRingElemPerLane]) { field_run_eids<T>(a, d, tid, e); };
  auto load_u = [&](unsigned g) { return field_load_real<T>(r_u, g * unsigned(sizeof(T))); };
  auto load_vals = [&](ring_rsrc_t r, int nq, unsigned id, bool live, T (&v)[QL]) {
    field_load_vals<T, QL>(r, nq, id, live, v);
  };

  int j = int(blockIdx.x >> 3);
  int t = tile_at(j);
  if (t < 0) return;  // whole workgroup, before any barrier
  RingDesc d = ring_desc<CHUNK>(a.plan, a.off_desc, t, wave);
  unsigned gid_own, gid_halo, eid[kRingElemPerLane] = {0u, 0u, 0u};
  load_ids(d, gid_own, gid_halo);
  load_eids(d, eid);
  for (;;) {
    const int r = d.row0 + lane;
    const bool own = r < d.row1;
    const int h = d.n_own + tid;
    const bool halo = h < d.n_vert;
    // coordinates and u of this tile's vertices, the row record and its slot codes
    T own_x, own_y, halo_x, halo_y, own_u = T(0), halo_u = T(0);
    ring_load_xy<T>(r_coords, own ? gid_own : kNone, own_x, own_y);
    ring_load_xy<T>(r_coords, halo ? gid_halo : kNone, halo_x, halo_y);
    if (MODE == kFieldApply) {
      own_u = load_u(own ? gid_own : kNone);
      halo_u = load_u(halo ? gid_halo : kNone);
    }
    const unsigned row = own ? unsigned(d.row_off + r) : kNone;
    RingRec<SLOTS> rec;
    ring_load_rec<SLOTS>(r_plan, a.off_rows + row * kRecBytes, rec);
    CodeCursor<SLOTS> ec;
#pragma unroll
    for (int i = 0; i < kEW; i += 3) {
      const ru32x3 v = __builtin_amdgcn_raw_buffer_load_b96(r_plan, a.off_elems + row * unsigned(4 * kEW) + unsigned(4 * i), 0, 0);
      ec.w[i] = v.x;
      ec.w[i + 1] = v.y;
      ec.w[i + 2] = v.z;
    }
    int rowstart = 0;
    if (MODE == kFieldStore && !CHUNK)
      rowstart = int(__builtin_amdgcn_raw_buffer_load_b32(r_plan, a.off_rowstart + row * 4u, 0, 0));
    // the values of the tile's elements: three per lane, by the ids that arrived a tile earlier
    run_eids(d, eid);
    T kv[kRingElemPerLane][QL], cv[MASS ? kRingElemPerLane : 1][QL];
#pragma unroll
    for (int e = 0; e < kRingElemPerLane; ++e) {
      const bool live = tid + e * kRingBlock < d.n_elem;
      load_vals(r_kappa, b.kappa_nq, eid[e], live, kv[e]);
      if (MASS) load_vals(r_c, b.c_nq, eid[e], live, cv[MASS ? e : 0]);
    }
    // vertex and element ids of the next tile, behind this tile's loads
    const unsigned gid_row = gid_own;
    const int n_elem = d.n_elem;
    const int t_n = tile_at(j + stride);
    RingDesc dn = d;
    unsigned eid_n[kRingElemPerLane] = {0u, 0u, 0u};
    if (t_n >= 0) {
      dn = ring_desc<CHUNK>(a.plan, a.off_desc, t_n, wave);
      load_ids(dn, gid_own, gid_halo);
      load_eids(dn, eid_n);
    }
    if (own) {
      xy[2 * r] = own_x;
      xy[2 * r + 1] = own_y;
      if (MODE == kFieldApply) us[r] = own_u;
    }
    if (halo) {
      xy[2 * h] = halo_x;
      xy[2 * h + 1] = halo_y;
      if (MODE == kFieldApply) us[h] = halo_u;
    }
    // wk and m_ij of the elements just loaded -> LDS, by their position in the tile's list
    TFEM_FIELD_FILL_TABLE(T, MASS, QL, a, b, etab, tid, n_elem, kv, cv)
    __syncthreads();
    const uint32_t lv = unsigned(own ? r : 0);
    const int k = rec.k();
    int kmax = 0;  // the largest fan of the wave
#pragma unroll
    for (int i = 1; i <= SLOTS; ++i) kmax = __builtin_amdgcn_ballot_w64(k >= i) != 0ull ? i : kmax;
    T diag, yv = T(0);
    int total = 0, pre = 0;
    const int len = k > 0 ? k + 1 : 0;
    if (MODE == kFieldStore) {  // the wave's stage, compact and in CSR order (ring_stage)
      const int incl = wave_inclusive_scan(len);
      pre = incl - len;
      total = __builtin_amdgcn_readlane(incl, 63);
    }
    ring_row_field<T, SLOTS, MASS>(rec, ec, lv, xy, etab, kmax, diag,
                                   [&](bool live, uint32_t id, int pos, T value) {
                                     if (MODE == kFieldApply) yv = yv + (live ? value : T(0)) * us[live ? id : lv];
                                     if (MODE == kFieldStore) my_stage[live ? pre + pos : kSpare] = value;
                                   });
    if (MODE == kFieldStore) {
      my_stage[k > 0 ? pre + rec.dpos() : kSpare] = diag;
      if (CHUNK) {  // one run per wave by construction, its CSR offset in the descriptor
        __builtin_amdgcn_wave_barrier();
        ring_store_run1<T, SLOTS>(my_stage, total, d.rs0, r_vals, a.plain_stores);
        __builtin_amdgcn_wave_barrier();
      } else {
        ring_store<T, SLOTS>(my_stage, total, pre, rowstart, len, r_vals, a.plain_stores);
      }
    } else {
      yv = MODE == kFieldDiag ? diag : yv + diag * us[lv];
      if (own) {
        if constexpr (sizeof(T) == 8)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, yv), r_y, gid_row * 8u, 0, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv), r_y, gid_row * 4u, 0, 0);
      }
    }
    if (t_n < 0) break;
    __syncthreads();  // every row has read the tile's tables before the next tile overwrites them
    j += stride;
    t = t_n;
    d = dn;
#pragma unroll
    for (int e = 0; e < kRingElemPerLane; ++e) eid[e] = eid_n[e];
  }
}

template <typename T, int SLOTS, bool MASS, bool CHUNK, int QL>
static void *pick_field_mode(int mode) {
  switch (mode) {
    case kFieldApply: return reinterpret_cast<void *>(k_p1_field_rows<T, SLOTS, MASS, CHUNK, QL, kFieldApply>);
    case kFieldDiag: return reinterpret_cast<void *>(k_p1_field_rows<T, SLOTS, MASS, CHUNK, QL, kFieldDiag>);
    default: return reinterpret_cast<void *>(k_p1_field_rows<T, SLOTS, MASS, CHUNK, QL, kFieldStore>);
  }
}

template <typename T, int SLOTS, bool MASS, bool CHUNK>
static void *pick_field_q(int nq, int mode) {
  switch (nq) {
    case 1: return pick_field_mode<T, SLOTS, MASS, CHUNK, 1>(mode);
    case 3: return pick_field_mode<T, SLOTS, MASS, CHUNK, 3>(mode);
    case 4: return pick_field_mode<T, SLOTS, MASS, CHUNK, 4>(mode);
    case 6: return pick_field_mode<T, SLOTS, MASS, CHUNK, 6>(mode);
    default: return nullptr;
  }
}

template <typename T, int SLOTS>
static void *pick_field_chunk(bool mass, bool chunk, int nq, int mode) {
  if (mass)
    return chunk ? pick_field_q<T, SLOTS, true, true>(nq, mode) : pick_field_q<T, SLOTS, true, false>(nq, mode);
  return chunk ? pick_field_q<T, SLOTS, false, true>(nq, mode) : pick_field_q<T, SLOTS, false, false>(nq, mode);
}

template <typename T>
static int launch_field(const TriTables &tables, const void *coords, int64_t n_verts, double alpha, double beta,
                        const void *kappa, int kappa_nq, const void *c, int c_nq, int64_t n_elems,
                        const unsigned char *plan, const int64_t *z, int mode, void *vals, const void *u, void *y,
                        hipStream_t stream) {
  if (z[0] == 0 || n_verts == 0) return TFEM_OK;
  if (!coords || !plan || !(mode == kFieldStore ? vals : y)) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  if (z[23] > 0)
    return fail(TFEM_ERR_UNSUPPORTED, "a ring plan with long rows does not take coefficient data");
  if (z[18] == 0 || z[17] > kRingElemPerLane * kRingBlock)
    return fail(TFEM_ERR_UNSUPPORTED, "a tile of this ring plan has %lld elements: the coefficient-data launch "
                "stages at most %d", (long long)z[17], kRingElemPerLane * kRingBlock);
  FieldLaunch<T> K;
  int st = field_args_init<T>(tables, coords, n_verts, alpha, beta, kappa, kappa_nq, c, c_nq, n_elems, plan, z, K);
  if (st != TFEM_OK) return st;
  RingArgs<T> &a = K.a;
  FieldArgs<T> &b = K.b;
  // the CSR values: bounded by rows x longest row, as in the coefficient-program launch
  const int64_t bytes[2] = {n_verts * int64_t(sizeof(T)), mode == kFieldStore ? z[1] * z[5] * int64_t(sizeof(T)) : 0};
  st = check_extents("ring kernel", bytes, 2);
  if (st != TFEM_OK) return st;
  const bool mass = beta != 0.0, chunk = z[13] != 0;
  const int slots = int(z[6]);
  const size_t lds = size_t((mode == kFieldApply ? 3 : 2) * a.lds_vert) * sizeof(T) +
                     (mode == kFieldStore ? size_t(kRingWaves) * size_t(64 * (slots + 1) + 2) * sizeof(T) : 0) +
                     size_t(mass ? 7 : 1) * size_t(a.lds_elem) * sizeof(T);
  if (lds > kFieldLdsLimit)
    return fail(TFEM_ERR_UNSUPPORTED, "the coefficient-data launch needs %zu bytes of LDS for this plan (%lld "
                "vertices, %lld elements per tile), more than %zu", lds, (long long)z[3], (long long)z[17],
                kFieldLdsLimit);
  b.u = static_cast<const T *>(u);
  b.y = static_cast<T *>(y);
  b.u_bytes = mode == kFieldApply ? unsigned(bytes[0]) : 0u;
  b.y_bytes = mode == kFieldStore ? 0u : unsigned(bytes[0]);
  a.vals = static_cast<T *>(vals);
  a.vals_bytes = mode == kFieldStore ? unsigned(bytes[1]) : 0u;
  a.plain_stores = 1;  // the matrix alone: the store policy of the matrix-only ring launch
  void *kernel = slots == 7 ? pick_field_chunk<T, 7>(mass, chunk, tables.nq, mode)
                            : pick_field_chunk<T, 15>(mass, chunk, tables.nq, mode);
  if (!kernel) return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  int per_cu = 0;
  st = resident_per_cu(kernel, kRingBlock, lds, &per_cu);
  if (st != TFEM_OK) return st;
  const int per = int((z[0] + 7) / 8);
  const int blocks = std::min(per * 8, (device_cu_count() * per_cu / 8) * 8);
  void *params[] = {&K};
  hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(std::max(blocks, 8))), dim3(kRingBlock), params, lds, stream);
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "coefficient-data kernel launch: %s", hipGetErrorString(e));
  return TFEM_OK;
}

static bool ranges_overlap(const void *p, const void *q, int64_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + uintptr_t(bytes) && b < a + uintptr_t(bytes);
}

static int field_entry(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha, double beta,
                       const void *kappa, int kappa_nq, const void *c, int c_nq, int64_t n_elems,
                       const void *plan_device, const int64_t *plan_layout_host, int mode, void *vals, const void *u,
                       void *y, void *stream) {
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (n_verts < 0 || n_elems < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  if (!kappa && !c)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "no coefficient data: constant coefficients take "
                "tfem_p1_assemble_rings / tfem_p1_apply_rings");
  TriTables tables;
  if (!build_tri_tables(quad_order, real_bytes, &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if ((kappa && kappa_nq != 1 && kappa_nq != tables.nq) || (c && c_nq != 1 && c_nq != tables.nq))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "coefficient data: %d / %d values per element, expected 1 or %d",
                kappa ? kappa_nq : 0, c ? c_nq : 0, tables.nq);
  if (u && y && n_verts > 0 && ranges_overlap(u, y, n_verts * int64_t(real_bytes)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "u and y overlap");
  const unsigned char *plan = static_cast<const unsigned char *>(plan_device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8 ? launch_field<double>(tables, coords, n_verts, alpha, beta, kappa, kappa_nq, c, c_nq,
                                                n_elems, plan, plan_layout_host, mode, vals, u, y, s)
                         : launch_field<float>(tables, coords, n_verts, alpha, beta, kappa, kappa_nq, c, c_nq,
                                               n_elems, plan, plan_layout_host, mode, vals, u, y, s);
}

// ------------------------------------------------------------------------------------------------
// The adjoint in the values
// ------------------------------------------------------------------------------------------------
constexpr int kAdjBlock = 256;

template <typename T>
struct FieldAdjArgs {
  const T *coords;      // (n_verts, 2)
  const int32_t *conn;  // (n_elems, 3)
  const T *g, *u;       // (n_verts, n_vec), row-major
  T *grad_kappa, *grad_c;  // (n_elems, Q) or NULL
  int64_t n_elems, n_vec;
  T alpha, beta;
  T hw[kMaxQuad];
  T lam[3][kMaxQuad];
};

template <typename T, int Q>
__global__ __launch_bounds__(kAdjBlock) void k_p1_field_adjoint(const FieldAdjArgs<T> a) {
  const int64_t e = int64_t(blockIdx.x) * kAdjBlock + threadIdx.x;
  if (e >= a.n_elems) return;
  const int32_t *cn = a.conn + 3 * e;
  const int64_t v[3] = {cn[0], cn[1], cn[2]};
  // J = X^T G (basis.py:87-88), signed det and (1/det) adj (element_tri.py:132-145), gradients
  // G @ inv (element_tri.py:41) -- res_geometry's operations
  const T x0 = a.coords[2 * v[0]], y0 = a.coords[2 * v[0] + 1];
  const T ja = a.coords[2 * v[1]] - x0, jb = a.coords[2 * v[2]] - x0;
  const T jc = a.coords[2 * v[1] + 1] - y0, jd = a.coords[2 * v[2] + 1] - y0;
  const T det = ja * jd - jb * jc;
  const T r = T(1) / det;
  const T inv[2][2] = {{r * jd, r * (-jb)}, {r * (-jc), r * ja}};
  T vg[3][2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    vg[0][k] = (-inv[0][k]) + (-inv[1][k]);
    vg[1][k] = inv[0][k];
    vg[2][k] = inv[1][k];
  }
  T sk = T(0), sc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) sc[q] = T(0);
  for (int64_t col = 0; col < a.n_vec; ++col) {
    const T g0 = a.g[v[0] * a.n_vec + col], g1 = a.g[v[1] * a.n_vec + col], g2 = a.g[v[2] * a.n_vec + col];
    const T u0 = a.u[v[0] * a.n_vec + col], u1 = a.u[v[1] * a.n_vec + col], u2 = a.u[v[2] * a.n_vec + col];
    const T ggx = (g0 * vg[0][0] + g1 * vg[1][0]) + g2 * vg[2][0];
    const T ggy = (g0 * vg[0][1] + g1 * vg[1][1]) + g2 * vg[2][1];
    const T ugx = (u0 * vg[0][0] + u1 * vg[1][0]) + u2 * vg[2][0];
    const T ugy = (u0 * vg[0][1] + u1 * vg[1][1]) + u2 * vg[2][1];
    sk = sk + (ggx * ugx + ggy * ugy);
    if (a.grad_c) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const T gq = (g0 * a.lam[0][q] + g1 * a.lam[1][q]) + g2 * a.lam[2][q];
        const T uq = (u0 * a.lam[0][q] + u1 * a.lam[1][q]) + u2 * a.lam[2][q];
        sc[q] = sc[q] + gq * uq;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const T dx = a.hw[q] * det;  // the reference's signed determinant
    if (a.grad_kappa) a.grad_kappa[Q * e + q] = a.alpha * (dx * sk);
    if (a.grad_c) a.grad_c[Q * e + q] = a.beta * (dx * sc[q]);
  }
}

template <typename T>
static int launch_field_adjoint(const TriTables &tables, const void *coords, const void *conn, int64_t n_elems,
                                double alpha, double beta, const void *g, const void *u, int64_t n_vec,
                                void *grad_kappa, void *grad_c, hipStream_t stream) {
  FieldAdjArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  a.coords = static_cast<const T *>(coords);
  a.conn = static_cast<const int32_t *>(conn);
  a.g = static_cast<const T *>(g);
  a.u = static_cast<const T *>(u);
  a.grad_kappa = static_cast<T *>(grad_kappa);
  a.grad_c = static_cast<T *>(grad_c);
  a.n_elems = n_elems;
  a.n_vec = n_vec;
  a.alpha = T(alpha);
  a.beta = T(beta);
  for (int q = 0; q < tables.nq; ++q) {
    a.hw[q] = T(tables.hw[q]);
    for (int i = 0; i < 3; ++i) a.lam[i][q] = T(tables.lam[q][i]);
  }
  const dim3 grid(unsigned((n_elems + kAdjBlock - 1) / kAdjBlock)), block(kAdjBlock);
  switch (tables.nq) {
    case 1: hipLaunchKernelGGL((k_p1_field_adjoint<T, 1>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_p1_field_adjoint<T, 3>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((k_p1_field_adjoint<T, 4>), grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL((k_p1_field_adjoint<T, 6>), grid, block, 0, stream, a); break;
    default: return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "coefficient-data adjoint launch: %s", hipGetErrorString(e));
  return TFEM_OK;
}

}  // namespace tfem

extern "C" {

int tfem_p1_rings_field(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha, double beta,
                        const void *kappa, int kappa_nq, const void *c, int c_nq, int64_t n_elems,
                        const void *plan_device, const int64_t *plan_layout_host, void *vals, void *stream) {
  return tfem::field_entry(coords, real_bytes, n_verts, quad_order, alpha, beta, kappa, kappa_nq, c, c_nq, n_elems,
                           plan_device, plan_layout_host, tfem::kFieldStore, vals, nullptr, nullptr, stream);
}

int tfem_p1_apply_rings_field(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha,
                              double beta, const void *kappa, int kappa_nq, const void *c, int c_nq, int64_t n_elems,
                              const void *plan_device, const int64_t *plan_layout_host, const void *u, void *y,
                              void *stream) {
  return tfem::field_entry(coords, real_bytes, n_verts, quad_order, alpha, beta, kappa, kappa_nq, c, c_nq, n_elems,
                           plan_device, plan_layout_host, u ? tfem::kFieldApply : tfem::kFieldDiag, nullptr, u, y,
                           stream);
}

int tfem_p1_field_adjoint(const void *coords, int real_bytes, const void *conn, int64_t n_elems, int64_t n_verts,
                          int quad_order, double alpha, double beta, const void *g, const void *u, int64_t n_vec,
                          void *grad_kappa, void *grad_c, void *stream) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (n_elems < 0 || n_verts < 0 || n_vec < 1) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  TriTables tables;
  if (!build_tri_tables(quad_order, real_bytes, &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if (n_elems >= (int64_t(1) << 31) * kAdjBlock)
    return fail(TFEM_ERR_INDEX_RANGE, "too many elements for one launch");
  if (n_elems == 0 || (!grad_kappa && !grad_c)) return TFEM_OK;
  if (!coords || !conn || !g || !u) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8 ? launch_field_adjoint<double>(tables, coords, conn, n_elems, alpha, beta, g, u, n_vec,
                                                        grad_kappa, grad_c, s)
                         : launch_field_adjoint<float>(tables, coords, conn, n_elems, alpha, beta, g, u, n_vec,
                                                       grad_kappa, grad_c, s);
}

}  // extern "C"
