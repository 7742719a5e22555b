// P1 operator with coefficient DATA on several vectors in one launch: Y = K U for
//     K = alpha * int kappa grad u . grad v  +  beta * int c u v
// over a ring plan, kappa and c values at the integration points (tfem_rings_field.hip), U and Y
// (n_verts, n_vec) row-major.
//
// What k_p1_field_rows pays beyond the constant-coefficient launch does not depend on the vector: the
// coalesced read of the tile's (E, Q) values and their reduction to one number per element
// (stiffness) or seven (with mass) in LDS, the row records, the slot codes and the coordinates.
// k_p1_field_rows_multi is its apply mode with the column staging of k_p1_coef_rows_multi
// (tfem_rings_coef_multi.hip, tfem_rings_cols.hpp): the element table of a tile is filled ONCE per
// pass -- by the statements of the single kernel in their order (TFEM_FIELD_FILL_TABLE), so it holds the
// same bits --, ring_row_field walks a row's fan ONCE per pass, and every finished entry is
// multiplied by NV staged columns: a column costs one LDS read and one multiply-add per entry.
//
// Every column's sum is formed in the order and with the operations of k_p1_field_rows:
//     yv = 0;  per emitted slot  yv = yv + (live ? value : 0) * us[live ? id : lv];  yv = yv + diag * us[lv]
// -- the build does not contract, so column j of Y is bit for bit tfem_p1_apply_rings_field on column
// j of U.
//
// LDS: xy[2 * lds_vert], us[NV * lds_vert] (16-byte aligned: lds_vert is even; a vertex's NV values
// consecutive), etab[ES * lds_elem].  Tile walk and the two barriers per tile: as k_p1_field_rows.
// The NV sums are the only values that live across ring_row_field's slot loop besides its own; no
// array is indexed by that loop's counter (no scratch memory).  No atomics.
#include "tfem_rings_cols.hpp"
#include "tfem_rings_field.hpp"

namespace tfem {

template <typename T>
struct FieldMultiLaunch {  // the kernel's only parameter
  FieldLaunch<T> f;        // f.b.u / f.b.y are not used: the vectors are m's
  ApplyMultiArgs<T> m;
};

template <typename T, int SLOTS, bool MASS, bool CHUNK, int QL, int NV>
__global__ __launch_bounds__(kRingBlock) void k_p1_field_rows_multi(const FieldMultiLaunch<T> L) {
  static_assert(NV >= 2 && NV % 2 == 0, "columns per pass come in pairs");
  const RingArgs<T> &a = L.f.a;
  const FieldArgs<T> &b = L.f.b;
  const ApplyMultiArgs<T> &m = L.m;
  constexpr int kEW = CodeCursor<SLOTS>::kWords;
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_smem[];
  T *xy = reinterpret_cast<T *>(ring_smem);  // [2 * lds_vert]
  T *us = static_cast<T *>(__builtin_assume_aligned(xy + 2 * a.lds_vert, 16));  // [NV * lds_vert]
  T *etab = xy + (2 + NV) * a.lds_vert;  // [ES * lds_elem]: what the tile's elements contribute
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per = (a.n_tiles + 7) / 8;
  const int xcd = blockIdx.x & 7;
  const int stride = gridDim.x >> 3;
  const ring_rsrc_t r_coords = ring_rsrc(a.coords, a.coords_bytes);
  const ring_rsrc_t r_plan = ring_rsrc(a.plan, a.plan_bytes);
  const ring_rsrc_t r_u = ring_rsrc(m.u, m.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(m.y, m.y_bytes);
  const ring_rsrc_t r_kappa = ring_rsrc(b.kappa, b.kappa_bytes);
  const ring_rsrc_t r_c = ring_rsrc(b.c, b.c_bytes);
  constexpr unsigned kRecBytes = unsigned(4 * RingRec<SLOTS>::kWords);
  constexpr unsigned kNone = kFieldNone;
  constexpr unsigned kNoByte = 0xFFFFFF00u;  // lanes without a vertex: their values are not staged
  const unsigned row_bytes = m.n_vec * unsigned(sizeof(T)), col_byte = m.col0 * unsigned(sizeof(T));

  auto tile_at = [&](int j) { return (j < per && xcd * per + j < a.n_tiles) ? xcd * per + j : -1; };

  int j = int(blockIdx.x >> 3);
  int t = tile_at(j);
  if (t < 0) return;  // whole workgroup, before any barrier
  RingDesc d = ring_desc<CHUNK>(a.plan, a.off_desc, t, wave);
  unsigned gid_own, gid_halo, eid[kRingElemPerLane] = {0u, 0u, 0u};
  field_load_ids<T, CHUNK>(a, r_plan, d, tid, lane, gid_own, gid_halo);
  field_load_eids<T>(a, r_plan, d, tid, eid);
  for (;;) {
    const int r = d.row0 + lane;
    const bool own = r < d.row1;
    const int h = d.n_own + tid;
    const bool halo = h < d.n_vert;
    // coordinates and the NV columns of this tile's vertices, the row record and its slot codes
    T own_x, own_y, halo_x, halo_y, own_u[NV], halo_u[NV];
    ring_load_xy<T>(r_coords, own ? gid_own : kNone, own_x, own_y);
    ring_load_xy<T>(r_coords, halo ? gid_halo : kNone, halo_x, halo_y);
    apply_load_cols<T, NV>(r_u, own ? gid_own * row_bytes + col_byte : kNoByte, own_u);
    apply_load_cols<T, NV>(r_u, halo ? gid_halo * row_bytes + col_byte : kNoByte, halo_u);
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
    // the values of the tile's elements: three per lane, by the ids that arrived a tile earlier
    field_run_eids<T>(a, d, tid, eid);
    T kv[kRingElemPerLane][QL], cv[MASS ? kRingElemPerLane : 1][QL];
#pragma unroll
    for (int e = 0; e < kRingElemPerLane; ++e) {
      const bool live = tid + e * kRingBlock < d.n_elem;
      field_load_vals<T, QL>(r_kappa, b.kappa_nq, eid[e], live, kv[e]);
      if (MASS) field_load_vals<T, QL>(r_c, b.c_nq, eid[e], live, cv[MASS ? e : 0]);
    }
    // vertex and element ids of the next tile, behind this tile's loads
    const unsigned gid_row = gid_own;
    const int n_elem = d.n_elem;
    const int t_n = tile_at(j + stride);
    RingDesc dn = d;
    unsigned eid_n[kRingElemPerLane] = {0u, 0u, 0u};
    if (t_n >= 0) {
      dn = ring_desc<CHUNK>(a.plan, a.off_desc, t_n, wave);
      field_load_ids<T, CHUNK>(a, r_plan, dn, tid, lane, gid_own, gid_halo);
      field_load_eids<T>(a, r_plan, dn, tid, eid_n);
    }
    if (own) {
      xy[2 * r] = own_x;
      xy[2 * r + 1] = own_y;
#pragma unroll
      for (int c = 0; c < NV; ++c) us[NV * r + c] = own_u[c];
    }
    if (halo) {
      xy[2 * h] = halo_x;
      xy[2 * h + 1] = halo_y;
#pragma unroll
      for (int c = 0; c < NV; ++c) us[NV * h + c] = halo_u[c];
    }
    // wk and m_ij of the elements just loaded -> LDS, by their position in the tile's list
    TFEM_FIELD_FILL_TABLE(T, MASS, QL, a, b, etab, tid, n_elem, kv, cv)
    __syncthreads();
    const uint32_t lv = unsigned(own ? r : 0);
    const int k = rec.k();
    int kmax = 0;  // the largest fan of the wave
#pragma unroll
    for (int i = 1; i <= SLOTS; ++i) kmax = __builtin_amdgcn_ballot_w64(k >= i) != 0ull ? i : kmax;
    T diag, yv[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) yv[c] = T(0);
    ring_row_field<T, SLOTS, MASS>(rec, ec, lv, xy, etab, kmax, diag, [&](bool live, uint32_t id, int, T value) {
      const T *ui = us + NV * (live ? id : lv);
      const T w = live ? value : T(0);
#pragma unroll
      for (int c = 0; c < NV; ++c) yv[c] = yv[c] + w * ui[c];
    });
    {
      const T *ud = us + NV * lv;
#pragma unroll
      for (int c = 0; c < NV; ++c) yv[c] = yv[c] + diag * ud[c];
    }
    if (own) apply_store_cols<T, NV>(r_y, gid_row * row_bytes + col_byte, yv, m.n_col);
    if (t_n < 0) break;
    __syncthreads();  // every row has read the tile's tables before the next tile overwrites them
    j += stride;
    t = t_n;
    d = dn;
#pragma unroll
    for (int e = 0; e < kRingElemPerLane; ++e) eid[e] = eid_n[e];
  }
}

template <typename T, int SLOTS, bool MASS, bool CHUNK, int NV>
static void *pick_field_multi_q(int nq) {
  switch (nq) {
    case 1: return reinterpret_cast<void *>(k_p1_field_rows_multi<T, SLOTS, MASS, CHUNK, 1, NV>);
    case 3: return reinterpret_cast<void *>(k_p1_field_rows_multi<T, SLOTS, MASS, CHUNK, 3, NV>);
    case 4: return reinterpret_cast<void *>(k_p1_field_rows_multi<T, SLOTS, MASS, CHUNK, 4, NV>);
    case 6: return reinterpret_cast<void *>(k_p1_field_rows_multi<T, SLOTS, MASS, CHUNK, 6, NV>);
    default: return nullptr;
  }
}

template <typename T, int SLOTS, int NV>
static void *pick_field_multi_chunk(bool mass, bool chunk, int nq) {
  if (mass)
    return chunk ? pick_field_multi_q<T, SLOTS, true, true, NV>(nq) : pick_field_multi_q<T, SLOTS, true, false, NV>(nq);
  return chunk ? pick_field_multi_q<T, SLOTS, false, true, NV>(nq) : pick_field_multi_q<T, SLOTS, false, false, NV>(nq);
}

// Widths of k_p1_field_rows_multi that are built (DESIGN.md section 3 says why these); 15-slot
// records up to kFieldWide15 columns, as k_p1_coef_rows_multi.
constexpr int kFieldWidths[] = {2, 4, 8};
constexpr int kFieldWide15 = 4;

template <typename T>
static void *pick_field_multi(int nv, int slots, bool mass, bool chunk, int nq) {
  if (slots == 7) {
    switch (nv) {
      case 2: return pick_field_multi_chunk<T, 7, 2>(mass, chunk, nq);
      case 4: return pick_field_multi_chunk<T, 7, 4>(mass, chunk, nq);
      default: return pick_field_multi_chunk<T, 7, 8>(mass, chunk, nq);
    }
  }
  return nv == 2 ? pick_field_multi_chunk<T, 15, 2>(mass, chunk, nq) : pick_field_multi_chunk<T, 15, 4>(mass, chunk, nq);
}

// LDS of a pass of nv columns: coordinates, nv reals per vertex, the element table.
static size_t field_multi_lds(int nv, int64_t lds_vert, int64_t lds_elem, bool mass, int real_bytes) {
  return size_t((2 + nv) * lds_vert + (mass ? 7 : 1) * lds_elem) * size_t(real_bytes);
}

// Y = K U for n_vec >= 2 columns: the passes of launch_coef_multi (the widest built width whose LDS
// fits kFieldLdsLimit -- no function attribute is set --, the narrowest that holds the rest for the
// last pass, TFEM_APPLY_NV as a cap) with the grid of launch_field.  The entry point has checked
// the sizes, the pointers of u and y, the fields, the plan's element stage, that width 2 fits and
// the order.
template <typename T>
static int launch_field_multi(const TriTables &tables, const void *coords, int64_t n_verts, double alpha, double beta,
                              const void *kappa, int kappa_nq, const void *c, int c_nq, int64_t n_elems,
                              const unsigned char *plan, const int64_t *z, const void *u, void *y, int64_t n_vec,
                              hipStream_t stream) {
  if (!coords || !plan || !y) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  FieldMultiLaunch<T> K;
  int st = field_args_init<T>(tables, coords, n_verts, alpha, beta, kappa, kappa_nq, c, c_nq, n_elems, plan, z, K.f);
  if (st != TFEM_OK) return st;
  const RingArgs<T> &a = K.f.a;
  ApplyMultiArgs<T> &m = K.m;
  m.u = static_cast<const T *>(u);
  m.y = static_cast<T *>(y);
  m.u_bytes = m.y_bytes = unsigned(n_verts * n_vec * int64_t(sizeof(T)));
  m.n_vec = unsigned(n_vec);
  const bool mass = beta != 0.0, chunk = z[13] != 0;
  const int slots = int(z[6]);
  int cap = 0;
  if (const char *env = std::getenv("TFEM_APPLY_NV")) cap = std::atoi(env);
  int widest = 0;
  for (int w : kFieldWidths)
    if (field_multi_lds(w, a.lds_vert, a.lds_elem, mass, int(sizeof(T))) <= kFieldLdsLimit && (cap < 2 || w <= cap) &&
        (slots == 7 || w <= kFieldWide15))
      widest = w;
  if (widest == 0)
    return fail(TFEM_ERR_UNSUPPORTED, "the coefficient-data block launch needs %zu bytes of LDS for two columns of "
                "this plan, more than %zu", field_multi_lds(kFieldWidths[0], a.lds_vert, a.lds_elem, mass, int(sizeof(T))),
                kFieldLdsLimit);
  const int per = int((z[0] + 7) / 8);
  for (int64_t col0 = 0; col0 < n_vec;) {
    const int64_t left = n_vec - col0;
    int nv = widest;
    for (int w : kFieldWidths)
      if (w >= left && w < nv) nv = w;
    m.col0 = unsigned(col0);
    m.n_col = unsigned(std::min<int64_t>(left, nv));
    void *kernel = pick_field_multi<T>(nv, slots, mass, chunk, tables.nq);
    if (!kernel) return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
    const size_t lds = field_multi_lds(nv, a.lds_vert, a.lds_elem, mass, int(sizeof(T)));
    int per_cu = 0;
    st = resident_per_cu(kernel, kRingBlock, lds, &per_cu);
    if (st != TFEM_OK) return st;
    const int blocks = std::min(per * 8, (device_cu_count() * per_cu / 8) * 8);
    void *params[] = {&K};
    hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(std::max(blocks, 8))), dim3(kRingBlock), params, lds, stream);
    if (e != hipSuccess) return fail(TFEM_ERR_HIP, "coefficient-data kernel launch: %s", hipGetErrorString(e));
    col0 += m.n_col;
  }
  return TFEM_OK;
}

}  // namespace tfem

extern "C" {

int tfem_p1_apply_rings_field_multi(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha,
                                    double beta, const void *kappa, int kappa_nq, const void *c, int c_nq,
                                    int64_t n_elems, const void *plan_device, const int64_t *plan_layout_host,
                                    const void *u, void *y, int64_t n_vec, void *stream) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (n_verts < 0 || n_elems < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  if (n_vec < 1) return fail(TFEM_ERR_INVALID_ARGUMENT, "n_vec must be at least 1");
  if (!u) return fail(TFEM_ERR_INVALID_ARGUMENT, "u is NULL (the diagonal: tfem_p1_apply_rings_field)");
  if (!kappa && !c)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "no coefficient data: constant coefficients take "
                "tfem_p1_apply_rings_multi");
  TriTables tables;
  const bool known = build_tri_tables(quad_order, real_bytes, &tables);  // an unknown order is refused last
  if (known && ((kappa && kappa_nq != 1 && kappa_nq != tables.nq) || (c && c_nq != 1 && c_nq != tables.nq)))
    return fail(TFEM_ERR_INVALID_ARGUMENT, "coefficient data: %d / %d values per element, expected 1 or %d",
                kappa ? kappa_nq : 0, c ? c_nq : 0, tables.nq);
  // the extents of u and y and of the values, before anything is derived from them
  const int64_t limit = int64_t(1) << 32;
  auto extent = [&](int64_t rows, int64_t per_row) {
    return (rows > 0 && per_row >= limit / rows) ? limit : rows * per_row * real_bytes;
  };
  const int64_t bytes[3] = {extent(n_verts, n_vec), kappa ? extent(n_elems, std::max(kappa_nq, 0)) : 0,
                            c ? extent(n_elems, std::max(c_nq, 0)) : 0};
  int st = check_extents("ring kernel", bytes, 3);
  if (st != TFEM_OK) return st;
  const char *ub = static_cast<const char *>(u), *yb = static_cast<const char *>(y);
  if (y && ub < yb + bytes[0] && yb < ub + bytes[0]) return fail(TFEM_ERR_INVALID_ARGUMENT, "u and y overlap");
  const int64_t *z = plan_layout_host;
  if (n_vec == 1)  // one column: the single-vector launch, same layout (its own plan checks)
    return tfem_p1_apply_rings_field(coords, real_bytes, n_verts, quad_order, alpha, beta, kappa, kappa_nq, c, c_nq,
                                     n_elems, plan_device, z, u, y, stream);
  if (z[23] > 0)
    return fail(TFEM_ERR_UNSUPPORTED, "a ring plan with long rows does not take coefficient data");
  if (z[0] > 0 && n_verts > 0) {
    if (z[18] == 0 || z[17] > kRingElemPerLane * kRingBlock)
      return fail(TFEM_ERR_UNSUPPORTED, "a tile of this ring plan has %lld elements: the coefficient-data launch "
                  "stages at most %d", (long long)z[17], kRingElemPerLane * kRingBlock);
    const int64_t lds_vert = (z[3] + 1) & ~int64_t(1), lds_elem = std::max<int64_t>(z[17], 1);
    const size_t lds = field_multi_lds(kFieldWidths[0], lds_vert, lds_elem, beta != 0.0, real_bytes);
    if (lds > kFieldLdsLimit)
      return fail(TFEM_ERR_UNSUPPORTED, "the coefficient-data block launch needs %zu bytes of LDS for two columns "
                  "of this plan (%lld vertices, %lld elements per tile), more than %zu", lds, (long long)z[3],
                  (long long)z[17], kFieldLdsLimit);
  }
  if (!known) return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if (z[0] == 0 || n_verts == 0) return TFEM_OK;
  const unsigned char *plan = static_cast<const unsigned char *>(plan_device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8 ? launch_field_multi<double>(tables, coords, n_verts, alpha, beta, kappa, kappa_nq, c, c_nq,
                                                      n_elems, plan, z, u, y, n_vec, s)
                         : launch_field_multi<float>(tables, coords, n_verts, alpha, beta, kappa, kappa_nq, c, c_nq,
                                                     n_elems, plan, z, u, y, n_vec, s);
}

}  // extern "C"
