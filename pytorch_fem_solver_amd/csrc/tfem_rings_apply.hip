// Matrix-free P1 operator over a ring plan: y = (alpha * stiffness + beta * mass) u without the
// CSR values (abstract_basis.py:74-93 with basis.py:64-85, applied instead of stored).
//
// The row form of k_p1_rings (tfem_rings.hip) already builds every row of K in registers: one
// lane owns one vertex v, ring_row evaluates its fan from tile-local coordinates in LDS and hands
// back the diagonal and the off-diagonal entries in fan order.  Here the tile also stages u of its
// local vertices (owned rows and halo) beside the coordinates, and the lane forms
//     y_v = K_vv u_v + sum_i K_{v, n_i} u_{n_i}
// and writes that one number: no CSR stage, no permutation, no row offsets.  With chunked plans a
// wave's rows are 64 consecutive vertices, so the stores of y coalesce.  u == NULL writes diag(K)
// (Jacobi preconditioner).
//
// Tile walk: as the matrix-only launches of k_p1_rings (one contiguous range of the tile list
// per XCD, workgroups strided inside it); per tile one LDS stage and two barriers.  The vertex
// ids of the next tile are fetched while the current tile's rows are evaluated.
//
// Plans with long rows (TFEM_RING_LONG=1: vertices with 8 .. 15 neighbours listed apart): the
// tile launch skips those rows and k_p1_apply_long_rows forms them, sixteen lanes per row as in
// k_p1_long_rows.
#include "tfem_rings_cols.hpp"
#include "tfem_rings_kernel.hpp"

namespace tfem {

template <typename T>
struct ApplyArgs {
  const T *u;  // NULL: y = diag(K)
  T *y;
  unsigned u_bytes, y_bytes;
};

template <typename T, int SLOTS, bool MASS, bool CHUNK, bool DIAG>
__global__ __launch_bounds__(kRingBlock) void k_p1_apply_rows(const RingArgs<T> a, const ApplyArgs<T> b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_smem[];
  T *xy = reinterpret_cast<T *>(ring_smem);  // [2 * lds_vert]
  T *us = xy + 2 * a.lds_vert;               // [lds_vert]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per = (a.n_tiles + 7) / 8;
  const int xcd = blockIdx.x & 7;
  const int stride = gridDim.x >> 3;
  const ring_rsrc_t r_coords = ring_rsrc(a.coords, a.coords_bytes);
  const ring_rsrc_t r_plan = ring_rsrc(a.plan, a.plan_bytes);
  const ring_rsrc_t r_u = ring_rsrc(b.u, b.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(b.y, b.y_bytes);
  constexpr unsigned kRecBytes = unsigned(4 * RingRec<SLOTS>::kWords);
  constexpr unsigned kNone = 0x3FFFFFFu;  // index behind every array: buffer loads give 0

  auto tile_at = [&](int j) { return (j < per && xcd * per + j < a.n_tiles) ? xcd * per + j : -1; };
  // vertex ids of a tile: the lane's own row and halo vertex number tid (as k_p1_rings)
  auto load_ids = [&](const RingDesc &d, unsigned &g_own, unsigned &g_halo) {
    const int r = d.row0 + lane;
    if (CHUNK)
      g_own = unsigned(d.gid0 + lane);
    else
      g_own = __builtin_amdgcn_raw_buffer_load_b32(
          r_plan, a.off_gid + (r < d.row1 ? unsigned(d.vert_off + r) : kNone) * 4u, 0, 0);
    const int h = d.n_own + tid;
    g_halo = __builtin_amdgcn_raw_buffer_load_b32(
        r_plan, a.off_gid + (h < d.n_vert ? unsigned(d.vert_off + h) : kNone) * 4u, 0, 0);
  };
  auto load_u = [&](unsigned g) {
    if constexpr (sizeof(T) == 8) {
      const ru32x2 v{__builtin_amdgcn_raw_buffer_load_b32(r_u, g * 8u, 0, 0),
                     __builtin_amdgcn_raw_buffer_load_b32(r_u, g * 8u + 4u, 0, 0)};
      return __builtin_bit_cast(double, v);
    } else {
      return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_u, g * 4u, 0, 0));
    }
  };

  int j = int(blockIdx.x >> 3);
  int t = tile_at(j);
  if (t < 0) return;  // whole workgroup, before any barrier
  RingDesc d = ring_desc<CHUNK>(a.plan, a.off_desc, t, wave);
  unsigned gid_own, gid_halo;
  load_ids(d, gid_own, gid_halo);
  for (;;) {
    const int r = d.row0 + lane;
    const bool own = r < d.row1;
    const int h = d.n_own + tid;
    const bool halo = h < d.n_vert;
    // coordinates and u of this tile's vertices, the row record
    T own_x, own_y, halo_x, halo_y, own_u = T(0), halo_u = T(0);
    ring_load_xy<T>(r_coords, own ? gid_own : kNone, own_x, own_y);
    ring_load_xy<T>(r_coords, halo ? gid_halo : kNone, halo_x, halo_y);
    if (!DIAG) {
      own_u = load_u(own ? gid_own : kNone);
      halo_u = load_u(halo ? gid_halo : kNone);
    }
    RingRec<SLOTS> rec;
    ring_load_rec<SLOTS>(r_plan, a.off_rows + (own ? unsigned(d.row_off + r) : kNone) * kRecBytes, rec);
    // vertex ids of the next tile, behind this tile's loads
    const unsigned gid_row = gid_own;
    const int t_n = tile_at(j + stride);
    RingDesc dn = d;
    if (t_n >= 0) {
      dn = ring_desc<CHUNK>(a.plan, a.off_desc, t_n, wave);
      load_ids(dn, gid_own, gid_halo);
    }
    if (own) {
      xy[2 * r] = own_x;
      xy[2 * r + 1] = own_y;
      if (!DIAG) us[r] = own_u;
    }
    if (halo) {
      xy[2 * h] = halo_x;
      xy[2 * h + 1] = halo_y;
      if (!DIAG) us[h] = halo_u;
    }
    __syncthreads();
    T off[SLOTS + 1], diag, sdets[SLOTS];
    const uint32_t lv = unsigned(own ? r : 0);
    ring_row<T, SLOTS, MASS, false>(a, rec, lv, xy, off, diag, sdets);
    const int k = rec.k();
    T yv = diag;
    if (!DIAG) {
      yv = diag * us[lv];
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        // off[i] for i >= k is scratch of ring_row: those slots take no part
        const T ui = us[i < k ? rec.id(i) : lv];
        yv = yv + (i < k ? off[i] : T(0)) * ui;
      }
    }
    // a long row (k = 0, bit 31 of the last record word) is written by k_p1_apply_long_rows
    const bool is_long = SLOTS == 7 && k == 0 && (rec.w[3] >> 31) != 0u;
    if (own && !is_long) {
      if constexpr (sizeof(T) == 8)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, yv), r_y, gid_row * 8u, 0, 0);
      else
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv), r_y, gid_row * 4u, 0, 0);
    }
    if (t_n < 0) break;
    __syncthreads();  // every row has read the stage before the next tile overwrites it
    j += stride;
    t = t_n;
    d = dn;
  }
}

// Rows of vertices with 8 .. 15 neighbours (plans with long rows): sixteen lanes per row
// (ring_long_slot); each slot lane multiplies its entry by u of its column, the products are
// summed over the sixteen lanes and lane 0 writes y_v.
template <typename T, bool MASS, bool DIAG>
__global__ __launch_bounds__(kRingBlock) void k_p1_apply_long_rows(const T *coords, const unsigned char *plan,
                                                                   unsigned off_long, int n_long, const T *u, T *y,
                                                                   T stiff_w, T mass_d, T mass_o) {
  RingLongSlot<T> s;
  ring_long_slot<T, MASS, !DIAG>(coords, plan, off_long, n_long, stiff_w, mass_o, u, s);
  if (!s.live || s.i != 0) return;
  const T diag = ring_diag<T, MASS>(s.sum, s.dsum, mass_d, mass_o);
  y[s.v] = DIAG ? diag : diag * u[s.v] + s.prod;
}

// ---------------------------------------------------------------------------------------
// Several vectors in one launch: Y = K U, U and Y (n_verts, n_vec) row-major.  The row record, the
// coordinates, ring_row and the chain loads -> barrier -> rows -> barrier of a tile are paid once
// for the NV columns of a pass; the lane then forms NV sums, each in the order of k_p1_apply_rows.
// The columns are staged with tfem_rings_cols.hpp (ApplyMultiArgs, apply_load_cols, apply_store_cols).
// ---------------------------------------------------------------------------------------
// k_p1_apply_rows for NV columns per pass.  LDS: the coordinates, then NV reals per local vertex
// (us[NV * lv + c]: a vertex's values are one 16-byte-aligned piece, read with the widest LDS loads).
template <typename T, int SLOTS, bool MASS, bool CHUNK, int NV>
__global__ __launch_bounds__(kRingBlock) void k_p1_apply_rows_multi(const RingArgs<T> a, const ApplyMultiArgs<T> b) {
  static_assert(NV >= 2 && NV % 2 == 0, "columns per pass come in pairs");
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_smem[];
  T *xy = reinterpret_cast<T *>(ring_smem);  // [2 * lds_vert]
  T *us = static_cast<T *>(__builtin_assume_aligned(xy + 2 * a.lds_vert, 16));  // [NV * lds_vert]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per = (a.n_tiles + 7) / 8;
  const int xcd = blockIdx.x & 7;
  const int stride = gridDim.x >> 3;
  const ring_rsrc_t r_coords = ring_rsrc(a.coords, a.coords_bytes);
  const ring_rsrc_t r_plan = ring_rsrc(a.plan, a.plan_bytes);
  const ring_rsrc_t r_u = ring_rsrc(b.u, b.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(b.y, b.y_bytes);
  constexpr unsigned kRecBytes = unsigned(4 * RingRec<SLOTS>::kWords);
  constexpr unsigned kNone = 0x3FFFFFFu;       // index behind every array: buffer loads give 0
  constexpr unsigned kNoByte = 0xFFFFFF00u;    // lanes without a vertex: their values are not staged
  const unsigned row_bytes = b.n_vec * unsigned(sizeof(T)), col_byte = b.col0 * unsigned(sizeof(T));

  auto tile_at = [&](int j) { return (j < per && xcd * per + j < a.n_tiles) ? xcd * per + j : -1; };
  auto load_ids = [&](const RingDesc &d, unsigned &g_own, unsigned &g_halo) {
    const int r = d.row0 + lane;
    if (CHUNK)
      g_own = unsigned(d.gid0 + lane);
    else
      g_own = __builtin_amdgcn_raw_buffer_load_b32(
          r_plan, a.off_gid + (r < d.row1 ? unsigned(d.vert_off + r) : kNone) * 4u, 0, 0);
    const int h = d.n_own + tid;
    g_halo = __builtin_amdgcn_raw_buffer_load_b32(
        r_plan, a.off_gid + (h < d.n_vert ? unsigned(d.vert_off + h) : kNone) * 4u, 0, 0);
  };

  int j = int(blockIdx.x >> 3);
  int t = tile_at(j);
  if (t < 0) return;  // whole workgroup, before any barrier
  RingDesc d = ring_desc<CHUNK>(a.plan, a.off_desc, t, wave);
  unsigned gid_own, gid_halo;
  load_ids(d, gid_own, gid_halo);
  for (;;) {
    const int r = d.row0 + lane;
    const bool own = r < d.row1;
    const int h = d.n_own + tid;
    const bool halo = h < d.n_vert;
    T own_x, own_y, halo_x, halo_y, own_u[NV], halo_u[NV];
    ring_load_xy<T>(r_coords, own ? gid_own : kNone, own_x, own_y);
    ring_load_xy<T>(r_coords, halo ? gid_halo : kNone, halo_x, halo_y);
    apply_load_cols<T, NV>(r_u, own ? gid_own * row_bytes + col_byte : kNoByte, own_u);
    apply_load_cols<T, NV>(r_u, halo ? gid_halo * row_bytes + col_byte : kNoByte, halo_u);
    RingRec<SLOTS> rec;
    ring_load_rec<SLOTS>(r_plan, a.off_rows + (own ? unsigned(d.row_off + r) : kNone) * kRecBytes, rec);
    // vertex ids of the next tile, behind this tile's loads
    const unsigned gid_row = gid_own;
    const int t_n = tile_at(j + stride);
    RingDesc dn = d;
    if (t_n >= 0) {
      dn = ring_desc<CHUNK>(a.plan, a.off_desc, t_n, wave);
      load_ids(dn, gid_own, gid_halo);
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
    __syncthreads();
    T off[SLOTS + 1], diag, sdets[SLOTS];
    const uint32_t lv = unsigned(own ? r : 0);
    ring_row<T, SLOTS, MASS, false>(a, rec, lv, xy, off, diag, sdets);
    const int k = rec.k();
    T yv[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) yv[c] = diag * us[NV * lv + c];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      // off[i] for i >= k is scratch of ring_row: those slots take no part
      const T *ui = us + NV * (i < k ? rec.id(i) : lv);
      const T w = i < k ? off[i] : T(0);
#pragma unroll
      for (int c = 0; c < NV; ++c) yv[c] = yv[c] + w * ui[c];
    }
    // a long row (k = 0, bit 31 of the last record word) is written by k_p1_apply_long_rows_multi
    const bool is_long = SLOTS == 7 && k == 0 && (rec.w[3] >> 31) != 0u;
    if (own && !is_long) apply_store_cols<T, NV>(r_y, gid_row * row_bytes + col_byte, yv, b.n_col);
    if (t_n < 0) break;
    __syncthreads();  // every row has read the stage before the next tile overwrites it
    j += stride;
    t = t_n;
    d = dn;
  }
}

// k_p1_apply_long_rows for n_vec columns: the sixteen lanes of a row evaluate their entries once,
// then every column is one product per slot lane and one sum over the sixteen lanes.
template <typename T, bool MASS>
__global__ __launch_bounds__(kRingBlock) void k_p1_apply_long_rows_multi(const T *coords, const unsigned char *plan,
                                                                         unsigned off_long, int n_long, const T *u,
                                                                         T *y, unsigned n_vec, T stiff_w, T mass_d,
                                                                         T mass_o) {
  RingLongSlot<T> s;
  ring_long_slot<T, MASS, false>(coords, plan, off_long, n_long, stiff_w, mass_o, u, s);
  const T diag = ring_diag<T, MASS>(s.sum, s.dsum, mass_d, mass_o);
  const size_t col = size_t(s.rec[4 + (s.slot ? s.i : 0)]) * n_vec, row = size_t(s.v) * n_vec;
  for (unsigned c = 0; c < n_vec; ++c) {  // uniform: every lane takes part in the sums
    T prod = s.slot ? s.entry * u[col + c] : T(0);
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) prod = prod + __shfl_xor(prod, m, 64);
    if (s.live && s.i == 0) y[row + c] = diag * u[row + c] + prod;
  }
}

template <typename T, int SLOTS, bool CHUNK, int NV>
static void *pick_apply_multi_mass(bool mass) {
  return mass ? reinterpret_cast<void *>(k_p1_apply_rows_multi<T, SLOTS, true, CHUNK, NV>)
              : reinterpret_cast<void *>(k_p1_apply_rows_multi<T, SLOTS, false, CHUNK, NV>);
}

// 15-slot records are built up to kApplyWide15 columns: with eight, the double instances hold
// sixteen entries and eight sums per lane in more than 256 registers (one wave per SIMD).
constexpr int kApplyWide15 = 4;

template <typename T, int NV>
static void *pick_apply_multi_kernel(int slots, bool chunk, bool mass) {
  if (slots == 7)
    return chunk ? pick_apply_multi_mass<T, 7, true, NV>(mass) : pick_apply_multi_mass<T, 7, false, NV>(mass);
  if constexpr (NV <= kApplyWide15)
    return chunk ? pick_apply_multi_mass<T, 15, true, NV>(mass) : pick_apply_multi_mass<T, 15, false, NV>(mass);
  return nullptr;
}

template <typename T, int SLOTS, bool CHUNK>
static void *pick_apply_diag(bool mass, bool diag) {
  if (mass)
    return diag ? reinterpret_cast<void *>(k_p1_apply_rows<T, SLOTS, true, CHUNK, true>)
                : reinterpret_cast<void *>(k_p1_apply_rows<T, SLOTS, true, CHUNK, false>);
  return diag ? reinterpret_cast<void *>(k_p1_apply_rows<T, SLOTS, false, CHUNK, true>)
              : reinterpret_cast<void *>(k_p1_apply_rows<T, SLOTS, false, CHUNK, false>);
}

template <typename T>
static void *pick_apply_kernel(int slots, bool chunk, bool mass, bool diag) {
  if (slots == 7)
    return chunk ? pick_apply_diag<T, 7, true>(mass, diag) : pick_apply_diag<T, 7, false>(mass, diag);
  return chunk ? pick_apply_diag<T, 15, true>(mass, diag) : pick_apply_diag<T, 15, false>(mass, diag);
}

template <typename T>
static int launch_apply(const void *coords, int64_t n_verts, int quad_order, double alpha, double beta,
                        const unsigned char *plan, const int64_t *z, const void *u, void *y, hipStream_t stream) {
  TriTables tables;
  if (!build_tri_tables(quad_order, int(sizeof(T)), &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if (z[0] == 0) return TFEM_OK;
  if (!coords || !plan || !y) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  RingArgs<T> a;
  int st = ring_args_init<T>(tables, z, coords, plan, n_verts, alpha, beta, a);
  if (st != TFEM_OK) return st;
  const int64_t vec_bytes = n_verts * int64_t(sizeof(T));
  st = check_extents("ring kernel", &vec_bytes, 1);
  if (st != TFEM_OK) return st;
  ApplyArgs<T> b;
  b.u = static_cast<const T *>(u);
  b.y = static_cast<T *>(y);
  b.u_bytes = u ? unsigned(vec_bytes) : 0u;
  b.y_bytes = unsigned(vec_bytes);
  const bool mass = beta != 0.0, diag = u == nullptr, chunk = z[13] != 0;
  const int slots = int(z[6]);
  void *kernel = pick_apply_kernel<T>(slots, chunk, mass, diag);
  const size_t lds = size_t(3 * a.lds_vert) * sizeof(T);
  int per_cu = 0;
  st = resident_per_cu(kernel, kRingBlock, lds, &per_cu);
  if (st != TFEM_OK) return st;
  const int per = int((z[0] + 7) / 8);
  const int blocks = std::min(per * 8, (device_cu_count() * per_cu / 8) * 8);
  void *params[] = {&a, &b};
  hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(std::max(blocks, 8))), dim3(kRingBlock), params, lds, stream);
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "apply kernel launch: %s", hipGetErrorString(e));
  if (z[23] > 0) {  // the rows of the vertices with 8 .. 15 neighbours
    const dim3 lgrid{unsigned((16 * z[23] + kRingBlock - 1) / kRingBlock)};
    void *long_kernel = mass ? (diag ? reinterpret_cast<void *>(k_p1_apply_long_rows<T, true, true>)
                                     : reinterpret_cast<void *>(k_p1_apply_long_rows<T, true, false>))
                             : (diag ? reinterpret_cast<void *>(k_p1_apply_long_rows<T, false, true>)
                                     : reinterpret_cast<void *>(k_p1_apply_long_rows<T, false, false>));
    unsigned off_long = unsigned(z[22]);
    int n_long = int(z[23]);
    void *long_params[] = {&a.coords, &a.plan, &off_long, &n_long, &b.u, &b.y, &a.stiff_w, &a.mass_d, &a.mass_o};
    e = hipLaunchKernel(long_kernel, lgrid, dim3(kRingBlock), long_params, 0, stream);
    if (e != hipSuccess) return fail(TFEM_ERR_HIP, "long-row apply launch: %s", hipGetErrorString(e));
  }
  return TFEM_OK;
}

// Widths of k_p1_apply_rows_multi that are built (DESIGN.md section 3 says why these).
constexpr int kApplyWidths[] = {2, 4, 8};

template <typename T>
static void *pick_apply_multi(int nv, int slots, bool chunk, bool mass) {
  switch (nv) {
    case 2: return pick_apply_multi_kernel<T, 2>(slots, chunk, mass);
    case 4: return pick_apply_multi_kernel<T, 4>(slots, chunk, mass);
    default: return pick_apply_multi_kernel<T, 8>(slots, chunk, mass);
  }
}

// Y = K U for n_vec >= 2 columns: passes of the widest width whose stage fits 64 KB of LDS (no
// function attribute is set in the launch path); the last pass takes the narrowest width that
// holds what is left.  TFEM_APPLY_NV caps the width (timing of the widths against each other).
template <typename T>
static int launch_apply_multi(const void *coords, int64_t n_verts, int quad_order, double alpha, double beta,
                              const unsigned char *plan, const int64_t *z, const void *u, void *y, int64_t n_vec,
                              hipStream_t stream) {
  TriTables tables;
  if (!build_tri_tables(quad_order, int(sizeof(T)), &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if (z[0] == 0) return TFEM_OK;
  if (!coords || !plan || !y) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  RingArgs<T> a;
  int st = ring_args_init<T>(tables, z, coords, plan, n_verts, alpha, beta, a);
  if (st != TFEM_OK) return st;
  ApplyMultiArgs<T> b;
  b.u = static_cast<const T *>(u);
  b.y = static_cast<T *>(y);
  b.u_bytes = b.y_bytes = unsigned(n_verts * n_vec * int64_t(sizeof(T)));
  b.n_vec = unsigned(n_vec);
  const int slots = int(z[6]);
  int cap = 0;
  if (const char *env = std::getenv("TFEM_APPLY_NV")) cap = std::atoi(env);
  int widest = 0;
  for (int w : kApplyWidths)
    if (size_t(2 + w) * size_t(a.lds_vert) * sizeof(T) <= size_t(64) * 1024 && (cap < 2 || w <= cap) &&
        (slots == 7 || w <= kApplyWide15))
      widest = w;
  if (widest == 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "ring plan exceeds the kernel's capacities");
  const bool mass = beta != 0.0, chunk = z[13] != 0;
  const int per = int((z[0] + 7) / 8);
  for (int64_t col0 = 0; col0 < n_vec;) {
    const int64_t left = n_vec - col0;
    int nv = widest;
    for (int w : kApplyWidths)
      if (w >= left && w < nv) nv = w;
    b.col0 = unsigned(col0);
    b.n_col = unsigned(std::min<int64_t>(left, nv));
    void *kernel = pick_apply_multi<T>(nv, slots, chunk, mass);
    const size_t lds = size_t(2 + nv) * size_t(a.lds_vert) * sizeof(T);
    int per_cu = 0;
    st = resident_per_cu(kernel, kRingBlock, lds, &per_cu);
    if (st != TFEM_OK) return st;
    const int blocks = std::min(per * 8, (device_cu_count() * per_cu / 8) * 8);
    void *params[] = {&a, &b};
    hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(std::max(blocks, 8))), dim3(kRingBlock), params, lds, stream);
    if (e != hipSuccess) return fail(TFEM_ERR_HIP, "apply kernel launch: %s", hipGetErrorString(e));
    col0 += b.n_col;
  }
  if (z[23] > 0) {  // the rows of the vertices with 8 .. 15 neighbours, every column in one launch
    const dim3 lgrid{unsigned((16 * z[23] + kRingBlock - 1) / kRingBlock)};
    void *long_kernel = mass ? reinterpret_cast<void *>(k_p1_apply_long_rows_multi<T, true>)
                             : reinterpret_cast<void *>(k_p1_apply_long_rows_multi<T, false>);
    unsigned off_long = unsigned(z[22]);
    int n_long = int(z[23]);
    void *long_params[] = {&a.coords, &a.plan, &off_long, &n_long, &b.u, &b.y, &b.n_vec, &a.stiff_w, &a.mass_d, &a.mass_o};
    hipError_t e = hipLaunchKernel(long_kernel, lgrid, dim3(kRingBlock), long_params, 0, stream);
    if (e != hipSuccess) return fail(TFEM_ERR_HIP, "long-row apply launch: %s", hipGetErrorString(e));
  }
  return TFEM_OK;
}

}  // namespace tfem

extern "C" {

int tfem_p1_apply_rings(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha,
                        double beta, const void *plan_device, const int64_t *plan_layout_host, const void *u,
                        void *y, void *stream) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (n_verts < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  const unsigned char *plan = static_cast<const unsigned char *>(plan_device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8 ? launch_apply<double>(coords, n_verts, quad_order, alpha, beta, plan, plan_layout_host, u, y, s)
                         : launch_apply<float>(coords, n_verts, quad_order, alpha, beta, plan, plan_layout_host, u, y, s);
}

int tfem_p1_apply_rings_multi(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha,
                              double beta, const void *plan_device, const int64_t *plan_layout_host, const void *u,
                              void *y, int64_t n_vec, void *stream) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (n_verts < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  if (n_vec < 1) return fail(TFEM_ERR_INVALID_ARGUMENT, "n_vec must be at least 1");
  if (!u) return fail(TFEM_ERR_INVALID_ARGUMENT, "u is NULL (the diagonal: tfem_p1_apply_rings)");
  // the extent of u and y, before anything is derived from it
  const int64_t limit = int64_t(1) << 32;
  const int64_t vec_bytes = (n_verts > 0 && n_vec >= limit / n_verts) ? limit : n_verts * n_vec * real_bytes;
  int st = check_extents("ring kernel", &vec_bytes, 1);
  if (st != TFEM_OK) return st;
  const char *ub = static_cast<const char *>(u), *yb = static_cast<const char *>(y);
  if (y && ub < yb + vec_bytes && yb < ub + vec_bytes) return fail(TFEM_ERR_INVALID_ARGUMENT, "u and y overlap");
  const unsigned char *plan = static_cast<const unsigned char *>(plan_device);
  const int64_t *z = plan_layout_host;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_vec == 1)  // one column: the single-vector launch, same layout
    return tfem_p1_apply_rings(coords, real_bytes, n_verts, quad_order, alpha, beta, plan_device, z, u, y, stream);
  return real_bytes == 8 ? launch_apply_multi<double>(coords, n_verts, quad_order, alpha, beta, plan, z, u, y, n_vec, s)
                         : launch_apply_multi<float>(coords, n_verts, quad_order, alpha, beta, plan, z, u, y, n_vec, s);
}

}  // extern "C"
