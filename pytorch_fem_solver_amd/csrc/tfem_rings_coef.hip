// Variable-coefficient P1 forms over a ring plan:
//     K = alpha * int kappa(x, y) grad u . grad v  +  beta * int c(x, y) u v
// (abstract_basis.py:74-93 with a coefficient in front of basis.py:64-85's integrands), assembled
// into the CSR values or applied matrix-free, with kappa and c given as source programs
// (tfem_source.hpp) that the launch evaluates at the integration points itself.  The reference
// (and this package's torch path) builds the (E, Q, 3, 3) integrand for such a form -- 72 Q bytes per
// element written and read again; here nothing per element exists in memory.
//
// For P1 the gradients are constant on an element, so the coefficient changes ONE number per
// triangle of a row's fan: its weight is alpha * sum_q (w_q / 2) kappa(x_q) where ring_row
// (tfem_rings_kernel.hpp) uses the constant RingArgs::stiff_w.  Rows of the stiffness part still sum
// to zero, so the diagonal is minus the sum of the off-diagonal stiffness entries.  The mass part
// needs, per triangle and seen from the row's vertex v (local vertex 0; n_i = 1, n_next = 2), the
// sums  sum_q (w_q / 2) c(x_q) l_0 l_0,  ... l_0 l_1,  ... l_0 l_2  times the signed determinant.
//
// ring_row_coef walks the fan like ring_row, but slot by slot in a loop that is NOT unrolled (one
// copy of the interpreter per kernel): all lanes of the wave run slot i together, the program's
// control flow stays wave-uniform.  Lanes whose slot carries flag 0 (no triangle) evaluate the
// programs at their own vertex and discard the values.  The record's fields are popped from shift
// registers and a finished entry is handed out per slot (K[v][n_i] = this triangle's share + the
// previous triangle's share), so no register array is indexed by the loop counter -- no kernel here
// uses scratch memory.  The loop runs to the largest fan of the wave.
//
// The row's vertex is local vertex 0 of every triangle AS THE ROW SEES IT, so the rule's points are
// visited in an order that depends on the row.  The symmetric rules of element_tri.py:77-130 are
// permutation-invariant as sets: K_ij and K_ji agree to rounding, not bit for bit.
//
// Every element's coefficient is evaluated once per row that touches it (three times per element,
// plus the dead slots below the wave's largest fan).  That is the price of needing no plan data
// beyond what k_p1_apply_rows reads.
//
// k_p1_coef_rows: the tile walk of k_p1_apply_rows (tfem_rings_apply.hip); MODE = apply (y = K u),
// diag (y = diag K) or store (the row's CSR values, staged per wave and streamed out with the store
// helpers of the matrix-only ring launch).  Plans with long rows (layout[23] > 0) are refused:
// such a form takes the generic path.  ring_row_coef and the launch arguments are in
// tfem_rings_coef.hpp; K U for a block of vectors is k_p1_coef_rows_multi (tfem_rings_coef_multi.hip).
//
// Built with the interpreter's flags (see tfem_rings_src.hip).
#include "tfem_rings_coef.hpp"

namespace tfem {

constexpr int kCoefApply = 0, kCoefDiag = 1, kCoefStore = 2;

template <typename T, int SLOTS, bool MASS, bool CHUNK, int QL, int MODE>
__global__ __launch_bounds__(kRingBlock) void k_p1_coef_rows(const CoefLaunch<T> L) {
  const RingArgs<T> &a = L.a;
  const CoefArgs<T> &b = L.b;
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_smem[];
  T *xy = reinterpret_cast<T *>(ring_smem);  // [2 * lds_vert]
  T *us = xy + 2 * a.lds_vert;               // [lds_vert] (apply only)
  T *stage = xy + 2 * a.lds_vert;            // [waves][stage entries] (store only)
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
  constexpr unsigned kRecBytes = unsigned(4 * RingRec<SLOTS>::kWords);
  constexpr unsigned kNone = 0x3FFFFFFu;  // index behind every array: buffer loads give 0
  constexpr int kSpare = 64 * (SLOTS + 1);  // the stage's spare entries (ring_stage_entries)

  // the programs, one operation per lane, for the whole launch
  const SrcLanes<T> pk = src_load_lanes<T>(src_in_kernarg<T>(__builtin_offsetof(CoefLaunch<T>, b.kappa)));
  const SrcLanes<T> pc = src_load_lanes<T>(src_in_kernarg<T>(__builtin_offsetof(CoefLaunch<T>, b.c)));

  auto tile_at = [&](int j) { return (j < per && xcd * per + j < a.n_tiles) ? xcd * per + j : -1; };
  // vertex ids of a tile: the lane's own row and halo vertex number tid (as k_p1_apply_rows)
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
    if (MODE == kCoefApply) {
      own_u = load_u(own ? gid_own : kNone);
      halo_u = load_u(halo ? gid_halo : kNone);
    }
    const unsigned row = own ? unsigned(d.row_off + r) : kNone;
    RingRec<SLOTS> rec;
    ring_load_rec<SLOTS>(r_plan, a.off_rows + row * kRecBytes, rec);
    int rowstart = 0;
    if (MODE == kCoefStore && !CHUNK)
      rowstart = int(__builtin_amdgcn_raw_buffer_load_b32(r_plan, a.off_rowstart + row * 4u, 0, 0));
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
      if (MODE == kCoefApply) us[r] = own_u;
    }
    if (halo) {
      xy[2 * h] = halo_x;
      xy[2 * h + 1] = halo_y;
      if (MODE == kCoefApply) us[h] = halo_u;
    }
    __syncthreads();
    const uint32_t lv = unsigned(own ? r : 0);
    const int k = rec.k();
    int kmax = 0;  // the largest fan of the wave
#pragma unroll
    for (int i = 1; i <= SLOTS; ++i) kmax = __builtin_amdgcn_ballot_w64(k >= i) != 0ull ? i : kmax;
    T diag, yv = T(0);
    int total = 0, pre = 0;
    const int len = k > 0 ? k + 1 : 0;
    if (MODE == kCoefStore) {  // the wave's stage, compact and in CSR order (ring_stage)
      const int incl = wave_inclusive_scan(len);
      pre = incl - len;
      total = __builtin_amdgcn_readlane(incl, 63);
    }
    ring_row_coef<T, SLOTS, MASS, QL>(a, b, pk, pc, rec, lv, xy, kmax, diag,
                                      [&](bool live, uint32_t id, int pos, T value) {
                                        if (MODE == kCoefApply) yv = yv + (live ? value : T(0)) * us[live ? id : lv];
                                        if (MODE == kCoefStore) my_stage[live ? pre + pos : kSpare] = value;
                                      });
    if (MODE == kCoefStore) {
      my_stage[k > 0 ? pre + rec.dpos() : kSpare] = diag;
      if (CHUNK) {  // one run per wave by construction, its CSR offset in the descriptor
        __builtin_amdgcn_wave_barrier();
        ring_store_run1<T, SLOTS>(my_stage, total, d.rs0, r_vals, a.plain_stores);
        __builtin_amdgcn_wave_barrier();
      } else {
        ring_store<T, SLOTS>(my_stage, total, pre, rowstart, len, r_vals, a.plain_stores);
      }
    } else {
      yv = MODE == kCoefDiag ? diag : yv + diag * us[lv];
      if (own) {
        if constexpr (sizeof(T) == 8)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, yv), r_y, gid_row * 8u, 0, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv), r_y, gid_row * 4u, 0, 0);
      }
    }
    if (t_n < 0) break;
    __syncthreads();  // every row has read the stage before the next tile overwrites it
    j += stride;
    t = t_n;
    d = dn;
  }
}

template <typename T, int SLOTS, bool MASS, bool CHUNK, int QL>
static void *pick_coef_mode(int mode) {
  switch (mode) {
    case kCoefApply: return reinterpret_cast<void *>(k_p1_coef_rows<T, SLOTS, MASS, CHUNK, QL, kCoefApply>);
    case kCoefDiag: return reinterpret_cast<void *>(k_p1_coef_rows<T, SLOTS, MASS, CHUNK, QL, kCoefDiag>);
    default: return reinterpret_cast<void *>(k_p1_coef_rows<T, SLOTS, MASS, CHUNK, QL, kCoefStore>);
  }
}

template <typename T, int SLOTS, bool MASS, bool CHUNK>
static void *pick_coef_q(int nq, int mode) {
  switch (nq) {
    case 1: return pick_coef_mode<T, SLOTS, MASS, CHUNK, 1>(mode);
    case 3: return pick_coef_mode<T, SLOTS, MASS, CHUNK, 3>(mode);
    case 4: return pick_coef_mode<T, SLOTS, MASS, CHUNK, 4>(mode);
    case 6: return pick_coef_mode<T, SLOTS, MASS, CHUNK, 6>(mode);
    default: return nullptr;
  }
}

template <typename T, int SLOTS>
static void *pick_coef_chunk(bool mass, bool chunk, int nq, int mode) {
  if (mass)
    return chunk ? pick_coef_q<T, SLOTS, true, true>(nq, mode) : pick_coef_q<T, SLOTS, true, false>(nq, mode);
  return chunk ? pick_coef_q<T, SLOTS, false, true>(nq, mode) : pick_coef_q<T, SLOTS, false, false>(nq, mode);
}

template <typename T>
static int launch_coef(const void *coords, int64_t n_verts, int quad_order, double alpha, double beta,
                       const tfem_source_program *kappa, const tfem_source_program *c, const unsigned char *plan,
                       const int64_t *z, int mode, void *vals, const void *u, void *y, hipStream_t stream) {
  TriTables tables;
  if (!build_tri_tables(quad_order, int(sizeof(T)), &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  // both programs are checked before anything else is (tfem_source_validate's rules)
  if (kappa && src_validate(kappa) != TFEM_OK) return TFEM_ERR_INVALID_ARGUMENT;
  if (c && src_validate(c) != TFEM_OK) return TFEM_ERR_INVALID_ARGUMENT;
  if (z[0] == 0 || n_verts == 0) return TFEM_OK;
  if (!coords || !plan || !(mode == kCoefStore ? vals : y)) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  if (z[23] > 0)
    return fail(TFEM_ERR_UNSUPPORTED, "a ring plan with long rows does not take coefficient programs");
  CoefLaunch<T> K;
  int st = coef_launch_init<T>(tables, coords, n_verts, alpha, beta, kappa, c, plan, z, K);
  if (st != TFEM_OK) return st;
  RingArgs<T> &a = K.a;
  CoefArgs<T> &b = K.b;
  // the CSR values: neither the entry point nor the plan's layout carries nnz, so the extent of the
  // value stores is the upper bound rows x longest row (layout[5]) -- the hardware bounds check of
  // the other ring launches' value stores guards less here, and the 32-bit offset limit is reached
  // earlier than nnz itself would (the engine sends such a form to the generic path)
  const int64_t out_bytes[2] = {n_verts * int64_t(sizeof(T)),
                                mode == kCoefStore ? z[1] * z[5] * int64_t(sizeof(T)) : 0};
  st = check_extents("ring kernel", out_bytes, 2);
  if (st != TFEM_OK) return st;
  b.u = static_cast<const T *>(u);
  b.y = static_cast<T *>(y);
  b.u_bytes = mode == kCoefApply ? unsigned(out_bytes[0]) : 0u;
  b.y_bytes = mode == kCoefStore ? 0u : unsigned(out_bytes[0]);
  a.vals = static_cast<T *>(vals);
  a.vals_bytes = mode == kCoefStore ? unsigned(out_bytes[1]) : 0u;
  a.plain_stores = 1;  // the matrix alone: the store policy of the matrix-only ring launch
  const bool mass = beta != 0.0, chunk = z[13] != 0;
  const int slots = int(z[6]);
  void *kernel = slots == 7 ? pick_coef_chunk<T, 7>(mass, chunk, tables.nq, mode)
                            : pick_coef_chunk<T, 15>(mass, chunk, tables.nq, mode);
  if (!kernel) return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  const size_t lds = size_t((mode == kCoefApply ? 3 : 2) * a.lds_vert) * sizeof(T) +
                     (mode == kCoefStore ? size_t(kRingWaves) * size_t(64 * (slots + 1) + 2) * sizeof(T) : 0);
  int per_cu = 0;
  st = resident_per_cu(kernel, kRingBlock, lds, &per_cu);
  if (st != TFEM_OK) return st;
  const int per = int((z[0] + 7) / 8);
  const int blocks = std::min(per * 8, (device_cu_count() * per_cu / 8) * 8);
  void *params[] = {&K};
  hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(std::max(blocks, 8))), dim3(kRingBlock), params, lds, stream);
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "coefficient kernel launch: %s", hipGetErrorString(e));
  return TFEM_OK;
}

static int coef_entry(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha, double beta,
                      const tfem_source_program *kappa, const tfem_source_program *c, const void *plan_device,
                      const int64_t *plan_layout_host, int mode, void *vals, const void *u, void *y, void *stream) {
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (n_verts < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  if (!kappa && !c)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "no coefficient program: constant coefficients take "
                "tfem_p1_assemble_rings / tfem_p1_apply_rings");
  const unsigned char *plan = static_cast<const unsigned char *>(plan_device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8 ? launch_coef<double>(coords, n_verts, quad_order, alpha, beta, kappa, c, plan,
                                               plan_layout_host, mode, vals, u, y, s)
                         : launch_coef<float>(coords, n_verts, quad_order, alpha, beta, kappa, c, plan,
                                              plan_layout_host, mode, vals, u, y, s);
}

}  // namespace tfem

extern "C" {

int tfem_p1_rings_coef(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha, double beta,
                       const tfem_source_program *kappa, const tfem_source_program *c, const void *plan_device,
                       const int64_t *plan_layout_host, void *vals, void *stream) {
  return tfem::coef_entry(coords, real_bytes, n_verts, quad_order, alpha, beta, kappa, c, plan_device,
                          plan_layout_host, tfem::kCoefStore, vals, nullptr, nullptr, stream);
}

int tfem_p1_apply_rings_coef(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha,
                             double beta, const tfem_source_program *kappa, const tfem_source_program *c,
                             const void *plan_device, const int64_t *plan_layout_host, const void *u, void *y,
                             void *stream) {
  return tfem::coef_entry(coords, real_bytes, n_verts, quad_order, alpha, beta, kappa, c, plan_device,
                          plan_layout_host, u ? tfem::kCoefApply : tfem::kCoefDiag, nullptr, u, y, stream);
}

}  // extern "C"
