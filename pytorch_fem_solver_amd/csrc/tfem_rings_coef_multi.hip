// Variable-coefficient P1 operator on several vectors in one launch: Y = K U for
//     K = alpha * int kappa(x, y) grad u . grad v  +  beta * int c(x, y) u v
// over a ring plan, U and Y (n_verts, n_vec) row-major.
//
// k_p1_coef_rows (tfem_rings_coef.hip) spends nearly all of its instructions in the coefficient
// programs, interpreted once per row and triangle -- and none of that depends on the vector.
// k_p1_coef_rows_multi is its apply mode with the column staging of k_p1_apply_rows_multi
// (tfem_rings_apply.hip, tfem_rings_cols.hpp): ring_row_coef walks a row's fan ONCE per pass and
// every finished entry is multiplied by NV staged columns, so the interpreter is paid once for NV
// columns; a column costs one LDS read and one multiply-add per entry.
//
// Every column's sum is formed in the order and with the operations of k_p1_coef_rows:
//     yv = 0;  per emitted slot  yv = yv + (live ? value : 0) * us[live ? id : lv];  yv = yv + diag * us[lv]
// -- the build does not contract, so column j of Y is bit for bit tfem_p1_apply_rings_coef on column
// j of U.
//
// Tile walk, LDS stage (coordinates, then NV reals per local vertex) and the two barriers per tile:
// as k_p1_apply_rows_multi.  The NV sums are the only values that live across ring_row_coef's slot
// loop besides its own; no array is indexed by that loop's counter (no scratch memory).
//
// Built with the interpreter's flags (see tfem_rings_src.hip).
#include "tfem_rings_coef.hpp"
#include "tfem_rings_cols.hpp"

namespace tfem {

template <typename T>
struct CoefMultiLaunch {  // the kernel's only parameter (src_in_kernarg addresses the programs in it)
  CoefLaunch<T> k;        // k.b.u / k.b.y are not used: the vectors are m's
  ApplyMultiArgs<T> m;
};

template <typename T, int SLOTS, bool MASS, bool CHUNK, int QL, int NV>
__global__ __launch_bounds__(kRingBlock) void k_p1_coef_rows_multi(const CoefMultiLaunch<T> L) {
  static_assert(NV >= 2 && NV % 2 == 0, "columns per pass come in pairs");
  const RingArgs<T> &a = L.k.a;
  const CoefArgs<T> &b = L.k.b;
  const ApplyMultiArgs<T> &m = L.m;
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
  const ring_rsrc_t r_u = ring_rsrc(m.u, m.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(m.y, m.y_bytes);
  constexpr unsigned kRecBytes = unsigned(4 * RingRec<SLOTS>::kWords);
  constexpr unsigned kNone = 0x3FFFFFFu;     // index behind every array: buffer loads give 0
  constexpr unsigned kNoByte = 0xFFFFFF00u;  // lanes without a vertex: their values are not staged
  const unsigned row_bytes = m.n_vec * unsigned(sizeof(T)), col_byte = m.col0 * unsigned(sizeof(T));

  // the programs, one operation per lane, for the whole launch
  const SrcLanes<T> pk = src_load_lanes<T>(src_in_kernarg<T>(__builtin_offsetof(CoefMultiLaunch<T>, k.b.kappa)));
  const SrcLanes<T> pc = src_load_lanes<T>(src_in_kernarg<T>(__builtin_offsetof(CoefMultiLaunch<T>, k.b.c)));

  auto tile_at = [&](int j) { return (j < per && xcd * per + j < a.n_tiles) ? xcd * per + j : -1; };
  // vertex ids of a tile: the lane's own row and halo vertex number tid (as k_p1_coef_rows)
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
    // coordinates and the NV columns of this tile's vertices, the row record
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
    const uint32_t lv = unsigned(own ? r : 0);
    const int k = rec.k();
    int kmax = 0;  // the largest fan of the wave
#pragma unroll
    for (int i = 1; i <= SLOTS; ++i) kmax = __builtin_amdgcn_ballot_w64(k >= i) != 0ull ? i : kmax;
    T diag, yv[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) yv[c] = T(0);
    ring_row_coef<T, SLOTS, MASS, QL>(a, b, pk, pc, rec, lv, xy, kmax, diag,
                                      [&](bool live, uint32_t id, int, T value) {
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
    __syncthreads();  // every row has read the stage before the next tile overwrites it
    j += stride;
    t = t_n;
    d = dn;
  }
}

template <typename T, int SLOTS, bool MASS, bool CHUNK, int NV>
static void *pick_coef_multi_q(int nq) {
  switch (nq) {
    case 1: return reinterpret_cast<void *>(k_p1_coef_rows_multi<T, SLOTS, MASS, CHUNK, 1, NV>);
    case 3: return reinterpret_cast<void *>(k_p1_coef_rows_multi<T, SLOTS, MASS, CHUNK, 3, NV>);
    case 4: return reinterpret_cast<void *>(k_p1_coef_rows_multi<T, SLOTS, MASS, CHUNK, 4, NV>);
    case 6: return reinterpret_cast<void *>(k_p1_coef_rows_multi<T, SLOTS, MASS, CHUNK, 6, NV>);
    default: return nullptr;
  }
}

template <typename T, int SLOTS, int NV>
static void *pick_coef_multi_chunk(bool mass, bool chunk, int nq) {
  if (mass)
    return chunk ? pick_coef_multi_q<T, SLOTS, true, true, NV>(nq) : pick_coef_multi_q<T, SLOTS, true, false, NV>(nq);
  return chunk ? pick_coef_multi_q<T, SLOTS, false, true, NV>(nq) : pick_coef_multi_q<T, SLOTS, false, false, NV>(nq);
}

// Widths of k_p1_coef_rows_multi that are built (DESIGN.md section 3 says why these); 15-slot
// records up to kCoefWide15 columns, as k_p1_apply_rows_multi.
constexpr int kCoefWidths[] = {2, 4, 8};
constexpr int kCoefWide15 = 4;

template <typename T>
static void *pick_coef_multi(int nv, int slots, bool mass, bool chunk, int nq) {
  if (slots == 7) {
    switch (nv) {
      case 2: return pick_coef_multi_chunk<T, 7, 2>(mass, chunk, nq);
      case 4: return pick_coef_multi_chunk<T, 7, 4>(mass, chunk, nq);
      default: return pick_coef_multi_chunk<T, 7, 8>(mass, chunk, nq);
    }
  }
  return nv == 2 ? pick_coef_multi_chunk<T, 15, 2>(mass, chunk, nq) : pick_coef_multi_chunk<T, 15, 4>(mass, chunk, nq);
}

// Y = K U for n_vec >= 2 columns: the passes of launch_apply_multi (the widest built width whose
// stage fits 64 KB of LDS -- no function attribute is set --, the narrowest that holds the rest
// for the last pass, TFEM_APPLY_NV as a cap) with the grid of launch_coef.  The entry point has
// checked the sizes, the pointers of u and y, the programs, the long rows and the order.
template <typename T>
static int launch_coef_multi(const TriTables &tables, const void *coords, int64_t n_verts, double alpha, double beta,
                             const tfem_source_program *kappa, const tfem_source_program *c,
                             const unsigned char *plan, const int64_t *z, const void *u, void *y, int64_t n_vec,
                             hipStream_t stream) {
  if (!coords || !plan || !y) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  CoefMultiLaunch<T> K;
  int st = coef_launch_init<T>(tables, coords, n_verts, alpha, beta, kappa, c, plan, z, K.k);
  if (st != TFEM_OK) return st;
  const RingArgs<T> &a = K.k.a;
  ApplyMultiArgs<T> &m = K.m;
  m.u = static_cast<const T *>(u);
  m.y = static_cast<T *>(y);
  m.u_bytes = m.y_bytes = unsigned(n_verts * n_vec * int64_t(sizeof(T)));
  m.n_vec = unsigned(n_vec);
  const int slots = int(z[6]);
  int cap = 0;
  if (const char *env = std::getenv("TFEM_APPLY_NV")) cap = std::atoi(env);
  int widest = 0;
  for (int w : kCoefWidths)
    if (size_t(2 + w) * size_t(a.lds_vert) * sizeof(T) <= size_t(64) * 1024 && (cap < 2 || w <= cap) &&
        (slots == 7 || w <= kCoefWide15))
      widest = w;
  if (widest == 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "ring plan exceeds the kernel's capacities");
  const bool mass = beta != 0.0, chunk = z[13] != 0;
  const int per = int((z[0] + 7) / 8);
  for (int64_t col0 = 0; col0 < n_vec;) {
    const int64_t left = n_vec - col0;
    int nv = widest;
    for (int w : kCoefWidths)
      if (w >= left && w < nv) nv = w;
    m.col0 = unsigned(col0);
    m.n_col = unsigned(std::min<int64_t>(left, nv));
    void *kernel = pick_coef_multi<T>(nv, slots, mass, chunk, tables.nq);
    if (!kernel) return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
    const size_t lds = size_t(2 + nv) * size_t(a.lds_vert) * sizeof(T);
    int per_cu = 0;
    st = resident_per_cu(kernel, kRingBlock, lds, &per_cu);
    if (st != TFEM_OK) return st;
    const int blocks = std::min(per * 8, (device_cu_count() * per_cu / 8) * 8);
    void *params[] = {&K};
    hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(std::max(blocks, 8))), dim3(kRingBlock), params, lds, stream);
    if (e != hipSuccess) return fail(TFEM_ERR_HIP, "coefficient kernel launch: %s", hipGetErrorString(e));
    col0 += m.n_col;
  }
  return TFEM_OK;
}

}  // namespace tfem

extern "C" {

int tfem_p1_apply_rings_coef_multi(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha,
                                   double beta, const tfem_source_program *kappa, const tfem_source_program *c,
                                   const void *plan_device, const int64_t *plan_layout_host, const void *u, void *y,
                                   int64_t n_vec, void *stream) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (n_verts < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  if (n_vec < 1) return fail(TFEM_ERR_INVALID_ARGUMENT, "n_vec must be at least 1");
  if (!u) return fail(TFEM_ERR_INVALID_ARGUMENT, "u is NULL (the diagonal: tfem_p1_apply_rings_coef)");
  if (!kappa && !c)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "no coefficient program: constant coefficients take "
                "tfem_p1_apply_rings_multi");
  // the extent of u and y, before anything is derived from it
  const int64_t limit = int64_t(1) << 32;
  const int64_t vec_bytes = (n_verts > 0 && n_vec >= limit / n_verts) ? limit : n_verts * n_vec * real_bytes;
  int st = check_extents("ring kernel", &vec_bytes, 1);
  if (st != TFEM_OK) return st;
  const char *ub = static_cast<const char *>(u), *yb = static_cast<const char *>(y);
  if (y && ub < yb + vec_bytes && yb < ub + vec_bytes) return fail(TFEM_ERR_INVALID_ARGUMENT, "u and y overlap");
  if (kappa && src_validate(kappa) != TFEM_OK) return TFEM_ERR_INVALID_ARGUMENT;
  if (c && src_validate(c) != TFEM_OK) return TFEM_ERR_INVALID_ARGUMENT;
  const int64_t *z = plan_layout_host;
  if (z[23] > 0)
    return fail(TFEM_ERR_UNSUPPORTED, "a ring plan with long rows does not take coefficient programs");
  TriTables tables;
  if (!build_tri_tables(quad_order, real_bytes, &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if (n_vec == 1)  // one column: the single-vector launch, same layout
    return tfem_p1_apply_rings_coef(coords, real_bytes, n_verts, quad_order, alpha, beta, kappa, c, plan_device, z, u,
                                    y, stream);
  if (z[0] == 0 || n_verts == 0) return TFEM_OK;
  const unsigned char *plan = static_cast<const unsigned char *>(plan_device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8
             ? launch_coef_multi<double>(tables, coords, n_verts, alpha, beta, kappa, c, plan, z, u, y, n_vec, s)
             : launch_coef_multi<float>(tables, coords, n_verts, alpha, beta, kappa, c, plan, z, u, y, n_vec, s);
}

}  // extern "C"
