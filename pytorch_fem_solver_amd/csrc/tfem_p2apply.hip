// Matrix-free P2 operator over the P2 row plan: y = (alpha * stiffness + beta * mass) u without the
// CSR values (abstract_basis.py:74-93 with element_tri.py:43-70, applied instead of stored).
//
// The row kernels of tfem_p2rows.hip form every row of K in registers: one lane owns the row of a
// vertex DoF (its fan) or of an edge DoF (its one or two triangles).  Here the lane does not stage
// its entries for a store; it multiplies each by u of the entry's column and writes the one number
//     y_row = sum_entries K_row,col u_col.
// The plan's records hold the CSR POSITION of every entry inside its row, not the column: the
// column is colind[row start + position], the row start is the wave's CSR offset from the tile
// descriptor plus the exclusive scan of the row lengths in front of the lane (true lengths: a long
// row in the wave moves the rows behind it).  The diagonal entry needs no lookup, its column is the
// row.  Every lane issues the column loads of its row together, then the loads of u.  u == NULL
// writes diag(K) and reads neither colind nor u.
//
// One tile per 256-lane workgroup, the coordinates of the tile's vertices in LDS, one barrier:
// as k_p2_rows.  No value stage, so the LDS is the coordinates alone.  A wave's rows are
// consecutive DoFs: the stores of y coalesce.  Vertices with 8 .. 15 neighbours (long rows) are
// left out by the tile launch and formed by k_p2_apply_long_rows, sixteen lanes per row.
#include <hip/hip_runtime.h>

#include <cstring>

#include "tfem_common.hpp"
#include "tfem_rowkit.hpp"
#include "tfem_p2rows_kernel.hpp"

#pragma clang fp contract(fast)

namespace tfem {

template <typename T>
struct P2ApplyArgs {
  const int32_t *colind;
  const T *u;  // NULL: y = diag(K)
  T *y;
  unsigned colind_bytes, u_bytes, y_bytes;
};

constexpr unsigned kP2ApplyPast = 0xFFFFFF00u;  // beyond every buffer the launch accepts: loads give 0

template <typename T>
__device__ __forceinline__ T p2_apply_load(ring_rsrc_t r, unsigned byte) {
  if constexpr (sizeof(T) == 8) {  // two dword loads: raw_buffer_load_b64 is miscompiled by this hipcc (tfem_tiles.hip)
    const ru32x2 v{__builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0),
                   __builtin_amdgcn_raw_buffer_load_b32(r, byte + 4u, 0, 0)};
    return __builtin_bit_cast(double, v);
  } else {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0));
  }
}

template <typename T>
__device__ __forceinline__ void p2_apply_store(ring_rsrc_t r, unsigned byte, T v) {
  if constexpr (sizeof(T) == 8)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, v), r, byte, 0, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byte, 0, 0);
}

// KIND 0: vertex rows, KIND 1: edge rows.  DIAG: y = diag(K).
template <typename T, int KIND, bool MASS, bool DIAG>
__global__ __launch_bounds__(kP2Block) void k_p2_apply_rows(const P2RowArgs<T> a, const P2ApplyArgs<T> b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p2a_smem[];
  T *xy = reinterpret_cast<T *>(p2a_smem);  // [2 * lds_vert]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per = (a.n_tiles + 7) / 8;
  const int tile = int(blockIdx.x & 7) * per + int(blockIdx.x >> 3);
  if (tile >= a.n_tiles || int(blockIdx.x >> 3) >= per) return;
  ring_const_i32 d = (ring_const_i32)(uintptr_t)(a.plan + a.off_desc + 64u * unsigned(tile));
  const int vert_off = d[0], n_vert = d[1], row_off = d[2], n_own = d[7];
  const int row0 = d[3 + wave], row1 = d[4 + wave], dof0 = d[8 + wave], rs0 = d[12 + wave];
  const ring_rsrc_t r_coords = ring_rsrc(a.coords, a.coords_bytes);
  const ring_rsrc_t r_plan = ring_rsrc(a.plan, a.plan_bytes);
  const ring_rsrc_t r_col = ring_rsrc(b.colind, b.colind_bytes);
  const ring_rsrc_t r_u = ring_rsrc(b.u, b.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(b.y, b.y_bytes);
  const int my_row = row0 + lane;
  const bool has_row = my_row < row1;
  constexpr int kWords = KIND == 0 ? 8 : 4;
  uint32_t w[kWords];
  {
    const unsigned byte = has_row ? a.off_rows + unsigned(row_off + my_row) * unsigned(4 * kWords) : kP2ApplyPast;
    const ru32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r_plan, byte, 0, 0);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
    if constexpr (KIND == 0) {
      const ru32x4 t = __builtin_amdgcn_raw_buffer_load_b128(r_plan, byte + 16u, 0, 0);
      w[4] = t.x;
      w[5] = t.y;
      w[6] = t.z;
      w[7] = t.w;
    }
  }
  // coordinates of the tile's vertices -> LDS, as k_p2_rows (called between the loads of the column
  // ids and the loads of u: the ids travel while the coordinates are fetched and parked)
  auto stage_coords = [&]() {
    if (KIND == 0) {
      if (has_row) {
        T x, y;
        ring_load_xy<T>(r_coords, unsigned(dof0 + lane), x, y);
        xy[2 * my_row] = x;
        xy[2 * my_row + 1] = y;
      }
      for (int l = n_own + tid; l < n_vert; l += kP2Block) {
        const unsigned g = __builtin_amdgcn_raw_buffer_load_b32(r_plan, a.off_gid + unsigned(vert_off + l) * 4u, 0, 0);
        T x, y;
        ring_load_xy<T>(r_coords, g, x, y);
        xy[2 * l] = x;
        xy[2 * l + 1] = y;
      }
    } else {
      for (int l = tid; l < n_vert; l += kP2Block) {
        const unsigned g = __builtin_amdgcn_raw_buffer_load_b32(r_plan, a.off_gid + unsigned(vert_off + l) * 4u, 0, 0);
        T x, y;
        ring_load_xy<T>(r_coords, g, x, y);
        xy[2 * l] = x;
        xy[2 * l + 1] = y;
      }
    }
  };
  // column of the entry at position p of the lane's row / u of a column; entries that do not exist
  // read behind the arrays: column 0, u = 0
  const unsigned self_byte = unsigned(dof0 + lane) * unsigned(sizeof(T));
  T yv;
  bool writes = has_row;
  if constexpr (KIND == 0) {
    const int k = int((w[2] >> 24) & 7u);
    auto id = [&](int i) { return (w[i / 3] >> (10 * (i % 3))) & 0x3FFu; };
    auto flag_of = [&](int i) { return (w[2] >> (10 + 2 * i)) & 3u; };
    auto field = [&](int f) { return int((w[3 + f / 6] >> (5 * (f % 6))) & 31u); };
    // long rows (8 .. 15 neighbours, written by k_p2_apply_long_rows): k = 0 here, their length only
    // moves the CSR position of the rows behind them
    const bool is_long = has_row && k == 0 && (w[3] >> 31) != 0u;
    writes = has_row && !is_long;
    unsigned vc[7], ec[7], oc[7];
    T uv[7], ue[7], uo[7], us = T(0);
    if constexpr (!DIAG) {
      const uint32_t flags = (w[2] >> 10) & 0x3FFFu;
      const int n_tri = __builtin_popcount((flags | (flags >> 1)) & 0x1555u);
      const int true_len = is_long ? int(w[3] & 0x7FFFFFFFu) : (k > 0 ? 1 + 2 * k + n_tri : 0);
      const int start = rs0 + wave_inclusive_scan(true_len) - true_len;
      auto col_at = [&](bool on, int p) {
        return __builtin_amdgcn_raw_buffer_load_b32(r_col, on ? unsigned(start + p) * 4u : kP2ApplyPast, 0, 0);
      };
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        vc[i] = col_at(i < k, field(i));
        ec[i] = col_at(i < k, field(7 + i));
        oc[i] = col_at(i < k && flag_of(i), field(14 + i));
      }
      stage_coords();
      auto u_at = [&](bool on, unsigned col) {
        return p2_apply_load<T>(r_u, on ? col * unsigned(sizeof(T)) : kP2ApplyPast);
      };
      us = u_at(k > 0, unsigned(dof0 + lane));
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        uv[i] = u_at(i < k, vc[i]);
        ue[i] = u_at(i < k, ec[i]);
        uo[i] = u_at(i < k && flag_of(i), oc[i]);
      }
    } else {
      stage_coords();
    }
    __syncthreads();
    // ---- vertex row: the fan, as k_p2_rows ---------------------------------------------------
    T xv, yvv, px, py;
    lds_xy(xy, unsigned(has_row ? my_row : 0), xv, yvv);
    const uint32_t id0 = id(0);
    lds_xy(xy, id0, px, py);
    T ecx = px - xv, ecy = py - yvv;
    T qc = ecx * ecx + ecy * ecy;
    T diag = T(0), vcol[8], ecol[8], ocol[7];
#pragma unroll
    for (int i = 0; i < 8; ++i) vcol[i] = ecol[i] = T(0);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const uint32_t idn = (i + 1 < 7 && i + 1 != k) ? id(i + 1 < 7 ? i + 1 : 0) : id0;
      lds_xy(xy, idn, px, py);
      const T enx = px - xv, eny = py - yvv;
      const T qn = enx * enx + eny * eny;
      const T p = ecx * enx + ecy * eny;
      const T cross = ecx * eny - ecy * enx;
      const uint32_t flag = flag_of(i);  // 0 for every slot i >= k
      T r[6];
      p2_block_row<T, MASS>(a, qc, qn, p, cross, flag, r);
      // r: v, p1, p2, edge (v,p1), edge (p1,p2), edge (p2,v); (p1, p2) = (n_i, n_next) for
      // flag 1 and (n_next, n_i) for flag 2
      const bool fwd = flag != 2u;
      diag = diag + r[0];
      vcol[i] = vcol[i] + (fwd ? r[1] : r[2]);
      vcol[i + 1] = vcol[i + 1] + (fwd ? r[2] : r[1]);
      ecol[i] = ecol[i] + (fwd ? r[3] : r[5]);
      ecol[i + 1] = ecol[i + 1] + (fwd ? r[5] : r[3]);
      ocol[i] = r[4];
      ecx = enx;
      ecy = eny;
      qc = qn;
    }
    // what the closing triangle left in slot k belongs to slot 0
    T wv = vcol[1], we = ecol[1];
#pragma unroll
    for (int j = 2; j <= 7; ++j) {
      wv = k == j ? vcol[j] : wv;
      we = k == j ? ecol[j] : we;
    }
    vcol[0] = vcol[0] + wv;
    ecol[0] = ecol[0] + we;
    if constexpr (DIAG) {
      yv = diag;
    } else {
      // a vertex without elements (k = 0): an empty row, y = 0 whatever u holds
      yv = k > 0 ? diag * us : T(0);
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        // slots i >= k hold what the walk left there (slot k: the closing triangle): no entry
        const bool on = i < k;
        yv = yv + (on ? vcol[i] : T(0)) * uv[i];
        yv = yv + (on ? ecol[i] : T(0)) * ue[i];
        yv = yv + ((on && flag_of(i)) ? ocol[i] : T(0)) * uo[i];
      }
    }
  } else {
    const bool has2 = (w[1] >> 10) & 1u;
    const bool rev = (w[1] >> 11) & 1u;
    auto pos = [&](int f) { return int(((f < 8 ? w[2] >> (4 * f) : w[3]) & 15u)); };
    T ue[9];
    if constexpr (!DIAG) {
      const int len = has_row ? (has2 ? 9 : 6) : 0;
      const int start = rs0 + wave_inclusive_scan(len) - len;
      unsigned col[9];
#pragma unroll
      for (int f = 0; f < 9; ++f) {
        const bool on = has_row && (f < 6 || has2);
        col[f] = f == 3 ? 0u  // the row itself
                        : __builtin_amdgcn_raw_buffer_load_b32(r_col, on ? unsigned(start + pos(f)) * 4u : kP2ApplyPast, 0, 0);
      }
      stage_coords();
#pragma unroll
      for (int f = 0; f < 9; ++f) {
        const bool on = has_row && (f < 6 || has2);
        const unsigned byte = f == 3 ? self_byte : col[f] * unsigned(sizeof(T));
        ue[f] = p2_apply_load<T>(r_u, on ? byte : kP2ApplyPast);
      }
    } else {
      stage_coords();
    }
    __syncthreads();
    // ---- edge row: one or two triangles, each in its own stored frame, as k_p2_rows ------------
    T ax, ay, bx, by, cx, cy, dx, dy;
    lds_xy(xy, w[0] & 0x3FFu, ax, ay);
    lds_xy(xy, (w[0] >> 10) & 0x3FFu, bx, by);
    lds_xy(xy, (w[0] >> 20) & 0x3FFu, cx, cy);
    lds_xy(xy, w[1] & 0x3FFu, dx, dy);
    T r[6], s[6];
    {
      const T e1x = bx - ax, e1y = by - ay, e2x = cx - ax, e2y = cy - ay;
      p2_block_row<T, MASS>(a, e1x * e1x + e1y * e1y, e2x * e2x + e2y * e2y, e1x * e2x + e1y * e2y,
                            e1x * e2y - e1y * e2x, has_row ? 1u : 0u, r);
    }
    {
      // frame (a2, b2, d) = (b, a, d) when rev, (a, b, d) otherwise
      const T ox = rev ? bx : ax, oy = rev ? by : ay;
      const T tx = rev ? ax : bx, ty = rev ? ay : by;
      const T e1x = tx - ox, e1y = ty - oy, e2x = dx - ox, e2y = dy - oy;
      p2_block_row<T, MASS>(a, e1x * e1x + e1y * e1y, e2x * e2x + e2y * e2y, e1x * e2x + e1y * e2y,
                            e1x * e2y - e1y * e2x, (has_row && has2) ? 1u : 0u, s);
    }
    if constexpr (DIAG) {
      yv = r[3] + s[3];
    } else {
      // s is all zero without a second triangle, and so are the u of its columns
      yv = (r[3] + s[3]) * ue[3];
      yv = yv + (r[0] + (rev ? s[1] : s[0])) * ue[0];
      yv = yv + (r[1] + (rev ? s[0] : s[1])) * ue[1];
      yv = yv + r[2] * ue[2];
      yv = yv + r[4] * ue[4];
      yv = yv + r[5] * ue[5];
      yv = yv + s[2] * ue[6];
      yv = yv + s[4] * ue[7];
      yv = yv + s[5] * ue[8];
    }
  }
  // a wave's rows are consecutive DoFs: one contiguous store per wave
  p2_apply_store<T>(r_y, writes ? self_byte : kP2ApplyPast, yv);
}

// Vertex rows with 8 .. 15 neighbours: SIXTEEN lanes per row, lane i = slot i of the fan, as
// k_p2_long_rows.  A slot lane multiplies its three entries by u of their columns (colind at the
// row's CSR offset rec[1] + the entry's position); the products and the diagonal's shares are
// summed over the sixteen lanes and lane 0 writes y_v.
template <typename T, bool MASS, bool DIAG>
__global__ __launch_bounds__(kP2Block) void k_p2_apply_long_rows(const P2RowArgs<T> a, const P2ApplyArgs<T> b,
                                                                 unsigned off_long, int n_long) {
  const int gtid = int(blockIdx.x) * kP2Block + int(threadIdx.x);
  const int row = gtid >> 4, i = gtid & 15;
  const bool live = row < n_long;
  const uint32_t *rec = reinterpret_cast<const uint32_t *>(a.plan + off_long) + 32 * size_t(live ? row : 0);
  const uint32_t v = rec[0];
  const int k = int(rec[2] & 0xFFu);
  const bool slot = live && i < k;
  const uint32_t flag = slot ? (rec[3] >> (2 * i)) & 3u : 0u;
  const int nxt = i + 1 == k ? 0 : i + 1;
  const uint32_t g0 = rec[4 + (slot ? i : 0)], g1 = rec[4 + (slot ? nxt : 0)];
  const ring_rsrc_t r_col = ring_rsrc(b.colind, b.colind_bytes);
  const ring_rsrc_t r_u = ring_rsrc(b.u, b.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(b.y, b.y_bytes);
  auto field = [&](int f) { return int((rec[19 + f / 5] >> (6 * (f % 5))) & 63u); };
  T u_v = T(0), u_e = T(0), u_o = T(0), u_self = T(0);
  if constexpr (!DIAG) {
    auto col_at = [&](bool on, int p) {
      return __builtin_amdgcn_raw_buffer_load_b32(r_col, on ? (rec[1] + unsigned(p)) * 4u : kP2ApplyPast, 0, 0);
    };
    const unsigned c_v = col_at(slot, field(i)), c_e = col_at(slot, field(15 + i));
    const unsigned c_o = col_at(slot && flag, field(30 + i));
    u_v = p2_apply_load<T>(r_u, slot ? c_v * unsigned(sizeof(T)) : kP2ApplyPast);
    u_e = p2_apply_load<T>(r_u, slot ? c_e * unsigned(sizeof(T)) : kP2ApplyPast);
    u_o = p2_apply_load<T>(r_u, (slot && flag) ? c_o * unsigned(sizeof(T)) : kP2ApplyPast);
    u_self = p2_apply_load<T>(r_u, (live && i == 0) ? v * unsigned(sizeof(T)) : kP2ApplyPast);
  }
  const T xv = a.coords[2 * size_t(v)], yv = a.coords[2 * size_t(v) + 1];
  const T ecx = a.coords[2 * size_t(g0)] - xv, ecy = a.coords[2 * size_t(g0) + 1] - yv;
  const T enx = a.coords[2 * size_t(g1)] - xv, eny = a.coords[2 * size_t(g1) + 1] - yv;
  T r[6];
  p2_block_row<T, MASS>(a, ecx * ecx + ecy * ecy, enx * enx + eny * eny, ecx * enx + ecy * eny,
                        ecx * eny - ecy * enx, flag, r);
  // r: v, p1, p2, edge (v,p1), edge (p1,p2), edge (p2,v); (p1, p2) = (n_i, n_next) for flag 1 and
  // (n_next, n_i) for flag 2
  const bool fwd = flag != 2u;
  const T own_v = fwd ? r[1] : r[2], own_e = fwd ? r[3] : r[5];    // to this slot's columns
  const T next_v = fwd ? r[2] : r[1], next_e = fwd ? r[5] : r[3];  // to the next slot's columns
  const int lane = int(threadIdx.x) & 63;
  const int from = (lane & ~15) + (i == 0 ? (k > 0 ? k - 1 : 0) : i - 1);
  const T vcol = own_v + __shfl(next_v, from, 64);
  const T ecol = own_e + __shfl(next_e, from, 64);
  // the diagonal's share of the slot, and with u the slot's three products (r is zero without a
  // triangle, vcol / ecol of a lane that is no slot are dropped)
  T sum = r[0];
  if constexpr (!DIAG) sum = r[0] * __shfl(u_self, lane & ~15, 64) + (slot ? vcol * u_v + ecol * u_e + r[4] * u_o : T(0));
  sum = sum + __shfl_xor(sum, 8, 64);
  sum = sum + __shfl_xor(sum, 4, 64);
  sum = sum + __shfl_xor(sum, 2, 64);
  sum = sum + __shfl_xor(sum, 1, 64);
  p2_apply_store<T>(r_y, (live && i == 0) ? v * unsigned(sizeof(T)) : kP2ApplyPast, sum);
}

template <typename T, int KIND>
static void *pick_p2_apply(bool mass, bool diag) {
  if (mass)
    return diag ? reinterpret_cast<void *>(k_p2_apply_rows<T, KIND, true, true>)
                : reinterpret_cast<void *>(k_p2_apply_rows<T, KIND, true, false>);
  return diag ? reinterpret_cast<void *>(k_p2_apply_rows<T, KIND, false, true>)
              : reinterpret_cast<void *>(k_p2_apply_rows<T, KIND, false, false>);
}

template <typename T>
static int launch_p2_apply(const void *coords, int quad_order, double alpha, double beta, const unsigned char *plan,
                           const int64_t *z, const int32_t *colind, int64_t nnz, const void *u, void *y,
                           int64_t n_dofs, hipStream_t stream) {
  TriTables tables;
  if (!build_tri_tables(quad_order, int(sizeof(T)), &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if (z[0] + z[1] == 0) return TFEM_OK;
  if (!coords || !plan || !colind || !y) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  if (z[4] > 1024 || z[5] > 1024 || z[6] > kP2Block)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "P2 row plan exceeds the kernel's capacities");
  const int64_t rb = int64_t(sizeof(T));
  const int64_t extents[4] = {z[2] * 2 * rb, z[16], nnz * 4, n_dofs * rb};
  const int st = check_extents("P2 apply kernel", extents, 4, int64_t(kP2ApplyPast));
  if (st != TFEM_OK) return st;
  const bool mass = beta != 0.0, diag = u == nullptr;
  P2ApplyArgs<T> b;
  b.colind = colind;
  b.u = static_cast<const T *>(u);
  b.y = static_cast<T *>(y);
  b.colind_bytes = unsigned(extents[2]);
  b.u_bytes = u ? unsigned(extents[3]) : 0u;
  b.y_bytes = unsigned(extents[3]);
  const dim3 block{unsigned(kP2Block)};
  for (int kind = 0; kind < 2; ++kind) {
    if (z[kind] == 0) continue;
    P2RowArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.coords = static_cast<const T *>(coords);
    a.plan = plan;
    a.coords_bytes = unsigned(extents[0]);
    a.plan_bytes = unsigned(extents[1]);
    a.off_desc = unsigned(z[10 + 3 * kind]);
    a.off_rows = unsigned(z[11 + 3 * kind]);
    a.off_gid = unsigned(z[12 + 3 * kind]);
    a.n_tiles = int(z[kind]);
    a.xcd_ranges = 1;
    a.lds_vert = (int(z[4 + kind]) + 1) & ~1;
    // row 0 (vertex DoF at p0) / row 3 (edge DoF (p0, p1)) of the constant maps, in T, sums in
    // quadrature order: the tables of launch_p2_rows (tfem_p2rows.hip)
    const int row = kind == 0 ? 0 : 3;
    for (int m = 0; m < 6; ++m) {
      T ca = T(0), cb = T(0), cd = T(0), cm = T(0);
      for (int q = 0; q < tables.nq; ++q) {
        const T hw = T(tables.hw[q]);
        const T r0 = T(tables.rgrad2[q][row][0]), r1 = T(tables.rgrad2[q][row][1]);
        const T m0 = T(tables.rgrad2[q][m][0]), m1 = T(tables.rgrad2[q][m][1]);
        ca = ca + hw * (r0 * m0);
        cb = cb + hw * (r0 * m1 + r1 * m0);
        cd = cd + hw * (r1 * m1);
        cm = cm + hw * (T(tables.phi2[q][row]) * T(tables.phi2[q][m]));
      }
      a.ca[m] = T(alpha) * ca;
      a.cb[m] = T(alpha) * cb;
      a.cd[m] = T(alpha) * cd;
      a.cm[m] = T(beta) * cm;
    }
    // the coordinates of at most 1024 vertices: 16 KB, no function attribute and no occupancy query
    const size_t lds = size_t(2 * a.lds_vert) * sizeof(T);
    void *kernel = kind == 0 ? pick_p2_apply<T, 0>(mass, diag) : pick_p2_apply<T, 1>(mass, diag);
    const int per = int((z[kind] + 7) / 8);
    void *params[] = {&a, &b};
    hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(per * 8)), block, params, lds, stream);
    if (e != hipSuccess) return fail(TFEM_ERR_HIP, "P2 apply kernel launch: %s", hipGetErrorString(e));
    if (kind == 0 && z[18] > 0) {  // the vertex rows with 8 .. 15 neighbours, sixteen lanes per row
      void *long_kernel = mass ? (diag ? reinterpret_cast<void *>(k_p2_apply_long_rows<T, true, true>)
                                       : reinterpret_cast<void *>(k_p2_apply_long_rows<T, true, false>))
                               : (diag ? reinterpret_cast<void *>(k_p2_apply_long_rows<T, false, true>)
                                       : reinterpret_cast<void *>(k_p2_apply_long_rows<T, false, false>));
      unsigned off_long = unsigned(z[17]);
      int n_long = int(z[18]);
      void *long_params[] = {&a, &b, &off_long, &n_long};
      const dim3 lgrid{unsigned((16 * z[18] + kP2Block - 1) / kP2Block)};
      e = hipLaunchKernel(long_kernel, lgrid, block, long_params, 0, stream);
      if (e != hipSuccess) return fail(TFEM_ERR_HIP, "P2 long-row apply launch: %s", hipGetErrorString(e));
    }
  }
  return TFEM_OK;
}

}  // namespace tfem

extern "C" {

int tfem_p2_apply_rows(const void *coords, int real_bytes, int quad_order, double alpha, double beta,
                       const void *plan_device, const int64_t *plan_layout_host, const int32_t *colind,
                       int64_t nnz, const void *u, void *y, int64_t n_dofs, void *stream) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (nnz < 0 || n_dofs < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  const int64_t *z = plan_layout_host;
  if (n_dofs != z[2] + z[3])
    return fail(TFEM_ERR_INVALID_ARGUMENT, "the plan is for %lld DoFs, not %lld", (long long)(z[2] + z[3]),
                (long long)n_dofs);
  const char *ub = static_cast<const char *>(u), *yb = static_cast<const char *>(y);
  const int64_t vec_bytes = n_dofs * real_bytes;  // past 4 GiB: refused with the other extents below
  if (u && y && ub < yb + vec_bytes && yb < ub + vec_bytes) return fail(TFEM_ERR_INVALID_ARGUMENT, "u and y overlap");
  const auto *plan = static_cast<const unsigned char *>(plan_device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8
             ? launch_p2_apply<double>(coords, quad_order, alpha, beta, plan, z, colind, nnz, u, y, n_dofs, s)
             : launch_p2_apply<float>(coords, quad_order, alpha, beta, plan, z, colind, nnz, u, y, n_dofs, s);
}

}  // extern "C"
