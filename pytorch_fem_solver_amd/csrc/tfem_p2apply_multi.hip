// Matrix-free P2 operator on several vectors in one launch: Y = (alpha * stiffness + beta * mass) U
// over the P2 row plan, U and Y (n_dofs, n_vec) row-major (ApplyMultiArgs of tfem_rings_cols.hpp).
//
// The tile walk is k_p2_apply_rows<T, KIND, MASS, false> of tfem_p2apply.hip: the same mapping of
// tiles to workgroups, descriptor reads, coordinates in LDS, one barrier, the exclusive scan of the
// true row lengths for the CSR start.  What does not depend on the column is paid once per pass of
// NV columns: the row record, the column ids (colind), the coordinates and the row's entries (22 of
// a vertex row, 9 of an edge row).  The lane then forms NV sums, each in exactly the order of the
// single kernel, so column j of Y has the bits tfem_p2_apply_rows gives for column j.  The u of a
// column id are one NV-wide load; entries that do not exist load behind the array (zeros).
//
// Vertex rows with 8 .. 15 neighbours: k_p2_apply_long_rows_multi, sixteen lanes per row as
// k_p2_apply_long_rows, the slot's entries formed once and every column one sum over the sixteen.
//
// That is the fp64 form.  In fp32 the roundings of the single kernel depend on how the compiler
// pairs the operations of a whole row into packed instructions (a product that shares a packed
// multiply is not contracted into the sum behind it), so sums formed NV at a time from entries
// formed once round differently.  The fp32 kernels (NV == 1) therefore read the record, the column
// ids and the coordinates once per row and launch, and then run the statements of the single kernel
// once per column: the traffic of the block launch, the arithmetic of k launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "tfem_assembly.h"
#include "tfem_common.hpp"
#include "tfem_rowkit.hpp"
#include "tfem_p2rows_kernel.hpp"
#include "tfem_rings_cols.hpp"

#pragma clang fp contract(fast)

namespace tfem {

constexpr unsigned kP2MultiPast = 0xFFFFFF00u;  // kP2ApplyPast of tfem_p2apply.hip: loads give 0, stores are dropped

template <typename T>
__device__ __forceinline__ T p2_multi_load(ring_rsrc_t r, unsigned byte) {
  if constexpr (sizeof(T) == 8) {  // two dword loads, as p2_apply_load
    const ru32x2 v{__builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0),
                   __builtin_amdgcn_raw_buffer_load_b32(r, byte + 4u, 0, 0)};
    return __builtin_bit_cast(double, v);
  } else {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte, 0, 0));
  }
}

template <typename T>
__device__ __forceinline__ void p2_multi_store(ring_rsrc_t r, unsigned byte, T v) {
  if constexpr (sizeof(T) == 8)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, v), r, byte, 0, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byte, 0, 0);
}

// Slots of a vertex row whose u are fetched in front of the barrier (they travel while the fan is
// walked); the u of the other slots are fetched slot by slot behind it, so that a lane never holds
// the 22 * NV values of its row at once.
template <typename T, int NV>
constexpr int p2_multi_early() {
  return NV * int(sizeof(T)) <= 16 ? 7 : (NV * int(sizeof(T)) <= 32 ? 3 : 1);
}

// ONE column of a vertex row, statement for statement the vertex branch of k_p2_apply_rows behind its
// barrier: the fan walk, the wrap of slot k into slot 0, the sum.  w: the row's record.
template <typename T, bool MASS>
__device__ __forceinline__ T p2_vertex_row_value(const P2RowArgs<T> &a, const uint32_t (&w)[8], const T *xy, bool has_row,
                                                 int my_row, T us, const T (&uv)[7], const T (&ue)[7],
                                                 const T (&uo)[7]) {
  const int k = int((w[2] >> 24) & 7u);
  auto id = [&](int i) { return (w[i / 3] >> (10 * (i % 3))) & 0x3FFu; };
  auto flag_of = [&](int i) { return (w[2] >> (10 + 2 * i)) & 3u; };
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
  T wv = vcol[1], we = ecol[1];
#pragma unroll
  for (int j = 2; j <= 7; ++j) {
    wv = k == j ? vcol[j] : wv;
    we = k == j ? ecol[j] : we;
  }
  vcol[0] = vcol[0] + wv;
  ecol[0] = ecol[0] + we;
  T yv = k > 0 ? diag * us : T(0);
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const bool on = i < k;
    yv = yv + (on ? vcol[i] : T(0)) * uv[i];
    yv = yv + (on ? ecol[i] : T(0)) * ue[i];
    yv = yv + ((on && flag_of(i)) ? ocol[i] : T(0)) * uo[i];
  }
  return yv;
}

// ONE column of an edge row, statement for statement the edge branch of k_p2_apply_rows.
template <typename T, bool MASS>
__device__ __forceinline__ T p2_edge_row_value(const P2RowArgs<T> &a, const uint32_t (&w)[4], const T *xy, bool has_row,
                                               const T (&ue)[9]) {
  const bool has2 = (w[1] >> 10) & 1u;
  const bool rev = (w[1] >> 11) & 1u;
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
    const T ox = rev ? bx : ax, oy = rev ? by : ay;
    const T tx = rev ? ax : bx, ty = rev ? ay : by;
    const T e1x = tx - ox, e1y = ty - oy, e2x = dx - ox, e2y = dy - oy;
    p2_block_row<T, MASS>(a, e1x * e1x + e1y * e1y, e2x * e2x + e2y * e2y, e1x * e2x + e1y * e2y,
                          e1x * e2y - e1y * e2x, (has_row && has2) ? 1u : 0u, s);
  }
  T yv = (r[3] + s[3]) * ue[3];
  yv = yv + (r[0] + (rev ? s[1] : s[0])) * ue[0];
  yv = yv + (r[1] + (rev ? s[0] : s[1])) * ue[1];
  yv = yv + r[2] * ue[2];
  yv = yv + r[4] * ue[4];
  yv = yv + r[5] * ue[5];
  yv = yv + s[2] * ue[6];
  yv = yv + s[4] * ue[7];
  yv = yv + s[5] * ue[8];
  return yv;
}

// The record of a row behind a fence the optimiser does not look through: what is computed from
// the copy is computed where the copy is made (inside the column loop of the NV = 1 kernels).
template <int N>
__device__ __forceinline__ void p2_fenced_copy(const uint32_t (&w)[N], uint32_t (&c)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    c[i] = w[i];
    asm volatile("" : "+v"(c[i]));
  }
}

// KIND 0: vertex rows, KIND 1: edge rows.  NV >= 2: b.col0 / b.n_col are the columns of this pass,
// the row's entries are formed once and NV sums are formed from them.  NV == 1: every column of the
// block in this one launch, one at a time; the record, the column ids and the coordinates are read
// once, but the row is formed again for every column by the code of the single kernel -- the fp32
// form.  The compiler pairs fp32 operations into packed instructions, and which products of the
// single kernel are contracted into an fma follows from that pairing over the whole row; only the
// same statements on one column at a time reproduce its roundings.  fp64 has no packed arithmetic.
template <typename T, int KIND, bool MASS, int NV>
__global__ __launch_bounds__(kP2Block) void k_p2_apply_rows_multi(const P2RowArgs<T> a, const ApplyMultiArgs<T> b,
                                                                  const int32_t *colind, unsigned colind_bytes) {
  static_assert(NV == 1 || NV % 2 == 0, "columns per pass come in pairs");
  extern __shared__ __attribute__((aligned(16))) unsigned char p2m_smem[];
  T *xy = reinterpret_cast<T *>(p2m_smem);  // [2 * lds_vert]
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
  const ring_rsrc_t r_col = ring_rsrc(colind, colind_bytes);
  const ring_rsrc_t r_u = ring_rsrc(b.u, b.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(b.y, b.y_bytes);
  const unsigned row_bytes = b.n_vec * unsigned(sizeof(T)), col_byte = b.col0 * unsigned(sizeof(T));
  const int my_row = row0 + lane;
  const bool has_row = my_row < row1;
  constexpr int kWords = KIND == 0 ? 8 : 4;
  uint32_t w[kWords];
  {
    const unsigned byte = has_row ? a.off_rows + unsigned(row_off + my_row) * unsigned(4 * kWords) : kP2MultiPast;
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
  // coordinates of the tile's vertices -> LDS, as k_p2_apply_rows
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
  // the NV values of the pass in the row of U of a column id; entries that do not exist read
  // behind the array: zeros
  auto u_at = [&](bool on, unsigned col, T(&v)[NV]) {
    if constexpr (NV > 1) apply_load_cols<T, NV>(r_u, on ? col * row_bytes + col_byte : kP2MultiPast, v);
  };
  // NV == 1: column c of the row of U of a column id
  auto u_one = [&](bool on, unsigned col, unsigned c) {
    return p2_multi_load<T>(r_u, on ? col * row_bytes + c * unsigned(sizeof(T)) : kP2MultiPast);
  };
  const unsigned self_byte = unsigned(dof0 + lane) * row_bytes + col_byte;
  T yv[NV];
  bool writes = has_row;
  if constexpr (KIND == 0) {
    const int k = int((w[2] >> 24) & 7u);
    auto id = [&](int i) { return (w[i / 3] >> (10 * (i % 3))) & 0x3FFu; };
    auto flag_of = [&](int i) { return (w[2] >> (10 + 2 * i)) & 3u; };
    auto field = [&](int f) { return int((w[3 + f / 6] >> (5 * (f % 6))) & 31u); };
    // long rows (written by k_p2_apply_long_rows_multi): k = 0 here, their length only moves the
    // CSR position of the rows behind them
    const bool is_long = has_row && k == 0 && (w[3] >> 31) != 0u;
    writes = has_row && !is_long;
    const uint32_t flags = (w[2] >> 10) & 0x3FFFu;
    const int n_tri = __builtin_popcount((flags | (flags >> 1)) & 0x1555u);
    const int true_len = is_long ? int(w[3] & 0x7FFFFFFFu) : (k > 0 ? 1 + 2 * k + n_tri : 0);
    const int start = rs0 + wave_inclusive_scan(true_len) - true_len;
    auto col_at = [&](bool on, int p) {
      return __builtin_amdgcn_raw_buffer_load_b32(r_col, on ? unsigned(start + p) * 4u : kP2MultiPast, 0, 0);
    };
    unsigned vc[7], ec[7], oc[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      vc[i] = col_at(i < k, field(i));
      ec[i] = col_at(i < k, field(7 + i));
      oc[i] = col_at(i < k && flag_of(i), field(14 + i));
    }
    stage_coords();
    if constexpr (NV == 1) {
      __syncthreads();
#pragma clang loop unroll(disable) vectorize(disable)
      for (unsigned c = 0; c < b.n_vec; ++c) {
        T us, uv[7], ue[7], uo[7];
        us = u_one(k > 0, unsigned(dof0 + lane), c);
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          uv[i] = u_one(i < k, vc[i], c);
          ue[i] = u_one(i < k, ec[i], c);
          uo[i] = u_one(i < k && flag_of(i), oc[i], c);
        }
        uint32_t wc[8];
        p2_fenced_copy<8>(w, wc);
        const T y1 = p2_vertex_row_value<T, MASS>(a, wc, xy, has_row, my_row, us, uv, ue, uo);
        p2_multi_store<T>(r_y, writes ? unsigned(dof0 + lane) * row_bytes + c * unsigned(sizeof(T)) : kP2MultiPast, y1);
      }
      return;
    }
    constexpr int kEarly = p2_multi_early<T, NV>();
    T us[NV], uv[kEarly][NV], ue[kEarly][NV], uo[kEarly][NV];
    u_at(k > 0, unsigned(dof0 + lane), us);
#pragma unroll
    for (int i = 0; i < kEarly; ++i) {
      u_at(i < k, vc[i], uv[i]);
      u_at(i < k, ec[i], ue[i]);
      u_at(i < k && flag_of(i), oc[i], uo[i]);
    }
    __syncthreads();
    // ---- vertex row: the fan, as k_p2_apply_rows ---------------------------------------------
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
    // a vertex without elements (k = 0): an empty row, y = 0 whatever u holds
#pragma unroll
    for (int c = 0; c < NV; ++c) yv[c] = k > 0 ? diag * us[c] : T(0);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      // slots i >= k hold what the walk left there (slot k: the closing triangle): no entry
      const bool on = i < k;
      const T kv = on ? vcol[i] : T(0), ke = on ? ecol[i] : T(0), ko = (on && flag_of(i)) ? ocol[i] : T(0);
      T sv[NV], se[NV], so[NV];
      if (i < kEarly) {
#pragma unroll
        for (int c = 0; c < NV; ++c) {
          sv[c] = uv[i < kEarly ? i : 0][c];
          se[c] = ue[i < kEarly ? i : 0][c];
          so[c] = uo[i < kEarly ? i : 0][c];
        }
      } else {
        u_at(on, vc[i], sv);
        u_at(on, ec[i], se);
        u_at(on && flag_of(i), oc[i], so);
      }
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        yv[c] = yv[c] + kv * sv[c];
        yv[c] = yv[c] + ke * se[c];
        yv[c] = yv[c] + ko * so[c];
      }
    }
  } else {
    const bool has2 = (w[1] >> 10) & 1u;
    const bool rev = (w[1] >> 11) & 1u;
    auto pos = [&](int f) { return int(((f < 8 ? w[2] >> (4 * f) : w[3]) & 15u)); };
    const int len = has_row ? (has2 ? 9 : 6) : 0;
    const int start = rs0 + wave_inclusive_scan(len) - len;
    unsigned col[9];
#pragma unroll
    for (int f = 0; f < 9; ++f) {
      const bool on = has_row && (f < 6 || has2);
      col[f] = f == 3 ? 0u  // the row itself
                      : __builtin_amdgcn_raw_buffer_load_b32(r_col, on ? unsigned(start + pos(f)) * 4u : kP2MultiPast, 0, 0);
    }
    stage_coords();
    if constexpr (NV == 1) {
      __syncthreads();
#pragma clang loop unroll(disable) vectorize(disable)
      for (unsigned c = 0; c < b.n_vec; ++c) {
        T u1[9];
#pragma unroll
        for (int f = 0; f < 9; ++f)
          u1[f] = u_one(has_row && (f < 6 || has2), f == 3 ? unsigned(dof0 + lane) : col[f], c);
        uint32_t wc[4];
        p2_fenced_copy<4>(w, wc);
        const T y1 = p2_edge_row_value<T, MASS>(a, wc, xy, has_row, u1);
        p2_multi_store<T>(r_y, writes ? unsigned(dof0 + lane) * row_bytes + c * unsigned(sizeof(T)) : kP2MultiPast, y1);
      }
      return;
    }
    T ue[9][NV];
#pragma unroll
    for (int f = 0; f < 9; ++f) {
      const bool on = has_row && (f < 6 || has2);
      u_at(on, f == 3 ? unsigned(dof0 + lane) : col[f], ue[f]);
    }
    __syncthreads();
    // ---- edge row: one or two triangles, each in its own stored frame, as k_p2_apply_rows ------
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
    // the nine entries once, then every column in the order of k_p2_apply_rows; s is all zero
    // without a second triangle, and so are the u of its columns
    const T k3 = r[3] + s[3], k0 = r[0] + (rev ? s[1] : s[0]), k1 = r[1] + (rev ? s[0] : s[1]);
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      T t = k3 * ue[3][c];
      t = t + k0 * ue[0][c];
      t = t + k1 * ue[1][c];
      t = t + r[2] * ue[2][c];
      t = t + r[4] * ue[4][c];
      t = t + r[5] * ue[5][c];
      t = t + s[2] * ue[6][c];
      t = t + s[4] * ue[7][c];
      t = t + s[5] * ue[8][c];
      yv[c] = t;
    }
  }
  // a wave's rows are consecutive DoFs: 64 * n_col consecutive reals per wave
  if constexpr (NV > 1) apply_store_cols<T, NV>(r_y, writes ? self_byte : kP2MultiPast, yv, b.n_col);
}

// k_p2_apply_long_rows for n_vec columns: the sixteen lanes of a row form their entries once, then
// every column is the slot's three products, the diagonal's share and one sum over the sixteen.
// fp32 forms the entries again for every column, by the statements of k_p2_apply_long_rows on one
// column (see k_p2_apply_rows_multi, NV == 1); the column ids are read once in both forms.
template <typename T, bool MASS>
__global__ __launch_bounds__(kP2Block) void k_p2_apply_long_rows_multi(const P2RowArgs<T> a, const ApplyMultiArgs<T> b,
                                                                       const int32_t *colind, unsigned colind_bytes,
                                                                       unsigned off_long, int n_long) {
  const int gtid = int(blockIdx.x) * kP2Block + int(threadIdx.x);
  const int row = gtid >> 4, i = gtid & 15;
  const bool live = row < n_long;
  const int lane = int(threadIdx.x) & 63;
  const ring_rsrc_t r_col = ring_rsrc(colind, colind_bytes);
  const ring_rsrc_t r_u = ring_rsrc(b.u, b.u_bytes);
  const ring_rsrc_t r_y = ring_rsrc(b.y, b.y_bytes);
  // the slot's share of the row from the record of long row `at`: the diagonal's share r0, the
  // entries of the slot's vertex, edge and opposite-edge columns
  struct Slot {
    uint32_t v, flag;
    bool slot;
    T r0, vcol, ecol, ocol;
  };
  auto form = [&](int at) {
    const uint32_t *rec = reinterpret_cast<const uint32_t *>(a.plan + off_long) + 32 * size_t(live ? at : 0);
    Slot s;
    s.v = rec[0];
    const int k = int(rec[2] & 0xFFu);
    s.slot = live && i < k;
    s.flag = s.slot ? (rec[3] >> (2 * i)) & 3u : 0u;
    const int nxt = i + 1 == k ? 0 : i + 1;
    const uint32_t g0 = rec[4 + (s.slot ? i : 0)], g1 = rec[4 + (s.slot ? nxt : 0)];
    const T xv = a.coords[2 * size_t(s.v)], yv = a.coords[2 * size_t(s.v) + 1];
    const T ecx = a.coords[2 * size_t(g0)] - xv, ecy = a.coords[2 * size_t(g0) + 1] - yv;
    const T enx = a.coords[2 * size_t(g1)] - xv, eny = a.coords[2 * size_t(g1) + 1] - yv;
    T r[6];
    p2_block_row<T, MASS>(a, ecx * ecx + ecy * ecy, enx * enx + eny * eny, ecx * enx + ecy * eny,
                          ecx * eny - ecy * enx, s.flag, r);
    // r: v, p1, p2, edge (v,p1), edge (p1,p2), edge (p2,v); (p1, p2) = (n_i, n_next) for flag 1 and
    // (n_next, n_i) for flag 2
    const bool fwd = s.flag != 2u;
    const T own_v = fwd ? r[1] : r[2], own_e = fwd ? r[3] : r[5];    // to this slot's columns
    const T next_v = fwd ? r[2] : r[1], next_e = fwd ? r[5] : r[3];  // to the next slot's columns
    const int from = (lane & ~15) + (i == 0 ? (k > 0 ? k - 1 : 0) : i - 1);
    s.vcol = own_v + __shfl(next_v, from, 64);
    s.ecol = own_e + __shfl(next_e, from, 64);
    s.r0 = r[0];
    s.ocol = r[4];
    return s;
  };
  Slot s = form(row);
  // the slot's three columns, read once
  const uint32_t *rec = reinterpret_cast<const uint32_t *>(a.plan + off_long) + 32 * size_t(live ? row : 0);
  auto field = [&](int f) { return int((rec[19 + f / 5] >> (6 * (f % 5))) & 63u); };
  auto col_at = [&](bool on, int p) {
    return __builtin_amdgcn_raw_buffer_load_b32(r_col, on ? (rec[1] + unsigned(p)) * 4u : kP2MultiPast, 0, 0);
  };
  const unsigned c_v = col_at(s.slot, field(i)), c_e = col_at(s.slot, field(15 + i));
  const unsigned c_o = col_at(s.slot && s.flag, field(30 + i));
  const unsigned row_bytes = b.n_vec * unsigned(sizeof(T));
  // byte of column 0 in the rows of U of the slot's three columns and of the row itself (used by
  // the lanes that have the entry alone: the others read behind the array)
  const unsigned b_v = c_v * row_bytes, b_e = c_e * row_bytes, b_o = c_o * row_bytes, b_self = s.v * row_bytes;
  const bool slot = s.slot, has_o = s.slot && s.flag, first = live && i == 0;
#pragma clang loop unroll(disable) vectorize(disable)
  for (unsigned c = 0; c < b.n_vec; ++c) {  // uniform: every lane takes part in the sums
    const unsigned cb = c * unsigned(sizeof(T));
    const T u_v = p2_multi_load<T>(r_u, slot ? b_v + cb : kP2MultiPast);
    const T u_e = p2_multi_load<T>(r_u, slot ? b_e + cb : kP2MultiPast);
    const T u_o = p2_multi_load<T>(r_u, has_o ? b_o + cb : kP2MultiPast);
    const T u_self = p2_multi_load<T>(r_u, first ? b_self + cb : kP2MultiPast);
    if constexpr (sizeof(T) == 4) {
      int at = row;
      asm volatile("" : "+v"(at));
      s = form(at);
    }
    T sum = s.r0 * __shfl(u_self, lane & ~15, 64) + (s.slot ? s.vcol * u_v + s.ecol * u_e + s.ocol * u_o : T(0));
    sum = sum + __shfl_xor(sum, 8, 64);
    sum = sum + __shfl_xor(sum, 4, 64);
    sum = sum + __shfl_xor(sum, 2, 64);
    sum = sum + __shfl_xor(sum, 1, 64);
    p2_multi_store<T>(r_y, first ? b_self + cb : kP2MultiPast, sum);
  }
}

// Widths of k_p2_apply_rows_multi that are built (DESIGN.md section 3 says why these).
constexpr int kP2ApplyWidths[] = {2, 4};

template <typename T, int KIND, int NV>
static void *pick_p2_multi_mass(bool mass) {
  return mass ? reinterpret_cast<void *>(k_p2_apply_rows_multi<T, KIND, true, NV>)
              : reinterpret_cast<void *>(k_p2_apply_rows_multi<T, KIND, false, NV>);
}

// fp32: the column loop inside the launch (NV == 1), whatever the width asked for
template <typename T, int KIND>
static void *pick_p2_multi(int nv, bool mass) {
  if constexpr (sizeof(T) == 4) {
    return pick_p2_multi_mass<T, KIND, 1>(mass);
  } else {
    switch (nv) {
      case 2: return pick_p2_multi_mass<T, KIND, 2>(mass);
      default: return pick_p2_multi_mass<T, KIND, 4>(mass);
    }
  }
}

// Y = K U for n_vec >= 2 columns: per kind, passes of the widest width over column ranges; the last
// pass takes the narrowest width that holds what is left (fp32: one launch per kind loops over all
// columns).  TFEM_P2_APPLY_NV caps the width (timing of the widths against each other).
template <typename T>
static int launch_p2_apply_multi(const void *coords, int quad_order, double alpha, double beta,
                                 const unsigned char *plan, const int64_t *z, const int32_t *colind, int64_t nnz,
                                 const void *u, void *y, int64_t n_dofs, int64_t n_vec, hipStream_t stream) {
  TriTables tables;
  if (!build_tri_tables(quad_order, int(sizeof(T)), &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  if (z[0] + z[1] == 0) return TFEM_OK;
  if (!coords || !plan || !colind || !u || !y) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  if (z[4] > 1024 || z[5] > 1024 || z[6] > kP2Block)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "P2 row plan exceeds the kernel's capacities");
  const int64_t rb = int64_t(sizeof(T));
  const int64_t extents[4] = {z[2] * 2 * rb, z[16], nnz * 4, n_dofs * n_vec * rb};
  const int st = check_extents("P2 apply kernel", extents, 4, int64_t(kP2MultiPast));
  if (st != TFEM_OK) return st;
  const bool mass = beta != 0.0;
  ApplyMultiArgs<T> b;
  b.u = static_cast<const T *>(u);
  b.y = static_cast<T *>(y);
  b.u_bytes = b.y_bytes = unsigned(extents[3]);
  b.n_vec = unsigned(n_vec);
  b.col0 = 0u;
  b.n_col = unsigned(n_vec);
  unsigned colind_bytes = unsigned(extents[2]);
  int cap = 0;
  if (const char *env = std::getenv("TFEM_P2_APPLY_NV")) cap = std::atoi(env);
  int widest = kP2ApplyWidths[0];
  for (int wd : kP2ApplyWidths)
    if (cap < 2 || wd <= cap) widest = wd;
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
    // quadrature order: the tables of launch_p2_apply (tfem_p2apply.hip), statement for statement
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
    const int per = int((z[kind] + 7) / 8);
    for (int64_t col0 = 0; col0 < n_vec;) {
      const int64_t left = n_vec - col0;
      int nv = widest;
      for (int wd : kP2ApplyWidths)
        if (wd >= left && wd < nv) nv = wd;
      if (sizeof(T) == 4) nv = int(left);  // one launch takes every column
      b.col0 = unsigned(col0);
      b.n_col = unsigned(std::min<int64_t>(left, nv));
      void *kernel = kind == 0 ? pick_p2_multi<T, 0>(nv, mass) : pick_p2_multi<T, 1>(nv, mass);
      void *params[] = {&a, &b, &colind, &colind_bytes};
      hipError_t e = hipLaunchKernel(kernel, dim3(unsigned(per * 8)), block, params, lds, stream);
      if (e != hipSuccess) return fail(TFEM_ERR_HIP, "P2 block apply kernel launch: %s", hipGetErrorString(e));
      col0 += b.n_col;
    }
    if (kind == 0 && z[18] > 0) {  // the vertex rows with 8 .. 15 neighbours, every column in one launch
      void *long_kernel = mass ? reinterpret_cast<void *>(k_p2_apply_long_rows_multi<T, true>)
                               : reinterpret_cast<void *>(k_p2_apply_long_rows_multi<T, false>);
      unsigned off_long = unsigned(z[17]);
      int n_long = int(z[18]);
      void *long_params[] = {&a, &b, &colind, &colind_bytes, &off_long, &n_long};
      const dim3 lgrid{unsigned((16 * z[18] + kP2Block - 1) / kP2Block)};
      hipError_t e = hipLaunchKernel(long_kernel, lgrid, block, long_params, 0, stream);
      if (e != hipSuccess) return fail(TFEM_ERR_HIP, "P2 long-row block apply launch: %s", hipGetErrorString(e));
    }
  }
  return TFEM_OK;
}

}  // namespace tfem

extern "C" {

int tfem_p2_apply_rows_multi(const void *coords, int real_bytes, int quad_order, double alpha, double beta,
                             const void *plan_device, const int64_t *plan_layout_host, const int32_t *colind,
                             int64_t nnz, const void *u, void *y, int64_t n_dofs, int64_t n_vec, void *stream) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  if (nnz < 0 || n_dofs < 0) return fail(TFEM_ERR_INVALID_ARGUMENT, "negative size");
  if (n_vec < 1) return fail(TFEM_ERR_INVALID_ARGUMENT, "n_vec must be at least 1");
  const int64_t *z = plan_layout_host;
  if (n_dofs != z[2] + z[3])
    return fail(TFEM_ERR_INVALID_ARGUMENT, "the plan is for %lld DoFs, not %lld", (long long)(z[2] + z[3]),
                (long long)n_dofs);
  if (!u && z[0] + z[1] != 0)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "u is NULL (the diagonal has one column: tfem_p2_apply_rows)");
  // the extent of U and Y, before anything is derived from it
  const int64_t limit = int64_t(kP2MultiPast);
  const int64_t block_bytes = (n_dofs > 0 && n_vec >= limit / n_dofs) ? limit : n_dofs * n_vec * real_bytes;
  const int st = check_extents("P2 apply kernel", &block_bytes, 1, limit);
  if (st != TFEM_OK) return st;
  const char *ub = static_cast<const char *>(u), *yb = static_cast<const char *>(y);
  if (u && y && ub < yb + block_bytes && yb < ub + block_bytes)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "U and Y overlap");
  if (n_vec == 1)  // one column: the single-vector launch, same layout
    return tfem_p2_apply_rows(coords, real_bytes, quad_order, alpha, beta, plan_device, z, colind, nnz, u, y, n_dofs,
                              stream);
  const auto *plan = static_cast<const unsigned char *>(plan_device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return real_bytes == 8 ? launch_p2_apply_multi<double>(coords, quad_order, alpha, beta, plan, z, colind, nnz, u, y,
                                                         n_dofs, n_vec, s)
                         : launch_p2_apply_multi<float>(coords, quad_order, alpha, beta, plan, z, colind, nnz, u, y,
                                                        n_dofs, n_vec, s);
}

}  // extern "C"
