// The P1 row-form kernel k_p1_rings (template) and its launch structure: shared by
// tfem_rings.hip (matrix-only launches and launches that read pre-evaluated source values) and
// tfem_rings_src.hip (launches that evaluate a source program; built with other flags).
// Description of the kernel: tfem_rings.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "tfem_common.hpp"
#include "tfem_rowkit.hpp"
#include "tfem_source.hpp"

// Reassociation is harmless here (see above: the row form is not the reference's operation
// order anyway; parity is asserted at 1e-12 against the oracle).
#pragma clang fp contract(fast)

namespace tfem {

constexpr int kRingBlock = 256;             // lanes per workgroup = owned rows per tile
constexpr int kRingWaves = kRingBlock / 64;
constexpr int kRingVertCap = 1024;          // 10-bit local ids

template <typename T>
struct RingArgs {
  const T *coords;
  const unsigned char *plan;
  T *vals;
  const T *fq;  // (n_elems, Q) source values, load vector only
  T *fout;
  unsigned coords_bytes, plan_bytes, vals_bytes, fq_bytes, fout_bytes;
  unsigned off_desc, off_rows, off_rowstart, off_gid, off_elems, off_telems;
  int lds_elem;   // element slots reserved in LDS per buffer (load vector)
  int xcd_interleave;  // 0: every XCD walks its own contiguous eighth of the tile list
                       // G > 0: the tile list is dealt to the XCDs in blocks of G tiles (one
                       //        front of tiles across the chip)
  int n_tiles;    // tiles of this launch (off_desc points at the first one's descriptor)
  int lds_vert;   // vertex slots reserved in LDS
  T stiff_w;      // alpha * sum_q w_q / 2
  T mass_d, mass_o;  // beta * sum_q (w_q/2) l_i l_i, beta * sum_q (w_q/2) l_i l_j (i != j)
  T lamw[3][kMaxQuad];  // l_i(q) * w_q / 2 by local vertex i (load vector)
  T lam[3][kMaxQuad];   // l_i(q): the integration points of an element (source programs)
  T hw[kMaxQuad];       // w_q / 2 (source programs: g_i = sum_q (f_q w_q / 2) l_i(q) needs this and `lam`
                        // only -- a second table of 3 Q doubles does not fit the scalar registers and
                        // came back from its spill lanes with two v_readlane per use)
  // source programs, the 4-point rule (order 3: the centroid, weights (c0, c0, c0), and the three
  // points with weights (b, b, b) + d on vertex 1, 2, 0; element_tri.py:99-107): [0..2] c0, b, d;
  // [3..5] c0 w_0 / 2, b w_1 / 2, d w_1 / 2 of g_i = sum_q (f_q w_q / 2) l_i(q) (w_1 = w_2 = w_3):
  // g_i = c0 w_0/2 f_0 + b w_1/2 (f_1 + f_2 + f_3) + d w_1/2 f_{q(i)}
  // A launch of a SEP instantiation carries k [3..5] instead, k = c1 c3 the product of the factors behind
  // the program's two functions (host: src_separable_factor): g_i is linear in f, so phase G evaluates the
  // bare functions and the factors ride on the constants the shares are multiplied with anyway.
  T qsym[6];
  unsigned off_tverts;  // packed local vertex triples of the tiles' elements (source programs)
  // source programs: the launch walks positions [u_first, u_first + n_tiles) of the plan's chain
  // order (off_chain: position -> tile), a workgroup takes chain_len consecutive positions;
  // off_hin: per owned row the local id its vertex has in the previous tile of the block (uint16)
  unsigned off_chain, off_hin;
  int chain_len, u_first;
  // n_runs > 0 (launches over the whole plan): the chain order in n_runs runs (off_runs: first
  // position of every run, + the number of tiles), one per resident workgroup, a run = one block
  int n_runs;
  unsigned off_runs;
  // 1: plain instead of non-temporal value stores (the launch's store policy).  An int tested by
  // its bit 0 rather than a bool: the kernels keep the single scalar bit test of the former flag
  // word, and with it their instruction schedule (a bool test reorders the store branches)
  int plain_stores;
  SrcProgram<T> src;  // SRC instantiations: f(x, y), evaluated at the integration points in the launch
};

static_assert(__builtin_offsetof(RingArgs<double>, hw) == __builtin_offsetof(RingArgs<double>, lam) + 3 * kMaxQuad * sizeof(double) &&
                  __builtin_offsetof(RingArgs<float>, hw) == __builtin_offsetof(RingArgs<float>, lam) + 3 * kMaxQuad * sizeof(float),
              "the kernels read hw through the pointer to lam");

constexpr int kRingBand = 11;  // short slot loop of the 15-slot kernels (0: none)
// Issue priority of the source-program launches: workgroup b takes turns with the others by
// (tile number + b >> kRingPrioShift) & 3 (the kernel's tile loop)
constexpr int kRingPrioShift = 3;

// Field accessors of a row record (bit layout: tfem_rings_host.cpp).
template <int SLOTS>
struct RingRec {
  static constexpr int kWords = SLOTS == 7 ? 4 : 8;
  uint32_t w[kWords];
  __device__ __forceinline__ uint32_t id(int i) const { return (w[i / 3] >> (10 * (i % 3))) & 0x3FFu; }
  __device__ __forceinline__ int k() const {
    return SLOTS == 7 ? int((w[0] >> 30) | (((w[1] >> 30) & 1u) << 2))
                      : int((w[0] >> 30) | ((w[1] >> 30) << 2));
  }
  __device__ __forceinline__ int dpos() const {
    return SLOTS == 7 ? int((w[2] >> 24) & 7u) : int((w[2] >> 30) | ((w[3] >> 30) << 2));
  }
  __device__ __forceinline__ uint32_t flag(int i) const {
    return SLOTS == 7 ? (w[2] >> (10 + 2 * i)) & 3u : (w[SLOTS == 7 ? 0 : 5] >> (2 * i)) & 3u;
  }
  __device__ __forceinline__ int pos(int i) const {
    if (SLOTS == 7) return int((w[3] >> (3 * i)) & 7u);
    return i < 8 ? int((w[SLOTS == 7 ? 0 : 6] >> (4 * (i & 7))) & 15u)
                 : int((w[SLOTS == 7 ? 0 : 7] >> (4 * (i & 7))) & 15u);
  }
};

// The diagonal of a row from the sum of its off-diagonal entries and, with mass, the sum of the
// signed determinants around the vertex.  Stiffness rows sum to zero (constants are in the kernel
// of the gradient): the diagonal is minus the sum of the off-diagonal stiffness entries.  With mass
// the sum also holds the off-diagonal mass (M_ij det, twice per triangle): it is taken out again
// before negating, and the diagonal mass is added.
template <typename T, bool MASS>
__device__ __forceinline__ T ring_diag(T sum, T dsum, T mass_d, T mass_o) {
  return MASS ? mass_d * dsum - (sum - T(2) * mass_o * dsum) : -sum;
}

// The row of local vertex `lv`: entries of the neighbour slots in off[0 .. k), the diagonal in
// diag (off[k ..] is scratch).  With q_i = |e_i|^2 and p = e_i.e_next the three entries of a
// triangle are c (p - q_next), c (p - q_i) and their negative sum, c = +-W / (e_i x e_next); the
// mass part adds det * M.  The triangle of slot i lands in off[i] and off[i + 1]; for the slot
// that closes the fan (i + 1 == k) the second one belongs to slot 0 and is moved there at the
// end (slots i >= k carry flag 0 and contribute nothing).  No branches: the reciprocal chains
// of the slots interleave.
// NIT < SLOTS: the caller knows that no row of the wave has more than NIT neighbours (the
// 15-slot records of unstructured meshes: 11 slots cover ~94 % of the waves of a Delaunay mesh).
template <typename T, int SLOTS, bool MASS, bool DETS, int NIT = SLOTS>
__device__ __forceinline__ void ring_row(const RingArgs<T> &a, const RingRec<SLOTS> &rec,
                                         uint32_t lv, const T *xy, T (&off)[SLOTS + 1], T &diag,
                                         T (&sdets)[SLOTS]) {
  const int k = rec.k();
  T xv, yv, px, py;
  lds_xy(xy, lv, xv, yv);
  const uint32_t id0 = rec.id(0);
  lds_xy(xy, id0, px, py);
  T ecx = px - xv, ecy = py - yv;
  T qc = ecx * ecx + ecy * ecy;
  T dsum = T(0);  // sum of the signed determinants around the vertex (mass part)
#pragma unroll
  for (int i = 0; i <= SLOTS; ++i) off[i] = T(0);
  if (DETS) {
#pragma unroll
    for (int i = NIT; i < SLOTS; ++i) sdets[i] = T(0);
  }
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    // neighbour behind slot i: slot i + 1, or slot 0 where the fan closes
    const uint32_t idn = (i + 1 < SLOTS && i + 1 != k) ? rec.id(i + 1 < SLOTS ? i + 1 : 0) : id0;
    lds_xy(xy, idn, px, py);
    const T enx = px - xv, eny = py - yv;
    const T qn = enx * enx + eny * eny;
    const T p = ecx * enx + ecy * eny;
    const T cross = ecx * eny - ecy * enx;  // +- the signed determinant (element_tri.py:139)
    const uint32_t flag = rec.flag(i);      // 0 for every slot i >= k
    const T cs = flag_weight<T>(a.stiff_w, flag) * fast_rcp<T>(flag ? cross : T(1));
    off[i] = off[i] + cs * (p - qn);
    off[i + 1] = off[i + 1] + cs * (p - qc);
    if (MASS || DETS) {
      const T sdet = flag_weight<T>(T(1), flag) * cross;  // signed determinant, 0 without triangle
      if (DETS) sdets[i] = sdet;
      if (MASS) {
        const T m = a.mass_o * sdet;
        off[i] = off[i] + m;
        off[i + 1] = off[i + 1] + m;
        dsum = dsum + sdet;
      }
    }
    ecx = enx;
    ecy = eny;
    qc = qn;
  }
  // the closing triangle's second entry sits in off[k]: it belongs to slot 0
  T wrapv = off[1];
#pragma unroll
  for (int j = 2; j <= SLOTS; ++j) wrapv = k == j ? off[j] : wrapv;
  T sum = off[0];
#pragma unroll
  for (int j = 1; j <= SLOTS; ++j) sum = sum + off[j];  // = sum_{j<k} off[j] + wrapv (once)
  off[0] = off[0] + wrapv;
  diag = ring_diag<T, MASS>(sum, dsum, a.mass_d, a.mass_o);
}

// ring_row for a REGULAR row: six neighbours, six triangles, all of them stored counter-clockwise
// around the vertex (record: k = 6, flags 1 1 1 1 1 1 0) -- the interior vertices of a structured
// mesh.  No flag arithmetic, no selection of the closing neighbour; the same operations in the
// same order as ring_row otherwise (bitwise the same entries).  7-slot records only.
template <typename T, bool MASS>
__device__ __forceinline__ void ring_row_regular(const RingArgs<T> &a, const RingRec<7> &rec, uint32_t lv,
                                                 const T *xy, T (&off)[8], T &diag) {
  T xv, yv, px, py;
  lds_xy(xy, lv, xv, yv);
  lds_xy(xy, rec.id(0), px, py);
  const T e0x = px - xv, e0y = py - yv;
  const T q0 = e0x * e0x + e0y * e0y;
  T ecx = e0x, ecy = e0y, qc = q0;
  T dsum = T(0), wrapv = T(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) off[i] = T(0);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    T enx = e0x, eny = e0y, qn = q0;
    if (i < 5) {
      lds_xy(xy, rec.id(i + 1), px, py);
      enx = px - xv;
      eny = py - yv;
      qn = enx * enx + eny * eny;
    }
    const T p = ecx * enx + ecy * eny;
    const T cross = ecx * eny - ecy * enx;
    const T cs = a.stiff_w * fast_rcp<T>(cross);
    T &behind = i < 5 ? off[i + 1] : wrapv;  // the neighbour behind the triangle (ring_row: off[6] for the last)
    off[i] = off[i] + cs * (p - qn);
    behind = behind + cs * (p - qc);
    if (MASS) {
      const T m = a.mass_o * cross;
      off[i] = off[i] + m;
      behind = behind + m;
      dsum = dsum + cross;
    }
    ecx = enx;
    ecy = eny;
    qc = qn;
  }
  T sum = off[0];
#pragma unroll
  for (int j = 1; j < 6; ++j) sum = sum + off[j];
  sum = (sum + wrapv) + T(0);  // off[6] = wrapv, off[7] = 0 in ring_row's sum
  off[0] = off[0] + wrapv;
  diag = ring_diag<T, MASS>(sum, dsum, a.mass_d, a.mass_o);
}

// What ring_long_slot hands back to its lane.
template <typename T>
struct RingLongSlot {
  const uint32_t *rec;  // the row's record
  uint32_t v;           // the row's vertex (global id)
  int i;                // the lane's slot
  int dpos;             // position of the diagonal in the row's CSR values
  bool live, slot;      // the row exists; slot i is one of its k neighbours
  T entry;              // K[v][n_i] (slots only)
  T sum, dsum;          // over the row's sixteen lanes: entries, signed determinants (ring_diag)
  T prod;               // PROD: over the row's sixteen lanes, entry * u[n_i]
};

// One lane of a long row (plans with long rows, tfem_rings_host.cpp: 24-dword records of the
// vertices with 8 .. 15 neighbours): SIXTEEN lanes per row, lane i = slot i of the fan,
// coordinates by global ids.  The lane evaluates its slot's triangle (ring_row's formulas) and
// takes what the previous slot's triangle adds to its own column from the lane before it (slot 0
// from slot k - 1); the diagonal follows from the sums over the sixteen lanes (ring_diag).
// k_p1_long_rows stores the entries; k_p1_apply_long_rows (PROD) also sums entry * u of the
// column over the sixteen lanes, in the same pass.  `s` is filled in place rather than returned:
// with a returned struct the long-row kernels took more VGPRs than before.
template <typename T, bool MASS, bool PROD>
__device__ __forceinline__ void ring_long_slot(const T *coords, const unsigned char *plan, unsigned off_long,
                                               int n_long, T stiff_w, T mass_o, const T *u, RingLongSlot<T> &s) {
  const int gtid = int(blockIdx.x) * kRingBlock + int(threadIdx.x);
  const int row = gtid >> 4, i = gtid & 15;
  s.i = i;
  s.live = row < n_long;
  const uint32_t *rec = reinterpret_cast<const uint32_t *>(plan + off_long) + 24 * size_t(s.live ? row : 0);
  s.rec = rec;
  const uint32_t v = rec[0];
  s.v = v;
  const int k = int(rec[2] & 0xFFu);
  s.dpos = int(rec[2] >> 8);
  s.slot = s.live && i < k;
  const uint32_t flag = s.slot ? (rec[3] >> (2 * i)) & 3u : 0u;
  const int nxt = i + 1 == k ? 0 : i + 1;
  const uint32_t g0 = rec[4 + (s.slot ? i : 0)], g1 = rec[4 + (s.slot ? nxt : 0)];
  const T xv = coords[2 * size_t(v)], yv = coords[2 * size_t(v) + 1];
  const T ecx = coords[2 * size_t(g0)] - xv, ecy = coords[2 * size_t(g0) + 1] - yv;
  const T enx = coords[2 * size_t(g1)] - xv, eny = coords[2 * size_t(g1) + 1] - yv;
  const T qc = ecx * ecx + ecy * ecy, qn = enx * enx + eny * eny;
  const T p = ecx * enx + ecy * eny;
  const T cross = ecx * eny - ecy * enx;
  const T cs = flag_weight<T>(stiff_w, flag) * fast_rcp<T>(flag ? cross : T(1));
  T here = cs * (p - qn), next = cs * (p - qc);  // to column n_i, to column n_next
  T sdet = T(0);
  if (MASS) {
    sdet = flag_weight<T>(T(1), flag) * cross;
    here = here + mass_o * sdet;
    next = next + mass_o * sdet;
  }
  const int lane = int(threadIdx.x) & 63;
  const int from = (lane & ~15) + (i == 0 ? (k > 0 ? k - 1 : 0) : i - 1);
  s.entry = here + __shfl(next, from, 64);
  s.sum = here + next;
  s.dsum = sdet;
  s.prod = (PROD && s.slot) ? s.entry * u[g0] : T(0);
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {
    s.sum = s.sum + __shfl_xor(s.sum, m, 64);
    if (MASS) s.dsum = s.dsum + __shfl_xor(s.dsum, m, 64);
    if (PROD) s.prod = s.prod + __shfl_xor(s.prod, m, 64);
  }
}

// Per-wave LDS stage: the wave's CSR entries, compact and in CSR order (row r of the wave
// starts at the exclusive prefix sum of the row lengths).  Two spare entries behind the
// 64 * (SLOTS + 1) real ones absorb the slots a row does not have, so staging has no branches.
template <typename T, int SLOTS>
constexpr int ring_stage_entries() { return 64 * (SLOTS + 1) + 2; }

// Row entries -> the wave's stage (plain LDS stores).  `pre` = stage index of this lane's row;
// returns the number of entries the wave staged (uniform).
template <typename T, int SLOTS, int NIT = SLOTS>
__device__ __forceinline__ int ring_stage(const RingRec<SLOTS> &rec, const T (&off)[SLOTS + 1], T diag,
                                          T *stage, int &pre) {
  const int k = rec.k();
  const int len = k > 0 ? k + 1 : 0;
  const int incl = wave_inclusive_scan(len);
  pre = incl - len;
  constexpr int kSpare = 64 * (SLOTS + 1);
#pragma unroll
  for (int i = 0; i < NIT; ++i) stage[i < k ? pre + rec.pos(i) : kSpare] = off[i];
  stage[k > 0 ? pre + rec.dpos() : kSpare] = diag;
  return __builtin_amdgcn_readlane(incl, 63);
}

// ring_stage for a wave of regular rows (ring_row_regular): every row has seven entries, so row r
// of the wave starts at 7 r -- no scan, no tests (lanes without a row sit behind the last row and
// write behind `total`, which nothing reads).
template <typename T>
__device__ __forceinline__ int ring_stage_regular(const RingRec<7> &rec, const T (&off)[8], T diag, T *stage,
                                                  int &pre, int n_rows) {
  pre = 7 * int(threadIdx.x & 63);
#pragma unroll
  for (int i = 0; i < 6; ++i) stage[pre + rec.pos(i)] = off[i];
  stage[pre + rec.dpos()] = diag;
  return 7 * n_rows;
}

// The wave's stage -> global memory when the wave's rows form ONE run (a group of rows that is
// contiguous in the CSR value array): stage index + delta = CSR index for the whole wave.
// Lane j of step u takes entries 128 u + 2 j and the next one: 16-byte stores, 1 KiB
// contiguous per wave instruction; whole steps need no per-lane test.  Every LDS read is
// issued first (one LDS latency per tile).  Same wave as ring_stage: LDS executes a wave's
// operations in order.
template <typename T, int SLOTS>
__device__ __forceinline__ void ring_store_run1(const T *stage, int total, int delta, ring_rsrc_t r_vals,
                                                int plain_stores) {
  const int lane = threadIdx.x & 63;
  constexpr int kSteps = 64 * (SLOTS + 1) / 128;
  T va[kSteps][2];
#pragma unroll
  for (int u = 0; u < kSteps; ++u) {
    // 15-slot stage: rows hold ~7 of 16 entries, the steps behind `total` are skipped (uniform)
    if (SLOTS > 7 && u >= 2 && 128 * u >= total) {
      va[u][0] = va[u][1] = T(0);
      continue;
    }
    va[u][0] = stage[128 * u + 2 * lane];
    va[u][1] = stage[128 * u + 2 * lane + 1];
  }
#pragma unroll
  for (int u = 0; u < kSteps; ++u) {
    if (SLOTS > 7 && u >= 2 && 128 * u >= total) continue;
    const int s0 = 128 * u + 2 * lane;
    const unsigned byte = unsigned(s0 + delta) * unsigned(sizeof(T));
    const T v0 = va[u][0], v1 = va[u][1];
    if (128 * (u + 1) <= total || s0 + 1 < total) {  // first test is wave-uniform
      if constexpr (sizeof(T) == 8) {
        const ru32x2 x = __builtin_bit_cast(ru32x2, v0), y = __builtin_bit_cast(ru32x2, v1);
        if (plain_stores & 1)  // plain (temporal) stores: the launch's store policy (RingArgs::plain_stores)
          __builtin_amdgcn_raw_buffer_store_b128(ru32x4{x.x, x.y, y.x, y.y}, r_vals, byte, 0, 0);
        else
          __builtin_amdgcn_raw_buffer_store_b128(ru32x4{x.x, x.y, y.x, y.y}, r_vals, byte, 0, kStreamNT);
      } else {
        __builtin_amdgcn_raw_buffer_store_b64(
            ru32x2{__builtin_bit_cast(unsigned, v0), __builtin_bit_cast(unsigned, v1)}, r_vals, byte, 0, kStreamNT);
      }
    } else if (s0 < total) {
      if constexpr (sizeof(T) == 8)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, v0), r_vals, byte, 0, kStreamNT);
      else
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v0), r_vals, byte, 0, kStreamNT);
    }
  }
}

// ring_store_run1 through a descriptor of the run's own (the SEP instantiations, consecutive-vertex tiles,
// 7-slot records; fp64): `r_run` starts at the run's first CSR entry and is as long as the run's whole PAIRS
// of entries (8 * (total & ~1) bytes, clipped to the array's end by the caller), so lane j of step u stores
// its pair at 16 j + 1024 u, four launch constants, and the range check drops the lanes behind the run: no
// offset arithmetic, no test, one 16-byte LDS read per step (the stage of a wave starts on 16 bytes).  An odd
// run (7 x an odd number of rows) ends in a lone entry, which is in no pair: it goes through a descriptor of
// its own (last_rsrc(), formed behind the wave-uniform test), which only lane 0's offset is inside.
template <typename T, typename LastRsrc>
__device__ __forceinline__ void ring_store_run1_desc(const T *stage, int total, ring_rsrc_t r_run, unsigned lane_b16,
                                                     LastRsrc last_rsrc, int plain_stores) {
  static_assert(sizeof(T) == 8, "pairs of doubles");
  typedef T stage_pair __attribute__((ext_vector_type(2)));
  const stage_pair *pairs = reinterpret_cast<const stage_pair *>(stage) + (threadIdx.x & 63);
  constexpr int kSteps = 64 * 8 / 128;  // 7-slot records
  stage_pair va[kSteps];
#pragma unroll
  for (int u = 0; u < kSteps; ++u) va[u] = pairs[64 * u];
  // the launch's store policy (RingArgs::plain_stores), asked once for all steps
  if (plain_stores & 1) {
#pragma unroll
    for (int u = 0; u < kSteps; ++u)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ru32x4, va[u]), r_run, lane_b16 + unsigned(1024 * u), 0,
                                             0);
  } else {
#pragma unroll
    for (int u = 0; u < kSteps; ++u)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ru32x4, va[u]), r_run, lane_b16 + unsigned(1024 * u), 0,
                                             kStreamNT);
  }
  if (total & 1)  // eight bytes long: 16 j is inside for lane 0 alone
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, stage[total - 1]), last_rsrc(), lane_b16, 0,
                                          kStreamNT);
}

// One run per wave EXCEPT for long rows (plans of unstructured meshes: vertices with 8 .. 15
// neighbours are written by k_p1_long_rows): their entries are not in the stage, the rows behind
// them start further on in the CSR array.  `pre` = stage index of the lane's row, `csr` = CSR
// offset of the lane's row; the stage is streamed out piece by piece between the long rows.
template <typename T>
__device__ __forceinline__ void ring_store_pieces(const T *stage, int total, int pre, int csr, bool is_long,
                                                  ring_rsrc_t r_vals) {
  const int lane = threadIdx.x & 63;
  unsigned long long holes = __ballot(is_long);
  int first_lane = 0;
  for (;;) {
    const int stop_lane = holes ? __builtin_ctzll(holes) : 64;
    if (first_lane < stop_lane) {
      const int b = __builtin_amdgcn_readlane(pre, first_lane);
      const int e = stop_lane < 64 ? __builtin_amdgcn_readlane(pre, stop_lane) : total;
      const int delta = __builtin_amdgcn_readlane(csr, first_lane) - b;
      for (int s0 = b + lane; s0 < e; s0 += 64) {
        const unsigned byte = unsigned(s0 + delta) * unsigned(sizeof(T));
        if constexpr (sizeof(T) == 8)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, stage[s0]), r_vals, byte, 0, kStreamNT);
        else
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, stage[s0]), r_vals, byte, 0, kStreamNT);
      }
    }
    if (!holes) break;
    holes &= holes - 1;
    first_lane = stop_lane + 1;
  }
}

// General form: the rows of a wave form several runs (one per grid line of a Z-order tile;
// one per row for a numbering without locality).  Per run, as above.
template <typename T, int SLOTS>
__device__ __forceinline__ void ring_store(const T *stage, int total, int pre, int rowstart, int len,
                                           ring_rsrc_t r_vals, int plain_stores) {
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_wave_barrier();
  // A row starts a run when the rows since the previous non-empty row are not one contiguous
  // piece of the CSR array.  `breaks` = lanes whose row does not begin where the row of lane
  // r - 1 ends (wave_shr:1; rows without entries -- isolated vertices -- take part with their
  // offset: an empty row between two pieces must not glue them together).
  const int prev_end = __builtin_amdgcn_update_dpp(-1, rowstart + len, 0x138, 0xF, 0xF, false);
  const unsigned long long has_row = __ballot(len > 0);
  const unsigned long long breaks = __ballot(prev_end != rowstart);
  const unsigned long long below = (1ull << lane) - 1ull;           // lanes < this one
  const unsigned long long ne_below = has_row & below;
  // lanes in (previous non-empty lane, this lane]
  const unsigned long long since = ne_below ? ~((2ull << (63 - __builtin_clzll(ne_below))) - 1ull) : ~0ull;
  const bool start = len > 0 && ((breaks & since & (below | (1ull << lane))) != 0ull || ne_below == 0ull);
  unsigned long long starts = __ballot(start);
  if ((starts & (starts - 1)) == 0) {
    const int delta = starts ? __builtin_amdgcn_readlane(rowstart, __builtin_ctzll(starts)) : 0;
    ring_store_run1<T, SLOTS>(stage, total, delta, r_vals, plain_stores);
    __builtin_amdgcn_wave_barrier();
    return;
  }
  while (starts) {
    const int r = __builtin_ctzll(starts);
    starts &= starts - 1;
    const int b = __builtin_amdgcn_readlane(pre, r);
    const int delta = __builtin_amdgcn_readlane(rowstart, r) - b;
    const int e = starts ? __builtin_amdgcn_readlane(pre, __builtin_ctzll(starts)) : total;
    for (int s0 = b + 2 * lane; s0 - 2 * lane < e; s0 += 128) {
      const T v0 = stage[s0], v1 = stage[s0 + 1];
      const unsigned byte = unsigned(s0 + delta) * unsigned(sizeof(T));
      if (s0 + 1 < e) {
        if constexpr (sizeof(T) == 8) {
          const ru32x2 x = __builtin_bit_cast(ru32x2, v0), y = __builtin_bit_cast(ru32x2, v1);
          __builtin_amdgcn_raw_buffer_store_b128(ru32x4{x.x, x.y, y.x, y.y}, r_vals, byte, 0, kStreamNT);
        } else {
          __builtin_amdgcn_raw_buffer_store_b64(
              ru32x2{__builtin_bit_cast(unsigned, v0), __builtin_bit_cast(unsigned, v1)}, r_vals, byte, 0, kStreamNT);
        }
      } else if (s0 < e) {
        if constexpr (sizeof(T) == 8)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, v0), r_vals, byte, 0, kStreamNT);
        else
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v0), r_vals, byte, 0, kStreamNT);
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

template <int SLOTS>
__device__ __forceinline__ void ring_load_rec(ring_rsrc_t r, unsigned byte, RingRec<SLOTS> &rec) {
  const ru32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, byte, 0, kStreamLoadNT);
  rec.w[0] = v.x;
  rec.w[1] = v.y;
  rec.w[2] = v.z;
  rec.w[3] = v.w;
  if constexpr (SLOTS == 15) {
    const ru32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, byte + 16u, 0, kStreamLoadNT);
    rec.w[4] = u.x;
    rec.w[5] = u.y;
    rec.w[6] = u.z;
    rec.w[7] = u.w;
  }
}

// What one WAVE needs of a tile descriptor (20 ints, tfem_rings_host.cpp): the wave owns the
// tile's rows [row0, row1), at most 64.  In a plan with consecutive-vertex tiles those rows
// are the consecutive vertices gid0, gid0 + 1, ... and their CSR entries start at rs0: neither
// the ids of the owned vertices nor the row offsets are read from memory.  Scalar loads with a
// wave-uniform index (the plan is immutable during the launch: constant address space).
struct RingDesc {
  int vert_off, n_vert, row_off, n_own, row0, row1, gid0, rs0, elem_off, n_elem, elem_mode, tvert_off;
  int n_tv;  // elements the tile evaluates itself (source programs)
};
constexpr int kRingElemRuns = 8;  // desc[18] = 1: the tile's elements are <= 8 runs of consecutive ids

template <bool CHUNK>
__device__ __forceinline__ RingDesc ring_desc(const unsigned char *plan, unsigned off_desc, int tile,
                                              int wave) {
  ring_const_i32 d = (ring_const_i32)(uintptr_t)(plan + off_desc + 80u * unsigned(tile));
  RingDesc r{d[0], d[1], d[2], d[7], d[3 + wave], d[4 + wave], 0, 0, d[16], d[17], d[18] & 0xFF, d[19], d[18] >> 8};
  if (CHUNK) {
    r.gid0 = d[8 + wave];
    r.rs0 = d[12 + wave];
  }
  return r;
}

// ---------------------------------------------------------------------------------------
// Persistent, pipelined kernel: workgroups stay resident and walk a strided list of tiles
// inside their XCD's piece of the curve (workgroup b: XCD b & 7, so every XCD -- own L2 --
// walks one contiguous piece and neighbouring tiles share their halo coordinates in that L2).
// Every lane owns one row; it also fetches the coordinates of its row's vertex and of one halo
// vertex of the tile.  Iteration k (tile k: record and row offset in registers, coordinates in
// xy[k & 1]):
//   A  issue the loads of tile k+1 (row record, row offset, coordinates by the vertex ids that
//      arrived during iteration k-1) and the vertex ids of tile k+2
//   B  rows of tile k: LDS reads, arithmetic, entries -> the wave's stage
//   C  s_waitcnt vmcnt(0): the loads of A were issued a whole row phase ago, the stores of
//      tile k-1 a whole iteration ago
//   D  coordinates of tile k+1 -> xy[(k+1) & 1]; stage -> global stores of tile k
//   E  LDS barrier (the only one): xy[(k+1) & 1] is complete, nobody reads xy[k & 1] any more
// Neither a load's latency nor a store's acknowledgement is waited for inside an iteration.
// The fp64 launches of a source program on the wide interpreter (kCoordsToLds) fetch the coordinates differently: the loads
// of tile k+1 are issued at the top of iteration k, in front of phase G, and write xy[(k+1) & 1]
// themselves (16 bytes per lane, buffer_load ... lds) -- no register holds them, D copies nothing.
// ---------------------------------------------------------------------------------------
constexpr int kRingHaloCap = kRingBlock;  // halo vertices per tile: one per lane
constexpr int kRingElemPerLane = 3;       // elements staged per tile <= 3 * kRingBlock

__device__ __forceinline__ void ring_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

constexpr int kFqLoadNT = 0;  // cache policy of the source-value loads: plain, like kStreamLoadNT
// Q source values of one element (load vector): 16-byte loads where the type allows.
template <typename T, int QL>
__device__ __forceinline__ void ring_load_fq(ring_rsrc_t r, unsigned byte, T (&v)[QL > 0 ? QL : 1]) {
#pragma unroll
  for (int q = 0; q + 1 < QL; q += 2) {
    if constexpr (sizeof(T) == 8) {
      const ru32x4 x = __builtin_amdgcn_raw_buffer_load_b128(r, byte + unsigned(q) * 8u, 0, kFqLoadNT);
      v[q] = __builtin_bit_cast(double, ru32x2{x.x, x.y});
      v[q + 1] = __builtin_bit_cast(double, ru32x2{x.z, x.w});
    } else {  // two dword loads: raw_buffer_load_b64 is miscompiled by this hipcc (tfem_tiles.hip)
      v[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte + unsigned(q) * 4u, 0, 0));
      v[q + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte + unsigned(q) * 4u + 4u, 0, 0));
    }
  }
  if (QL & 1) {
    const unsigned o = byte + unsigned(QL - 1) * unsigned(sizeof(T));
    if constexpr (sizeof(T) == 8) {
      const unsigned lo = __builtin_amdgcn_raw_buffer_load_b32(r, o, 0, 0);
      const unsigned hi = __builtin_amdgcn_raw_buffer_load_b32(r, o + 4u, 0, 0);
      v[QL > 0 ? QL - 1 : 0] = __builtin_bit_cast(double, ru32x2{lo, hi});
    } else {
      v[QL > 0 ? QL - 1 : 0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, o, 0, 0));
    }
  }
}

// QL = 0: matrix only.  QL = Q > 0: the launch also forms the load vector
//   f_v = sum over the triangles T of the fan  det_T * g[T][loc],
//   g[T][i] = sum_q fq[T][q] l_i(q) w_q / 2
// (abstract_basis.py:95-112 with basis.py:93-96).  The source values of a tile's elements
// (plan: tile_elems, ascending) are fetched ONCE per tile with coalesced 16-byte loads -- three
// elements per lane, prefetched like the coordinates -- reduced to the three numbers g[T][.]
// and staged in LDS; a row reads one of them per fan slot by the slot's
// 12-bit code (tile-local element | loc << 10).  (Gathering the Q values per row and slot
// instead is bound by the texture addresser: 14 scattered loads per row.)
// SRC (1: any program, one element per pass of the interpreter; 2: programs that hold at most two
// values, three elements per pass): the source values are not read from memory but computed in the launch from the program
// in RingArgs::src: per tile element the three tile-local vertex ids arrive with the plan
// (tile_tverts, 4 bytes instead of 8 Q), the integration points are formed from the
// coordinates the tile holds in LDS anyway, f is evaluated there (tfem_source.hpp) and reduced
// to g[T][.] as above.  That happens at the START of the tile's iteration (its coordinates are
// complete after the previous iteration's barrier), behind the issue of the next tile's loads.
// SEP (the sixth parameter, with KMAT and SRC behind it at positions 6 and 7 of the demangled kernel
// name, where bench.py finds the bench launches in the committed profiles): the program is a separable
// one, k U(a x) V(b y) with proven sines / cosines (host: src_is_separable), and phase G evaluates it in
// straight-line code -- no interpreter in the kernel (fp64, Q = 4, SRC = 2 only).
template <typename T, int SLOTS, bool MASS, bool CHUNK, int QL, bool SEP, bool KMAT = true, int SRC = 0>
// The matrix-only 15-slot instantiations are asked for 3 waves per SIMD: left alone, hipcc's
// scheduler hoists every LDS read of the unrolled fan loop and ends at 250 VGPRs (2 waves); with
// the bound it needs 112-128 and nothing spills (the load-vector instantiations would spill).
__global__ __launch_bounds__(kRingBlock, (SRC && SLOTS == 7 && QL <= 4) ? 4 : (SLOTS > 7 && QL == 0) ? 3 : 1) void k_p1_rings(const RingArgs<T> a) {
  constexpr bool LOAD = QL > 0;
  constexpr bool FQ = LOAD && !SRC;  // source values streamed from memory
  // fp64 source programs of the wide interpreter: a lane's coordinate pair is 16 bytes, which a buffer
  // load can write to LDS itself (float32: 8 bytes, a size the LDS form does not have -- those keep the
  // register path; so does the general interpreter, SRC = 1, whose launches were measured 2 % SLOWER
  // with it: 264 -> 270 us for a depth-3 program at 1e7 elements, profiles/fused_lds_direct.log)
  constexpr bool kCoordsToLds = SRC == 2 && sizeof(T) == 8;
  static_assert(KMAT || LOAD, "nothing to assemble");
  static_assert(LOAD || !SRC, "a source program needs a load vector");
  static_assert(!SEP || (SRC == 2 && QL == 4 && sizeof(T) == 8), "the separable form: fp64, four points, wide passes");
  constexpr int kEW = (12 * SLOTS + 31) / 32;  // dwords of packed 12-bit slot codes per row: 3 or 6
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_smem[];
  T *xy = reinterpret_cast<T *>(ring_smem);                      // [2][2 * lds_vert]
  T *stage = xy + 4 * a.lds_vert;                                // [waves][stage entries]
  // [3 * lds_elem + 4]; the load-vector-only instantiation has no stage
  T *gtab = stage + (KMAT ? kRingWaves * ring_stage_entries<T, SLOTS>() : 0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  T *my_stage = stage + wave * ring_stage_entries<T, SLOTS>();
  // tiles per XCD, a whole number of blocks when the tile list is dealt in blocks
  const int deal = a.xcd_interleave > 0 ? a.xcd_interleave : 1;
  const int per = (a.n_tiles + 8 * deal - 1) / (8 * deal) * deal;
  const int xcd = blockIdx.x & 7;
  const int j0 = blockIdx.x >> 3;
  const int stride = gridDim.x >> 3;
  // SRC: positions of the plan's chain order instead of tile numbers.  Blocks of chain_len
  // positions (aligned to multiples of chain_len in the plan's order, whatever range the launch
  // takes: the plan hands shares over inside such blocks) are dealt to the XCDs round-robin; a
  // workgroup takes the positions of a block one after the other.
  const int clen = SRC ? a.chain_len : 1;
  const int u_end = a.u_first + a.n_tiles;
  const int block0 = SRC ? a.u_first / clen : 0;
  // kTileDesc (the SEP instantiations): per-tile buffer descriptors for the plan loads of the tile loop, below.
  // The plan and its length as the tile loop knows them: the kernel argument's, which these instantiations
  // read again behind every phase G -- whatever reads the plan in the loop takes these (plan_now), so that the
  // argument's own copy is not a second pointer alive across G.  Every other instantiation reads a.plan as before.
  constexpr bool kTileDesc = SEP;
  const unsigned char *plan_at = a.plan;
  unsigned plan_room = a.plan_bytes;
  T *vals_at = a.vals;  // the same for the value array (run_rsrc, below)
  unsigned vals_room = a.vals_bytes;
  // ... and for the store policy: asked of the argument itself, the answer is a launch constant that hipcc keeps
  // in a scalar pair through G, at the price of two spilled scalars
  int plain_now = a.plain_stores;
  auto plan_now = [&]() {
    if constexpr (kTileDesc)
      return plan_at;
    else
      return a.plan;
  };
  // SRC, runs: the workgroup takes runs blockIdx, blockIdx + gridDim, ... of the plan's run list (with
  // gridDim = the number of runs: its own one) and walks their positions one after the other
  const bool balanced = SRC && a.n_runs > 0;
  int run = int(blockIdx.x) - int(gridDim.x), run_at = 0, run_end = 0;
  auto next_position = [&]() {  // -1: the workgroup's share is done
    while (run_at == run_end) {
      run += int(gridDim.x);
      if (run >= a.n_runs) return -1;
      ring_const_i32 first = (ring_const_i32)(uintptr_t)(plan_now() + a.off_runs);
      run_at = first[run];
      run_end = first[run + 1];
    }
    return run_at++;
  };
  auto tile_at = [&](int k) {
    if constexpr (SRC != 0) {
      ring_const_i32 order = (ring_const_i32)(uintptr_t)(plan_now() + a.off_chain);
      if (balanced) {  // called with k = 0, 1, 2, ...: the positions in the workgroup's order
        const int u = next_position();
        return u < 0 ? -1 : __builtin_amdgcn_readfirstlane(order[u]);
      }
      // the workgroup of the launch's first block starts inside it when the range does
      const int k2 = k + ((xcd == 0 && j0 == 0) ? a.u_first - block0 * clen : 0);
      const int kb = k2 / clen, ki = k2 - kb * clen;
      const int u = (block0 + (j0 + kb * stride) * 8 + xcd) * clen + ki;
      if (u >= u_end) return -1;
      return __builtin_amdgcn_readfirstlane(order[u]);
    } else {
      const int j = j0 + k * stride;
      const int g = a.xcd_interleave;
      const int t = g ? ((j / g) * 8 + xcd) * g + j % g : xcd * per + j;
      return __builtin_amdgcn_readfirstlane((j < per && t < a.n_tiles) ? t : -1);
    }
  };
  // (not const: the SEP instantiations form them anew behind every phase G)
  ring_rsrc_t r_coords = ring_rsrc(a.coords, a.coords_bytes);
  ring_rsrc_t r_plan = ring_rsrc(a.plan, a.plan_bytes);
  ring_rsrc_t r_vals = ring_rsrc(a.vals, a.vals_bytes);
  const ring_rsrc_t r_fq = ring_rsrc(a.fq, a.fq_bytes);
  ring_rsrc_t r_fout = ring_rsrc(a.fout, a.fout_bytes);
  constexpr unsigned kRecBytes = unsigned(4 * RingRec<SLOTS>::kWords);
  constexpr unsigned kNone = 0x3FFFFFFu;  // row / vertex index behind every array: loads give 0
  // kTileDesc: the plan loads of a tile go through descriptors of their own, formed per tile and stream
  // from wave-uniform values on the scalar unit: the base is the first entry the WAVE
  // reads, num_records the number of entries it may read times their size.  A lane's offset is then a
  // launch constant (lane * entry size; the elements 256 and 512 further on ride in the instruction's
  // immediate offset) and a lane past the count is out of range by itself -- it receives zeros from the
  // same range check that `kNone` relies on, without the add, compare, select and scale per load that
  // moved it there.  Only voffset and the immediate take part: soffset stays 0.
  // tile_rsrc: `count` entries of `size` bytes, the first one `first` entries into the plan section at byte `off`;
  // clipped to the plan's end (nothing behind it is readable, as with r_plan), empty for count <= 0
  // (signed minimum and maximum: the scalar unit has both, while the saturating unsigned subtraction hipcc
  // makes of `room > at ? room - at : 0` exists on the vector unit only and turns every load that uses the
  // descriptor into a waterfall loop; the plan is shorter than 2^31 bytes, tfem_ring_plan_build)
  auto tile_rsrc = [&](unsigned off, int first, int count, int size) {
    const unsigned at = off + unsigned(first * size);
    const int room = int(plan_room - at), want = count * size;
    const int fits = want < room ? want : room;
    return ring_rsrc(plan_at + at, unsigned(fits > 0 ? fits : 0));
  };
  // run_rsrc: the same for a wave's run of CSR values, `count` entries from entry `first` of the value array.  The
  // array may be longer than 2^31 bytes (the launch admits 2^32) but not than 2^31 entries, so the clipping is
  // done in entries, with the signed minimum and maximum of tile_rsrc (an unsigned compare and select of byte
  // counts came out as a vector subtraction with borrow, and the stores in waterfall loops); a run that starts
  // behind the array's end is empty.
  auto run_rsrc = [&](T *vals, unsigned vals_room, int first, int count) {
    const int at = first > 0 ? first : 0;  // (nothing in front of the array either, whatever the plan says)
    const int room = int(vals_room / unsigned(sizeof(T))) - at;
    const int fits = count < room ? count : room;
    return ring_rsrc(reinterpret_cast<unsigned char *>(vals) + unsigned(at) * unsigned(sizeof(T)),
                     unsigned(fits > 0 ? fits : 0) * unsigned(sizeof(T)));
  };
  const unsigned lane_b2 = unsigned(lane) * 2u, lane_b4 = unsigned(lane) * 4u, lane_b16 = unsigned(lane) * 16u;
  if (FQ && tid < 4)  // the spare entries slots without a triangle read (times a zero determinant)
    gtab[3 * a.lds_elem + tid] = T(0);
  // SRC: the same LDS region holds the load-vector accumulators: THREE buffers (tile number modulo
  // 3) of one sum per tile-LOCAL vertex, halo included, + one entry that stays zero.  A tile adds
  // every share of every element it evaluates to the sum of the element's vertex -- no test, no
  // table.  A row takes its own sum from its tile's buffer and, when the tile before it in the chain
  // block evaluated elements of its fan (an element shared by consecutive tiles of a block is
  // evaluated by the earlier one only), what that tile summed for its vertex from the PREVIOUS
  // tile's buffer (plan: hand_in, the vertex's local id there).  A buffer is zeroed two tiles
  // after it was filled: behind the barrier that ends the iteration of the last tile reading it.
  const int acc_stride = a.lds_vert + 2;
  T *accs = gtab;  // [3][acc_stride]
  if (SRC)
    for (int i = tid; i < 3 * acc_stride; i += kRingBlock) accs[i] = T(0);

  // SRC: the program, one operation per lane, for the whole launch
  // (SEP: no lanes, what the passes need of the program are its two push constants and three bits)
  SrcLanes<T> prog;
  if constexpr (SRC && !SEP) prog = src_load_lanes<T>(src_in_kernarg<T>(__builtin_offsetof(RingArgs<T>, src)));
  int sep_flags = 0;
  if constexpr (SEP) sep_flags = src_separable_flags<T>(src_in_kernarg<T>(__builtin_offsetof(RingArgs<T>, src)));
  RingRec<SLOTS> rec, rec_ld;
  uint32_t se[FQ ? kEW : 1], se_ld[FQ ? kEW : 1];  // slot codes of the row (load vector from fq)
  unsigned eid[FQ ? kRingElemPerLane : 1], eid_ld[FQ ? kRingElemPerLane : 1];  // element ids, like gid_*
  T fqe_ld[FQ ? kRingElemPerLane : 1][QL > 0 ? QL : 1];  // their source values
  unsigned tev[SRC ? kRingElemPerLane : 1], tev_ld[SRC ? kRingElemPerLane : 1];  // local vertex triples
  unsigned gid_row = 0;                                    // vertex of this lane's current row
  int rowstart = 0, rowstart_ld = 0;
  unsigned gid_own = 0, gid_halo = 0;        // vertex ids of the tile whose coordinates load next
  unsigned gid_own_ld = 0, gid_halo_ld = 0;  // ... and of the tile after it
  T own_ld[2], halo_ld[2];
  unsigned hin = 0xFFFFu, hin_ld = 0xFFFFu;  // hand-in of this lane's current row, of the next tile's

  // vertex ids of a tile: the lane's own row vertex and halo vertex number tid.  With
  // consecutive-vertex tiles the own id is arithmetic on the descriptor.
  auto load_ids = [&](const RingDesc &d, unsigned &g_own, unsigned &g_halo) {
    if constexpr (kTileDesc) {
      // CHUNK: no own id at all -- the coordinate load and the f store form their offsets from the
      // descriptor's gid0 where they are issued (one shift-add each), nothing rides along from tile to tile
      if (!CHUNK)
        g_own = __builtin_amdgcn_raw_buffer_load_b32(tile_rsrc(a.off_gid, d.vert_off + d.row0, d.row1 - d.row0, 4u),
                                                     lane_b4, 0, 0);
      // halo vertex n_own + tid: the wave's 64 start at n_own + 64 wave
      g_halo = __builtin_amdgcn_raw_buffer_load_b32(
          tile_rsrc(a.off_gid, d.vert_off + d.n_own + 64 * wave, d.n_vert - d.n_own - 64 * wave, 4u), lane_b4, 0, 0);
      return;
    }
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
  auto load_eids = [&](const RingDesc &d, unsigned (&e)[FQ ? kRingElemPerLane : 1]) {
    if (!FQ || d.elem_mode) return;  // runs of consecutive ids: nothing to fetch
#pragma unroll
    for (int j = 0; j < kRingElemPerLane; ++j) {
      const int l = tid + j * kRingBlock;
      e[FQ ? j : 0] = __builtin_amdgcn_raw_buffer_load_b32(
          r_plan, a.off_telems + (l < d.n_elem ? unsigned(d.elem_off + l) : kNone) * 4u, 0, 0);
    }
  };
  // source values of the tile's elements by the ids that arrived an iteration earlier (lanes
  // past the tile's last element carry the id 0 of the zero-filled load: harmless)
  auto load_fq = [&](const RingDesc &d, const unsigned (&e)[FQ ? kRingElemPerLane : 1]) {
    if (!FQ) return;
    if (d.elem_mode) {
      // position l in the tile's ascending element list -> id, from the first ids of the runs
      // and the list positions they end at (16 scalars of the plan)
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
        ring_load_fq<T, QL>(r_fq, l < d.n_elem ? unsigned(id) * unsigned(QL * sizeof(T)) : 0xFFFFFFF0u,
                            fqe_ld[FQ ? j : 0]);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < kRingElemPerLane; ++j) {
      const int l = tid + j * kRingBlock;
      ring_load_fq<T, QL>(r_fq, l < d.n_elem ? e[FQ ? j : 0] * unsigned(QL * sizeof(T)) : 0xFFFFFFF0u,
                          fqe_ld[FQ ? j : 0]);
    }
  };
  // g[T][i] = sum_q fq[T][q] l_i(q) w_q / 2 of the elements just loaded -> LDS
  auto park_g = [&](const RingDesc &d, T *dst) {
    if (!FQ) return;
#pragma unroll
    for (int j = 0; j < kRingElemPerLane; ++j) {
      const int l = tid + j * kRingBlock;
      if (l < d.n_elem) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          T g = T(0);
#pragma unroll
          for (int q = 0; q < QL; ++q) g = g + fqe_ld[FQ ? j : 0][q] * a.lamw[i][q];
          dst[3 * l + i] = g;
        }
      }
    }
  };
  // SRC: the packed local vertex ids of the tile's elements (zero-filled past the last one)
  // Which lanes take which elements of a tile's table ROTATES over the waves from tile to tile
  // (`rot` = number of the tile in the workgroup's sequence): wave w takes the elements
  // ((w + rot) & 3) * 64 + lane + 256 j.  A table of ~520 elements holds 8 in its third round, which
  // one wave sees; wave w of every workgroup sits on SIMD w, so without the rotation SIMD 0 would run
  // three rounds for every tile while the others run two.
  auto load_tverts = [&](const RingDesc &d, unsigned (&tv)[SRC ? kRingElemPerLane : 1], int rot) {
    if (!SRC) return;
    if constexpr (kTileDesc) {
      // the wave's elements start at 64 ((wave + rot) & 3); rounds 1 and 2 lie 1 and 2 KiB behind round 0
      const int first = ((wave + rot) & (kRingWaves - 1)) << 6;
      const ring_rsrc_t r_tv = tile_rsrc(a.off_tverts, d.tvert_off + first, d.n_tv - first, 4u);
#pragma unroll
      for (int j = 0; j < kRingElemPerLane; ++j)
        tv[SRC ? j : 0] =
            __builtin_amdgcn_raw_buffer_load_b32(r_tv, lane_b4 + unsigned(4 * j * kRingBlock), 0, kStreamLoadNT);
      return;
    }
    const int vtid = (((wave + rot) & (kRingWaves - 1)) << 6) + lane;
#pragma unroll
    for (int j = 0; j < kRingElemPerLane; ++j) {
      const int l = vtid + j * kRingBlock;
      tv[SRC ? j : 0] = __builtin_amdgcn_raw_buffer_load_b32(
          r_plan, a.off_tverts + (l < d.n_tv ? unsigned(d.tvert_off + l) : kNone) * 4u, 0, kStreamLoadNT);
    }
  };
  // SRC: det_T g[T][i], g[T][i] = sum_q f(x_q) l_i(q) w_q / 2, of the tile's elements from the
  // tile's coordinates in LDS (basis.py:90-91: x_q = bar(q)^T X), added to the accumulators of
  // the elements' vertices in LDS (element form: no slot codes, nothing per fan slot)
  // one share det_T g[T][i] -> the accumulator the tile's table names for local vertex `lid`
  auto add_share = [&](unsigned lid, T *acc, T v) { atomicAdd(acc + lid, v); };
  // NE elements per lane through the wide interpreter, then their shares
  auto compute_g_wide = [&](auto ne_tag, const RingDesc &d, const unsigned (&tv)[SRC ? kRingElemPerLane : 1],
                            const T *xyc, T *acc, int vtid) {
    constexpr int kNE = decltype(ne_tag)::value;
    unsigned codes[kNE];
#pragma unroll
    for (int j = 0; j < kNE; ++j) codes[j] = tv[SRC ? j : 0];
    T fv[kNE * (QL > 0 ? QL : 1)];
    // where the elements' vertices sit in LDS: formed once, for both coordinate pushes and the
    // determinants (3 kNE registers)
    const T *vert_at[kNE][3];
#pragma unroll
    for (int j = 0; j < kNE; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) vert_at[j][i] = xyc + 2 * __builtin_amdgcn_ubfe(codes[j], 10 * i, 10);
    // SEP: ONE batch of LDS reads per pass -- the six coordinates of every element serve both factors'
    // points and, further down, the determinants (the interpreter fetches them per coordinate push and
    // cannot keep them: two stack entries are live while arbitrary operations run)
    T px[kNE][3], py[kNE][3];
    if constexpr (SEP) {
#pragma unroll
      for (int j = 0; j < kNE; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          px[j][i] = vert_at[j][i][0];
          py[j][i] = vert_at[j][i][1];
        }
      src_separable<T, kNE>(sep_flags, __builtin_offsetof(RingArgs<T>, src) + __builtin_offsetof(SrcProgram<T>, c),
                            __builtin_offsetof(RingArgs<T>, lam), px, py, fv);
    } else {
      src_run_wide<T, (QL > 0 ? QL : 1), kNE>(prog, vert_at, a.lam, __builtin_offsetof(RingArgs<T>, lam), fv);
    }
    // the constants of the shares; fp64: scalar loads in flight during the determinants' LDS reads
    // (src_kernarg_table: not carried through the interpreter in spill lanes)
    constexpr int kQ = QL > 0 ? QL : 1;
    T qs[3], hwq[kQ], lamq[3][kQ];
    if constexpr (QL == 4) {
      if constexpr (kSrcTableLoads<T>) {  // (SEP: the host has put the functions' factors on these three)
        const src_const_tab<T> t = src_kernarg_table<T>(__builtin_offsetof(RingArgs<T>, qsym));
#pragma unroll
        for (int i = 0; i < 3; ++i) qs[i] = t[3 + i];
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) qs[i] = a.qsym[3 + i];
      }
    } else if constexpr (kSrcTableLoads<T>) {
      const src_const_tab<T> tl = src_kernarg_table<T>(__builtin_offsetof(RingArgs<T>, lam));
      const src_const_tab<T> th = tl + 3 * kMaxQuad;  // RingArgs::hw follows lam: one opaque pointer
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        hwq[q] = th[q];
#pragma unroll
        for (int i = 0; i < 3; ++i) lamq[i][q] = tl[i * kMaxQuad + q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        hwq[q] = a.hw[q];
#pragma unroll
        for (int i = 0; i < 3; ++i) lamq[i][q] = a.lam[i][q];
      }
    }
    // The pass's LDS reads first, for all its elements (a lane without an element j holds the zero-filled
    // code 0: vertex 0 of the tile, a valid address), then the arithmetic across the elements; only the adds
    // sit behind the lanes' predicate.  With everything of element j behind `l < n_tv` a pass paid one LDS
    // round trip per element, in series; the operations and their order per element are unchanged.
    if constexpr (!SEP) {
#pragma unroll
      for (int j = 0; j < kNE; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          px[j][i] = vert_at[j][i][0];
          py[j][i] = vert_at[j][i][1];
        }
    }
    T share[kNE][3];  // share[j][i]: to local vertex i of element j
#pragma unroll
    for (int j = 0; j < kNE; ++j) {
      const T det = (px[j][1] - px[j][0]) * (py[j][2] - py[j][0]) - (px[j][2] - px[j][0]) * (py[j][1] - py[j][0]);
      if constexpr (QL == 4) {
        // the order-3 rule's structure (RingArgs::qsym): 7 operations instead of 16
        const T *f4 = fv + j * 4;
        const T base = src_fma<T>(qs[0], f4[0], qs[1] * ((f4[1] + f4[2]) + f4[3]));
        share[j][0] = det * src_fma<T>(qs[2], f4[3], base);
        share[j][1] = det * src_fma<T>(qs[2], f4[1], base);
        share[j][2] = det * src_fma<T>(qs[2], f4[2], base);
      } else {
        T fw[QL > 0 ? QL : 1];
#pragma unroll
        for (int q = 0; q < QL; ++q) fw[q] = fv[j * (QL > 0 ? QL : 1) + q] * hwq[q];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          T g = T(0);
#pragma unroll
          for (int q = 0; q < QL; ++q) g = g + fw[q] * lamq[i][q];
          share[j][i] = det * g;
        }
      }
    }
    // (the empty asm keeps reads and arithmetic where they are written: left alone, hipcc sinks each
    // element's back behind its predicate)
#pragma unroll
    for (int j = 0; j < kNE; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(share[j][i]));
#pragma unroll
    for (int j = 0; j < kNE; ++j) {
      if (vtid + j * kRingBlock < d.n_tv) {
#pragma unroll
        for (int i = 0; i < 3; ++i) add_share((codes[j] >> (10 * i)) & 0x3FFu, acc, share[j][i]);
      }
    }
  };
  // SRC: det_T g[T][i], g[T][i] = sum_q f(x_q) l_i(q) w_q / 2, of the elements the tile evaluates
  // from the tile's coordinates in LDS (basis.py:90-91: x_q = bar(q)^T X), added to the
  // accumulators of the elements' vertices in LDS (element form: no slot codes, nothing per fan
  // slot).  Lane `tid` takes the elements tid, tid + 256, tid + 512 of the tile's table; a wave
  // runs the interpreter on as many of them as ITS lanes have (wave-uniform): of a tile's ~520
  // elements the third round holds 8, which only wave 0 sees.
  auto compute_g = [&](const RingDesc &d, const unsigned (&tv)[SRC ? kRingElemPerLane : 1], const T *xyc,
                       T *acc, int rot) {
    const int vwave = (wave + rot) & (kRingWaves - 1);
    const int vtid = (vwave << 6) + lane;
    // rounds of this wave: elements vwave * 64 + 256 j + lane < n_tv
    const int rounds = (d.n_tv - vwave * 64 + kRingBlock - 1) / kRingBlock;
    if (rounds <= 0) return;  // wave-uniform
    if constexpr (SRC == 2) {
      if (rounds >= 3)
        compute_g_wide(std::integral_constant<int, 3>{}, d, tv, xyc, acc, vtid);
      else
        compute_g_wide(std::integral_constant<int, 2>{}, d, tv, xyc, acc, vtid);
    } else if constexpr (SRC == 1) {
      // the loop is not unrolled (one copy of the interpreter): every pass takes entry 0 and
      // rotates the array -- a register array indexed by the loop counter would go to scratch
      unsigned codes[kRingElemPerLane];
#pragma unroll
      for (int j = 0; j < kRingElemPerLane; ++j) codes[j] = tv[SRC ? j : 0];
#pragma unroll 1
      for (int j = 0; j < kRingElemPerLane; ++j) {
        if (j >= rounds) break;  // wave-uniform
        const int l = vtid + j * kRingBlock;
        const unsigned code = codes[0];
#pragma unroll
        for (int r = 0; r + 1 < kRingElemPerLane; ++r) codes[r] = codes[r + 1];
        T x0, y0, x1, y1, x2, y2;
        lds_xy(xyc, code & 0x3FFu, x0, y0);
        lds_xy(xyc, (code >> 10) & 0x3FFu, x1, y1);
        lds_xy(xyc, (code >> 20) & 0x3FFu, x2, y2);
        T xq[QL > 0 ? QL : 1], yq[QL > 0 ? QL : 1], fv[QL > 0 ? QL : 1];
        // (the tables stay the by-value argument's here: read by scalar loads like the wide pass reads
        // them, 100 -> 34 spilled scalars, but hipcc then leaves fourteen of these instantiations a
        // private segment of 36 bytes that no instruction touches -- profiles/fused_hot_loop.log)
#pragma unroll
        for (int q = 0; q < QL; ++q) {
          xq[q] = (a.lam[0][q] * x0 + a.lam[1][q] * x1) + a.lam[2][q] * x2;
          yq[q] = (a.lam[0][q] * y0 + a.lam[1][q] * y1) + a.lam[2][q] * y2;
        }
        src_run<T, (QL > 0 ? QL : 1)>(prog, xq, yq, fv);
        if (l < d.n_tv) {
          // signed determinant in the element's own vertex order (element_tri.py:139)
          const T det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
          T fw[QL > 0 ? QL : 1];
#pragma unroll
          for (int q = 0; q < QL; ++q) fw[q] = fv[q] * a.hw[q];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            T g = T(0);
#pragma unroll
            for (int q = 0; q < QL; ++q) g = g + fw[q] * a.lam[i][q];
            add_share((code >> (10 * i)) & 0x3FFu, acc, det * g);
          }
        }
      }
    }
  };

  auto load_tile = [&](const RingDesc &d, unsigned g_own, unsigned g_halo) {
    if constexpr (kTileDesc) {  // SEP: no slot codes, the coordinates go to LDS by themselves (load_xy_lds)
      static_assert(!kTileDesc || (!FQ && kCoordsToLds), "the per-tile descriptors cover the SEP launches' loads");
      const int first = d.row_off + d.row0, n = d.row1 - d.row0;  // the wave's rows
      ring_load_rec<SLOTS>(tile_rsrc(a.off_rows, first, n, kRecBytes), lane_b16 * (kRecBytes / 16u), rec_ld);
      if (!CHUNK)
        rowstart_ld = int(__builtin_amdgcn_raw_buffer_load_b32(tile_rsrc(a.off_rowstart, first, n, 4u), lane_b4, 0, 0));
      hin_ld = __builtin_amdgcn_raw_buffer_load_b16(tile_rsrc(a.off_hin, first, n, 2u), lane_b2, 0, 0);
      return;
    }
    const int r = d.row0 + lane;
    const unsigned row = r < d.row1 ? unsigned(d.row_off + r) : kNone;
    ring_load_rec<SLOTS>(r_plan, a.off_rows + row * kRecBytes, rec_ld);
    if (!CHUNK)
      rowstart_ld = int(__builtin_amdgcn_raw_buffer_load_b32(r_plan, a.off_rowstart + row * 4u, 0, 0));
    if (FQ) {  // 12-bit slot codes: 3 (SLOTS 7) or 6 dwords per row
      const unsigned eb = a.off_elems + row * unsigned(4 * kEW);
#pragma unroll
      for (int i = 0; i < kEW; i += 3) {
        const ru32x3 v = __builtin_amdgcn_raw_buffer_load_b96(r_plan, eb + unsigned(4 * i), 0, kStreamLoadNT);
        se_ld[FQ ? i : 0] = v.x;
        se_ld[FQ ? i + 1 : 0] = v.y;
        se_ld[FQ ? i + 2 : 0] = v.z;
      }
    }
    if constexpr (!kCoordsToLds) {
      ring_load_xy<T>(r_coords, g_own, own_ld[0], own_ld[1]);
      ring_load_xy<T>(r_coords, g_halo, halo_ld[0], halo_ld[1]);
    }
    if (SRC)  // local id of the row's vertex in the previous tile of the chain block (0xFFFF: none)
      hin_ld = __builtin_amdgcn_raw_buffer_load_b16(r_plan, a.off_hin + row * 2u, 0, 0);
  };
  auto park = [&](const RingDesc &d, T *dst) {
    if constexpr (kCoordsToLds) return;
    const int r = d.row0 + lane;
    if (r < d.row1) {
      dst[2 * r] = own_ld[0];
      dst[2 * r + 1] = own_ld[1];
    }
    const int h = d.n_own + tid;
    if (h < d.n_vert) {
      dst[2 * h] = halo_ld[0];
      dst[2 * h + 1] = halo_ld[1];
    }
  };
  // kCoordsToLds: the coordinates of a tile straight from memory into `dst`, 16 bytes per lane and no
  // register in between (buffer_load_dwordx4 ... lds: lane l of the wave lands 16 l bytes behind the
  // wave-uniform LDS base in m0).  The own rows land at dst[2 (row0 + l)], halo vertex n_own + tid at
  // dst[2 (n_own + 64 wave + l)]: where `park` puts them.  The bounds tests stay branches -- a lane
  // outside them is inactive and writes nothing.  The loads count in vmcnt like any other.
  auto load_xy_lds = [&](const RingDesc &d, unsigned g_own, unsigned g_halo, T *dst) {
    if constexpr (kCoordsToLds) {
      typedef __attribute__((address_space(3))) void *lds_ptr;
      if constexpr (kTileDesc && CHUNK) {
        // consecutive vertices: the lane's offset is 16 (gid0 + lane), one shift-add on the lane number, and
        // the lane test is against the wave's row count (a lane behind the rows must write nothing: the
        // next wave's rows or the halo land there)
        if (lane < d.row1 - d.row0)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(r_coords, (lds_ptr)(dst + 2 * d.row0), 16,
                                                   (unsigned(lane) << 4) + unsigned(d.gid0) * 16u, 0, 0, 0);
      } else if (d.row0 + lane < d.row1)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_coords, (lds_ptr)(dst + 2 * d.row0), 16, g_own * 16u, 0, 0, 0);
      if (d.n_own + tid < d.n_vert)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_coords, (lds_ptr)(dst + 2 * (d.n_own + 64 * wave)), 16,
                                                 g_halo * 16u, 0, 0, 0);
    }
  };

  int t_c = tile_at(0);
  if (t_c < 0) return;  // whole workgroup, before any barrier
  int t_n = tile_at(1), t_nn = tile_at(2);
  RingDesc dc = ring_desc<CHUNK>(a.plan, a.off_desc, t_c, wave);
  RingDesc dn = ring_desc<CHUNK>(a.plan, a.off_desc, t_n >= 0 ? t_n : t_c, wave);
  RingDesc dnn = ring_desc<CHUNK>(a.plan, a.off_desc, t_nn >= 0 ? t_nn : t_c, wave);
  // prologue: tile 0 taken over, vertex ids of tile 1 in registers
  load_ids(dc, gid_own, gid_halo);
  load_eids(dc, eid);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  load_tile(dc, gid_own, gid_halo);
  load_xy_lds(dc, gid_own, gid_halo, xy);
  load_fq(dc, eid);
  load_tverts(dc, tev_ld, 0);
  if (t_n >= 0) {
    load_ids(dn, gid_own_ld, gid_halo_ld);
    load_eids(dn, eid_ld);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);
  park(dc, xy);
  park_g(dc, gtab);
  rec = rec_ld;
  hin = hin_ld;
  rowstart = rowstart_ld;
  gid_row = gid_own;
#pragma unroll
  for (int i = 0; i < (FQ ? kEW : 1); ++i) se[i] = se_ld[i];
#pragma unroll
  for (int j = 0; j < (FQ ? kRingElemPerLane : 1); ++j) eid[j] = eid_ld[j];
#pragma unroll
  for (int j = 0; j < (SRC ? kRingElemPerLane : 1); ++j) tev[j] = tev_ld[j];
  gid_own = gid_own_ld;
  gid_halo = gid_halo_ld;
  __syncthreads();

  int cur = 0;
  int a_cur = 0, a_prev = 2, a_next = 1;  // accumulator buffers of this tile, the one before, the one after
  for (int k = 0;; ++k) {
    if (SRC) {
      // The vector pipe serves a SIMD's OLDEST wave first: of four equally loaded workgroups on a CU
      // the first one placed finished its loop after 100 us, the last after 190
      // (profiles/r03_wave_loop_spread.log).  The workgroups take turns in issue priority, tile by tile.
      switch ((k + int(blockIdx.x >> kRingPrioShift)) & 3) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
      }
    }
    // phase A stays a lambda: written out in place, it leaves hipcc with another instruction schedule
    auto phase_a = [&]() {
      if (t_n >= 0) {
        load_tile(dn, gid_own, gid_halo);
        load_fq(dn, eid);
        load_tverts(dn, tev_ld, k + 1);
        if (t_nn >= 0) {
          load_ids(dnn, gid_own_ld, gid_halo_ld);
          load_eids(dnn, eid_ld);
        }
      }
    };
    if (SRC) {
      // kCoordsToLds: the coordinates of tile k+1 (its vertex ids arrived in iteration k-1) set off
      // towards the other buffer, whose last readers ended at barrier E of iteration k-1.  They hold
      // no register and are in flight during the whole of G; C's vmcnt(0) and barrier E publish them.
      if (t_n >= 0) load_xy_lds(dn, gid_own, gid_halo, xy + (cur ^ 1) * 2 * a.lds_vert);
      // ---- G ---- source values of tile k (its coordinates are complete).  Before A: the
      // registers of tile k+1's loads are not live while the program runs (3 workgroups per CU)
      compute_g(dc, tev, xy + cur * 2 * a.lds_vert, accs + a_cur * acc_stride, k);
      if constexpr (SEP) {
        // The buffer descriptors are read again from the kernel-argument segment instead of being carried
        // through G: the straight-line pass needs the scalar registers, and what it pushed out came back
        // either from spill lanes (a v_readlane each) or by hipcc re-loading the by-value argument, which
        // left the kernel a private segment of 36 bytes that no instruction touches.  The opaque pointer
        // keeps the loads here (src_kernarg_table); nothing in front of G but the coordinate loads, which
        // take last iteration's r_coords, uses a descriptor.
        typedef const RingArgs<T> __attribute__((address_space(4))) *ring_kernargs;
        const ring_kernargs ka = (ring_kernargs)src_kernarg_table<char>(0);
        r_coords = ring_rsrc(ka->coords, ka->coords_bytes);
        plan_at = ka->plan;  // the tiles' own plan descriptors (tile_rsrc) are formed from these two, behind
        plan_room = ka->plan_bytes;  // this point
        vals_at = ka->vals;
        vals_room = ka->vals_bytes;
        plain_now = ka->plain_stores;
        r_vals = ring_rsrc(vals_at, vals_room);
        r_fout = ring_rsrc(ka->fout, ka->fout_bytes);
      }
      // (the barrier behind G stands in front of the rows' read of their sums -- SEP: behind D --: the
      // next tile's loads and the rows' own arithmetic need nothing of G)
    }
    // ---- A ----
    phase_a();
    // ---- B ----
    T off[SLOTS + 1], diag, sdets[SLOTS];
    // wave-uniform: shorter slot loops when no row of this wave needs the long ones
    // (7-slot records, launches bound by vector issue: the interior vertices of a structured mesh
    // have six neighbours, the seventh slot of such a wave is empty)
    constexpr int kBandSlots = (SLOTS > kRingBand && kRingBand > 0) ? kRingBand : (SLOTS == 7 && SRC ? 6 : SLOTS);
    const bool banded = kBandSlots < SLOTS && __builtin_amdgcn_ballot_w64(rec.k() > kBandSlots) == 0;
    bool regular = false;
    const int my_row = dc.row0 + lane;
    const uint32_t lv = unsigned(my_row < dc.row1 ? my_row : 0);
    if constexpr (SLOTS == 7 && SRC) {
      // wave-uniform: every row of the wave (lanes without a row aside) is a regular one
      const bool mine = ((rec.w[2] >> 10) & 0x3FFFu) == 0x555u && rec.k() == 6;
      regular = __builtin_amdgcn_ballot_w64(!(mine || my_row >= dc.row1)) == 0;
    }
    if (regular) {
      if constexpr (SLOTS == 7) ring_row_regular<T, MASS>(a, rec, lv, xy + cur * 2 * a.lds_vert, off, diag);
    } else if (banded)
      ring_row<T, SLOTS, MASS, FQ, kBandSlots>(a, rec, lv, xy + cur * 2 * a.lds_vert, off, diag, sdets);
    else
      ring_row<T, SLOTS, MASS, FQ>(a, rec, lv, xy + cur * 2 * a.lds_vert, off, diag, sdets);
    int total = 0, pre = 0;
    if (KMAT) {
      if (regular) {
        if constexpr (SLOTS == 7) total = ring_stage_regular<T>(rec, off, diag, my_stage, pre, dc.row1 - dc.row0);
      } else {
        total = banded ? ring_stage<T, SLOTS, kBandSlots>(rec, off, diag, my_stage, pre)
                       : ring_stage<T, SLOTS>(rec, off, diag, my_stage, pre);
      }
    }
    T facc = T(0);
    if (SRC && !SEP) {  // the row's sum is complete behind the barrier: one LDS read
      ring_lds_barrier();
      const unsigned from = (hin & 0xFFFFu) == 0xFFFFu ? unsigned(a.lds_vert) : (hin & 0xFFFFu);  // lds_vert: the zero
      facc = accs[a_cur * acc_stride + (my_row < dc.row1 ? my_row : a.lds_vert)] + accs[a_prev * acc_stride + from];
    }
    if (FQ) {
      const T *g = gtab;
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        // code: tile-local element | loc << 10; 0xFFF (no triangle) reads the spare entries
        // behind the table, its determinant is 0
        const int bit = 12 * i, w0 = bit / 32, sh = bit % 32;  // constants once the loop is unrolled
        const uint32_t lo = se[w0] >> sh;
        const uint32_t code = (sh > 20 ? lo | (se[w0 + 1 < kEW ? w0 + 1 : w0] << (32 - sh)) : lo) & 0xFFFu;
        const uint32_t at = code == 0xFFFu ? unsigned(3 * a.lds_elem) : 3u * (code & 0x3FFu) + (code >> 10);
        facc = facc + sdets[i] * g[at];
      }
    }
    const int kk = rec.k();
    const int len_c = kk > 0 ? kk + 1 : 0;
    // ---- C ----
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); the builtin, so that hipcc's own wait
                                         // insertion knows the loads have landed
    // ---- D ----
    if (SRC) {
      // the buffer the NEXT tile fills: the tile two back filled it, the rows of the tile before this
      // one were its last readers (previous iteration, in front of its closing barrier)
      if constexpr (kTileDesc) {
        // two sums per lane and store (ds_write_b128): one store per lane for up to 510 vertex slots.
        // acc_stride = lds_vert + 2 is even and the buffers start on 16 bytes (xy: 32 lds_vert bytes, the
        // stage: 4 (64 (SLOTS + 1) + 2) entries), so the last pair ends where the buffer does
        typedef T acc_pair __attribute__((ext_vector_type(2)));
        acc_pair *clean = reinterpret_cast<acc_pair *>(accs + a_next * acc_stride);
        for (int i = tid; 2 * i < acc_stride; i += kRingBlock) clean[i] = acc_pair{T(0), T(0)};
      } else {
        for (int i = tid; i < acc_stride; i += kRingBlock) accs[a_next * acc_stride + i] = T(0);
      }
    }
    if (t_n >= 0) {
      park(dn, xy + (cur ^ 1) * 2 * a.lds_vert);
      if (FQ) {
        // the element table is single-buffered (LDS for a third workgroup per CU): every wave
        // has read tile k's entries (the loop above) before anybody overwrites them
        ring_lds_barrier();
        park_g(dn, gtab);
      }
    }
    if (KMAT) {
      if constexpr (kTileDesc && CHUNK && SLOTS == 7) {
        // the same through a descriptor of the run's own (ring_store_run1_desc); a regular wave has no long
        // row and does not look for one.  (7-slot records: with the eight steps of a 15-slot stage read ahead of
        // the stores the K + f kernels need 187 registers and lose their third wave; they keep the code below.)
        __builtin_amdgcn_wave_barrier();
        bool holes = false;
        if (!regular) {
          const int k_row = rec.k();
          const bool is_long = dc.row0 + lane < dc.row1 && k_row == 0 && (rec.w[3] >> 31) != 0u;
          holes = __ballot(is_long) != 0ull;
          if (holes) {
            const int true_len = is_long ? int(rec.w[3] & 0x7FFFFFFFu) : k_row > 0 ? k_row + 1 : 0;
            const int csr = dc.rs0 + wave_inclusive_scan(true_len) - true_len;
            ring_store_pieces<T>(my_stage, total, pre, csr, is_long, r_vals);
          }
        }
        if (!holes)
          ring_store_run1_desc<T>(
              my_stage, total, run_rsrc(vals_at, vals_room, dc.rs0, total & ~1), lane_b16,
              [&]() { return run_rsrc(vals_at, vals_room, dc.rs0 + total - 1, 1); }, plain_now);
        __builtin_amdgcn_wave_barrier();
      } else if (CHUNK) {  // one run per wave by construction, its CSR offset in the descriptor
        __builtin_amdgcn_wave_barrier();
        // long rows (k = 0, bit 31 of the last record word, the row's length below it) leave holes
        const bool is_long = SLOTS == 7 && dc.row0 + lane < dc.row1 && kk == 0 && (rec.w[3] >> 31) != 0u;
        if (SLOTS != 7 || __ballot(is_long) == 0ull) {
          ring_store_run1<T, SLOTS>(my_stage, total, dc.rs0, r_vals, a.plain_stores);
        } else {
          const int true_len = is_long ? int(rec.w[3] & 0x7FFFFFFFu) : len_c;
          const int csr = dc.rs0 + wave_inclusive_scan(true_len) - true_len;
          ring_store_pieces<T>(my_stage, total, pre, csr, is_long, r_vals);
        }
        __builtin_amdgcn_wave_barrier();
      } else {
        ring_store<T, SLOTS>(my_stage, total, pre, rowstart, len_c, r_vals, a.plain_stores);
      }
    }
    if (SEP) {
      // SEP: the barrier behind G stands HERE, behind C and D.  The waves of a tile run two or three rounds
      // of G, and those with two waited at it for the one with three before they did anything of C and D --
      // none of which needs G's sums.  Hazards of what moved in front of it: the zeroing writes the buffer
      // a_next, whose last readers were the rows of the previous tile, in front of ITS barrier E; xy[cur ^ 1]
      // is written by the coordinate loads issued at the top of the iteration either way (`park` copies
      // nothing in these launches), last read by phases G and B of the previous iteration, in front of that
      // same barrier, while the waves still in G read xy[cur]; the stage is wave-private.  C's vmcnt(0)
      // stays ahead of the K stores, so it waits for loads issued a row phase ago and for the stores of the
      // previous tile only.  (Moved in every SRC instantiation it gave the other programs nothing and cost
      // the general interpreter's depth-3 program 1 %, profiles/fused_separable.log: they keep the barrier
      // in front of C.)
      ring_lds_barrier();
      const unsigned from = (hin & 0xFFFFu) == 0xFFFFu ? unsigned(a.lds_vert) : (hin & 0xFFFFu);
      facc = accs[a_cur * acc_stride + (my_row < dc.row1 ? my_row : a.lds_vert)] + accs[a_prev * acc_stride + from];
    }
    if (LOAD && dc.row0 + lane < dc.row1) {
      // kTileDesc, consecutive vertices: the row's vertex is gid0 + lane (load_ids)
      const unsigned byte = (kTileDesc && CHUNK) ? (unsigned(lane) << 3) + unsigned(dc.gid0) * 8u
                                                 : gid_row * unsigned(sizeof(T));
      if constexpr (sizeof(T) == 8)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ru32x2, facc), r_fout, byte, 0, kStreamNT);
      else
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, facc), r_fout, byte, 0, kStreamNT);
    }
    if (t_n < 0) break;
    rec = rec_ld;
    hin = hin_ld;
    rowstart = rowstart_ld;
    gid_row = gid_own;
#pragma unroll
    for (int i = 0; i < (FQ ? kEW : 1); ++i) se[i] = se_ld[i];
#pragma unroll
    for (int j = 0; j < (FQ ? kRingElemPerLane : 1); ++j) eid[j] = eid_ld[j];
#pragma unroll
    for (int j = 0; j < (SRC ? kRingElemPerLane : 1); ++j) tev[j] = tev_ld[j];
    gid_own = gid_own_ld;
    gid_halo = gid_halo_ld;
    {  // accumulator buffers: tile k + 1 fills what was the clean one
      const int t = a_prev;
      a_prev = a_cur;
      a_cur = a_next;
      a_next = t;
    }
    // ---- E ----
    ring_lds_barrier();
    t_c = t_n;
    dc = dn;
    t_n = t_nn;
    dn = dnn;
    t_nn = tile_at(k + 3);
    if (t_nn >= 0) dnn = ring_desc<CHUNK>(plan_now(), a.off_desc, t_nn, wave);
    cur ^= 1;
  }
}

// SRC instantiations (tfem_rings_src.hip): nq > 0; kmat = false: the load vector alone.
// wide: the three-elements-per-pass interpreter (programs of depth <= 2)
// separable: the straight-line instantiations (ring_src_route's 2; fp64, nq = 4, wide)
template <typename T>
void *pick_ring_src_kernel(int slots, bool mass, bool chunk, int nq, bool kmat, bool wide, bool separable);
// Which interpreter pick_ring_src_kernel's launch runs (`wide`: the program's depth allows the wide
// one): with Q = 6 the wide interpreter would hold 2 x 18 doubles, so it keeps the one-element form.
// The proven sin / cos operations (src_convert_proven) are known to the wide interpreter only.
inline bool ring_src_runs_wide(int nq, bool wide) { return wide && nq <= 4; }

// What every launch over a ring plan (layout z[], tfem_rings_host.cpp) sets alike: the capacity
// check, the coordinate and plan extents, the section offsets, the tile count (the whole plan),
// the LDS vertex slots and W / M_dd / M_od.  Every other field is zero.
template <typename T>
static int ring_args_init(const TriTables &tables, const int64_t *z, const void *coords, const unsigned char *plan,
                   int64_t n_verts, double alpha, double beta, RingArgs<T> &a) {
  if (z[0] < 0 || z[4] > kRingBlock || z[3] > kRingVertCap || z[4] > z[3] || z[14] > kRingHaloCap ||
      !((z[6] == 7 && z[7] == 4) || (z[6] == 15 && z[7] == 8)) || (z[5] > z[6] + 1 && z[23] == 0) || z[5] > 16)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "ring plan exceeds the kernel's capacities");
  const int64_t extents[2] = {n_verts * 2 * int64_t(sizeof(T)), z[12]};
  const int st = check_extents("ring kernel", extents, 2);
  if (st != TFEM_OK) return st;
  std::memset(&a, 0, sizeof(a));
  a.coords = static_cast<const T *>(coords);
  a.plan = plan;
  a.coords_bytes = unsigned(extents[0]);
  a.plan_bytes = unsigned(extents[1]);
  a.off_desc = unsigned(z[8]);
  a.off_rows = unsigned(z[9]);
  a.off_rowstart = unsigned(z[10]);
  a.off_gid = unsigned(z[11]);
  a.n_tiles = int(z[0]);
  a.lds_vert = (int(z[3]) + 1) & ~1;
  // W = sum_q w_q/2 and M_ij = sum_q (w_q/2) l_i l_j, formed in T in quadrature order.  The
  // rules of element_tri.py:77-130 are symmetric, so M has one diagonal and one off-diagonal
  // value (up to rounding: entries 00 and 01 are used).
  T w = T(0), md = T(0), mo = T(0);
  for (int q = 0; q < tables.nq; ++q) {
    w = w + T(tables.hw[q]);
    md = md + T(tables.hw[q]) * (T(tables.lam[q][0]) * T(tables.lam[q][0]));
    mo = mo + T(tables.hw[q]) * (T(tables.lam[q][0]) * T(tables.lam[q][1]));
  }
  a.stiff_w = T(alpha) * w;
  a.mass_d = T(beta) * md;
  a.mass_o = T(beta) * mo;
  return TFEM_OK;
}

}  // namespace tfem
