// P1 alpha * stiffness + beta * mass over a ring plan (tfem_rings_host.cpp): owner-computes
// ROW form of the element loop.  One lane owns one CSR row (= vertex v).  Its record lists
// the neighbours n_0 .. n_{k-1} of v in fan order as tile-local ids; the triangle of slot i is
// (v, n_i, n_next) with next = i + 1 (or 0 behind slot k - 1), flagged with the orientation it
// has in the connectivity.  With e_i = x(n_i) - x(v), d = e_next - e_i and the signed
// determinant det = +-(e_i x e_next) (element_tri.py:139) the P1 entries of row v are
// (basis.py:87-88, element_tri.py:41,132-145, abstract_basis.py:83; gradients are constant on
// the element, so sum_q w_q/2 = W is folded in)
//     K[v][v]      += (W / det) d.d
//     K[v][n_i]    -= (W / det) d.e_next
//     K[v][n_next] += (W / det) d.e_i
// and the mass part adds det * M_ii resp. det * M_ij (M = sum_q (w_q/2) l_i l_j).  Every
// triangle is evaluated by its three rows (three times the arithmetic of the element form)
// in exchange for: no atomics, no accumulators shared between lanes, one barrier per tile.
// The row's entries stay in registers; they are permuted into CSR order through a per-wave
// LDS stage (plain stores) and leave as lane-contiguous global stores.
//
// HBM traffic per element with consecutive-vertex tiles (N_v = N_T / 2; measured):
// row records 8 B + halo vertex ids ~1 B + coordinates ~9.5 B (halo re-reads included) +
// values 28.6 B = 47.6 B, against 48 B algorithmic: the 16-byte row records replace the
// 24 bytes of connectivity the row's triangles take.
#include <cmath>

#include "tfem_rings_kernel.hpp"

namespace tfem {

// Rows of vertices with 8 .. 15 neighbours in a plan with long rows: sixteen lanes per row
// (ring_long_slot); each slot lane writes its entry, lane 0 the diagonal.
template <typename T, bool MASS>
__global__ __launch_bounds__(kRingBlock) void k_p1_long_rows(const T *coords, const unsigned char *plan,
                                                             unsigned off_long, int n_long, T *vals, T stiff_w,
                                                             T mass_d, T mass_o) {
  RingLongSlot<T> s;
  ring_long_slot<T, MASS, false>(coords, plan, off_long, n_long, stiff_w, mass_o, nullptr, s);
  if (!s.slot) return;
  T *out = vals + s.rec[1];
  out[int((s.rec[19 + s.i / 8] >> (4 * (s.i % 8))) & 15u)] = s.entry;
  if (s.i == 0) out[s.dpos] = ring_diag<T, MASS>(s.sum, s.dsum, mass_d, mass_o);
}

struct RingLaunch {
  const void *coords;
  int quad_order;
  double alpha, beta;
  const unsigned char *plan;
  const int64_t *layout;
  int64_t n_verts, nnz;
  void *vals;
  hipStream_t stream;
  const void *fq = nullptr;  // nullptr: no load vector
  int64_t n_elems = 0;
  void *fout = nullptr;
  const tfem_source_program *source = nullptr;  // load vector of this program instead of fq
  int64_t tile_first = 0, tile_count = -1;       // tile range of the plan (-1: to the end)
  int blocks_per_cu = 0;  // > 0: cap on resident workgroups per CU (tuning)
};

// load vector alone (vals == NULL): the matrix part of the row is dead code
template <typename T, int SLOTS, bool CHUNK>
static void *pick_ring_load_only(int nq) {
  switch (nq) {
    case 1: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, false, CHUNK, 1, false, false>);
    case 3: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, false, CHUNK, 3, false, false>);
    case 4: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, false, CHUNK, 4, false, false>);
    case 6: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, false, CHUNK, 6, false, false>);
    default: return nullptr;
  }
}

template <typename T, int SLOTS, bool MASS, bool CHUNK>
static void *pick_ring_q(int nq) {
  switch (nq) {
    case 0: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, MASS, CHUNK, 0, false>);
    case 1: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, MASS, CHUNK, 1, false>);
    case 3: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, MASS, CHUNK, 3, false>);
    case 4: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, MASS, CHUNK, 4, false>);
    case 6: return reinterpret_cast<void *>(k_p1_rings<T, SLOTS, MASS, CHUNK, 6, false>);
    default: return nullptr;
  }
}

template <typename T, int SLOTS, bool CHUNK>
static void *pick_ring_mass(bool kmat, bool mass, int nq) {
  if (!kmat) return pick_ring_load_only<T, SLOTS, CHUNK>(nq);
  return mass ? pick_ring_q<T, SLOTS, true, CHUNK>(nq) : pick_ring_q<T, SLOTS, false, CHUNK>(nq);
}

// nq = 0: matrix only; kmat = false: the load vector alone; src: source program in the launch
// (those instantiations live in tfem_rings_src.hip)
template <typename T>
static void *pick_ring_kernel(int slots, bool mass, bool chunk, int nq, bool src, bool kmat, bool wide,
                              bool separable) {
  if (src) return pick_ring_src_kernel<T>(slots, mass, chunk, nq, kmat, wide, separable);
  if (slots == 7)
    return chunk ? pick_ring_mass<T, 7, true>(kmat, mass, nq) : pick_ring_mass<T, 7, false>(kmat, mass, nq);
  return chunk ? pick_ring_mass<T, 15, true>(kmat, mass, nq) : pick_ring_mass<T, 15, false>(kmat, mass, nq);
}

// programs that never hold more than two values: three elements per pass of the interpreter
static bool ring_src_wide(const tfem_source_program *source) {
  bool wide = src_depth(source) <= 2;
  if (const char *v = std::getenv("TFEM_SRC_WIDE")) wide = wide && std::atoi(v) != 0;  // developer switch
  return wide;
}

// The program as the launch hands it to the kernel.  With the caller's bound on THIS coordinate array
// (tfem_ring_plan_vouch_coords: layout[29] the array it vouched for, layout[31] the bound) the fp64
// launches of the wide interpreter -- the one that knows the proven operations -- skip the range tests
// of the SIN / COS the host proves; everything else is converted as it is.
// (-1: the caller vouched for nothing, or for another array)
static double ring_coord_bound(const int64_t *z, const void *coords) {
  double coord_bound = -1.0;
  if (z[29] != 0 && uintptr_t(z[29]) == reinterpret_cast<uintptr_t>(coords))
    std::memcpy(&coord_bound, &z[31], sizeof(coord_bound));
  return coord_bound;
}

template <typename T>
static int ring_src_convert(const int64_t *z, const void *coords, int nq, const tfem_source_program *source,
                            SrcProgram<T> *out) {
  const double coord_bound = ring_coord_bound(z, coords);
  if (sizeof(T) == 8 && coord_bound >= 0.0 && ring_src_runs_wide(nq, ring_src_wide(source)))
    return src_convert_proven<T>(source, coord_bound, out);
  return src_convert<T>(source, out);
}

// What evaluates the program in the launch: 0 the general interpreter, 1 the wide one, 2 straight-line
// code for a separable program (src_is_separable: fp64, four points, every sine / cosine proven for
// THIS coordinate array).  TFEM_RINGS_SEPARABLE=0 keeps such a program on the interpreter.
template <typename T>
static int ring_src_route(const int64_t *z, const void *coords, int nq, const tfem_source_program *source) {
  if (!ring_src_runs_wide(nq, ring_src_wide(source))) return 0;
  bool separable = sizeof(T) == 8 && nq == 4;
  if (const char *v = std::getenv("TFEM_RINGS_SEPARABLE")) separable = separable && std::atoi(v) != 0;
  if (!separable) return 1;
  const double coord_bound = ring_coord_bound(z, coords);
  return coord_bound >= 0.0 && src_is_separable(source, coord_bound) ? 2 : 1;
}

// The structure of the 4-point rule the QL = 4 instantiations use (RingArgs::qsym); false: the rule in
// `tables` is not the reference's order-3 rule.
// (c0, a, b from the rule's literals; 1 - xi - eta of the reference's table is the same to an ulp)
template <typename T>
static bool ring_rule_structure(const TriTables &tables, T (&qsym)[6]) {
  const double c0 = tables.lam[0][1], aa = tables.lam[1][1], b = tables.lam[1][2], d = aa - b;
  const int at[4] = {0, 1, 2, 0};
  const double tol = sizeof(T) == 8 ? 1e-15 : 1e-6;  // the tables are rounded to the launch's real type
  auto near = [tol](double x, double y) { return std::fabs(x - y) <= tol; };
  bool ok = tables.hw[1] == tables.hw[2] && tables.hw[1] == tables.hw[3];
  for (int i = 0; i < 3; ++i) {
    ok = ok && near(tables.lam[0][i], c0);
    for (int q = 1; q < 4; ++q) ok = ok && near(tables.lam[q][i], i == at[q] ? aa : b);
  }
  if (!ok) return false;
  qsym[0] = T(c0);
  qsym[1] = T(b);
  qsym[2] = T(d);
  qsym[3] = T(c0) * T(tables.hw[0]);
  qsym[4] = T(b) * T(tables.hw[1]);
  qsym[5] = T(d) * T(tables.hw[1]);
  return true;
}

// The share constants of a launch on route 2: qsym[3..5] with k = c1 c3, the product of the factors behind
// the program's two functions, on them (RingArgs::qsym).  Which coordinate the program pushes first does
// not enter: the product is the same either way.
template <typename T>
static void ring_separable_weights(const tfem_source_program *source, T (&qsym)[6]) {
  const T k = src_separable_factor<T>(source);
  for (int i = 3; i < 6; ++i) qsym[i] = k * qsym[i];
}

template <typename T>
static int ring_src_ops(const int64_t *z, const void *coords, int nq, const tfem_source_program *source,
                        uint8_t *ops_out) {
  SrcProgram<T> device;
  const int st = ring_src_convert<T>(z, coords, nq, source, &device);
  if (st != TFEM_OK) return st;
  std::memset(ops_out, 0, kSrcMaxOps);
  for (int i = 0; i < device.n_ops; ++i) ops_out[i] = uint8_t((device.opw[i >> 2] >> (8 * (i & 3))) & 0xFFu);
  return TFEM_OK;
}

template <typename T>
static int launch_rings(const RingLaunch &L) {
  TriTables tables;
  if (!build_tri_tables(L.quad_order, int(sizeof(T)), &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  const int64_t *z = L.layout;
  if (z[0] == 0) return TFEM_OK;
  const bool src = L.source != nullptr;
  const bool load = L.fq != nullptr || src;
  const bool kmat = L.vals != nullptr;
  if (src && L.fq) return fail(TFEM_ERR_INVALID_ARGUMENT, "source values AND a source program");
  if (!kmat && !load) return fail(TFEM_ERR_INVALID_ARGUMENT, "nothing to assemble");
  if (!L.coords || !L.plan || (load && !L.fout)) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  RingArgs<T> a;
  int st = ring_args_init<T>(tables, z, L.coords, L.plan, L.n_verts, L.alpha, L.beta, a);
  if (st != TFEM_OK) return st;
  const int64_t rb = int64_t(sizeof(T));
  const int64_t extents[3] = {kmat ? L.nnz * rb : 0, (load && !src) ? L.n_elems * tables.nq * rb : 0,
                              load ? L.n_verts * rb : 0};
  st = check_extents("ring kernel", extents, 3);
  if (st != TFEM_OK) return st;
  a.vals = static_cast<T *>(L.vals);
  a.fq = static_cast<const T *>(L.fq);
  a.fout = static_cast<T *>(L.fout);
  a.vals_bytes = unsigned(extents[0]);
  a.fq_bytes = unsigned(extents[1]);
  a.fout_bytes = unsigned(extents[2]);
  a.off_elems = unsigned(z[15]);
  a.off_telems = unsigned(z[16]);
  // measured at 1e7 elements: the matrix-only launch is 4-6 % faster with one contiguous range
  // per XCD (halo coordinates shared in that XCD's L2), the launches that read the source values
  // 6-7 % faster with the tile list dealt to the XCDs in blocks of 4 (one front of reads across
  // the chip; blocks of 1, 2, 8 within 1.5 %)
  a.xcd_interleave = load ? 4 : 0;
  if (const char *v = std::getenv("TFEM_RINGS_XCD"))  // developer switch: block size, 0 = ranges
    a.xcd_interleave = std::strcmp(v, "interleave") == 0 ? 1 : std::atoi(v);
  if (load && !src && z[23] > 0)
    return fail(TFEM_ERR_UNSUPPORTED, "a ring plan with long rows takes the load vector of a source program, "
                "not of pre-evaluated source values");
  if (load && !src && (z[18] == 0 || z[17] > kRingElemPerLane * kRingBlock))
    return fail(TFEM_ERR_UNSUPPORTED, "a tile of the ring plan has %lld elements: the fused load "
                "vector stages at most %d", (long long)z[17], kRingElemPerLane * kRingBlock);
  if (src && z[27] > kRingElemPerLane * kRingBlock)
    return fail(TFEM_ERR_UNSUPPORTED, "a tile of the ring plan evaluates %lld elements: the launch "
                "takes at most %d", (long long)z[27], kRingElemPerLane * kRingBlock);
  for (int i = 0; i < 3; ++i)
    for (int q = 0; q < tables.nq; ++q) {
      a.lamw[i][q] = T(tables.lam[q][i]) * T(tables.hw[q]);
      a.lam[i][q] = T(tables.lam[q][i]);
      a.hw[q] = T(tables.hw[q]);
    }
  if (src && tables.nq == 4 && !ring_rule_structure<T>(tables, a.qsym))
    return fail(TFEM_ERR_UNSUPPORTED, "the 4-point rule is not the reference's order-3 rule");
  if (src) {
    if (z[20] == 0 || z[21] == 0)
      return fail(TFEM_ERR_UNSUPPORTED, "the ring plan carries no element vertex table (source programs)");
    a.off_tverts = unsigned(z[20]);
    a.off_chain = unsigned(z[24]);
    a.off_hin = unsigned(z[26]);
    a.chain_len = int(z[25]);
    if (a.chain_len < 1 || z[24] == 0 || z[26] == 0)
      return fail(TFEM_ERR_INVALID_ARGUMENT, "the ring plan carries no chain order (layout of an older build?)");
    st = ring_src_convert<T>(z, L.coords, tables.nq, L.source, &a.src);
    if (st != TFEM_OK) return st;
  }
  const int64_t t_first = L.tile_first, t_count = L.tile_count < 0 ? z[0] - L.tile_first : L.tile_count;
  if (t_first < 0 || t_count < 0 || t_first + t_count > z[0])
    return fail(TFEM_ERR_INVALID_ARGUMENT, "tile range [%lld, +%lld) outside the plan's %lld tiles",
                (long long)t_first, (long long)t_count, (long long)z[0]);
  if (kmat && z[23] > 0 && (t_first != 0 || t_count != z[0]))
    return fail(TFEM_ERR_UNSUPPORTED, "a ring plan with long rows is launched over all of its tiles: the rows of "
                "the vertices with 8 .. 15 neighbours are written by one launch over all of them");
  if (t_count == 0) return TFEM_OK;
  a.n_tiles = int(t_count);
  // a tile's index only addresses its descriptor; the launches of a source program walk positions
  // [t_first, t_first + t_count) of the chain order instead (the same tiles for the ranges the
  // plan knows: the tiles owning flagged vertices come first in both orders)
  a.n_runs = 0;
  if (src) {
    a.u_first = int(t_first);
    if (z[28] > 0 && (t_first != 0 || t_count != z[0]))
      return fail(TFEM_ERR_UNSUPPORTED, "tile ranges need a plan built with flagged vertices (its blocks break between the ranges)");
    if (z[28] > 0) {  // runs (plans without flagged vertices): the whole plan in one launch
      a.n_runs = int(z[28]);
      a.off_runs = unsigned(z[30]);
    }
  } else {
    a.off_desc += 80u * unsigned(t_first);
  }
  const bool mass = L.beta != 0.0;
  const int slots = int(z[6]);
  a.lds_elem = load ? int(z[17]) : 0;
  const size_t lds = size_t(4 * a.lds_vert) * sizeof(T) +
                     (kmat ? size_t(kRingWaves) * size_t(64 * (slots + 1) + 2) * sizeof(T) : 0) +
                     (src ? size_t(3 * (a.lds_vert + 2)) * sizeof(T)  // three buffers of sums per local vertex
                          : load ? size_t(3 * a.lds_elem + 4) * sizeof(T) : 0);
  const bool chunk = z[13] != 0;
  // Store policy of the CSR values (TFEM_RINGS_STORES=nt | plain overrides).  Measured at S(2236)
  // and S(3162) (profiles/r03_k_store_policy.log): the matrix-only launch from COLD caches (behind
  // 512 MB of unrelated reads) takes 81 us with plain stores against 99 us with non-temporal ones
  // (74 % against 60 % of the roofline; 68 % against 59 % at 2e7 elements), behind unrelated writes
  // both take 112-113 us; only launches of the SAME mesh in a row, whose read set then survives in
  // the memory-side cache, prefer non-temporal stores (81-93 us against 100).  The launches that
  // also form a load vector are bound by vector issue and run 3-20 % faster with non-temporal
  // stores.  So: plain for the matrix alone, non-temporal with a load vector.
  a.plain_stores = !load;
  if (const char *v = std::getenv("TFEM_RINGS_STORES")) a.plain_stores = std::strcmp(v, "plain") == 0;
  // programs that never hold more than two values: three elements per pass of the interpreter
  const bool wide = src && ring_src_wide(L.source);
  const bool separable = src && ring_src_route<T>(z, L.coords, tables.nq, L.source) == 2;
  if (separable) ring_separable_weights<T>(L.source, a.qsym);  // (route 2: the 4-point rule, qsym is filled)
  void *kernel = pick_ring_kernel<T>(slots, mass, chunk, load ? tables.nq : 0, src, kmat, wide, separable);
  if (!kernel) return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  // resident workgroups: what LDS and registers allow per CU, on every CU
  int per_cu = 0;
  st = resident_per_cu(kernel, kRingBlock, lds, &per_cu);
  if (st != TFEM_OK) return st;
  const int deal = a.xcd_interleave > 0 ? a.xcd_interleave : 1;
  int per = int((t_count + 8 * deal - 1) / (8 * deal)) * deal;
  if (src) {  // blocks of the chain order, dealt to the XCDs round-robin: workgroups per XCD that get one
    const int64_t first_block = t_first / a.chain_len, last_block = (t_first + t_count - 1) / a.chain_len;
    per = int((last_block - first_block + 1 + 7) / 8);
    if (a.n_runs > 0) per = (a.n_runs + 7) / 8;
  }
  if (L.blocks_per_cu > 0 && L.blocks_per_cu < per_cu) per_cu = L.blocks_per_cu;
  // TFEM_RINGS_RESERVE_CUS: CUs per XCD this launch leaves free (a sharded step: the kernels of
  // the interface exchange of the previous step -- pack, RCCL's all-reduce, unpack -- find room
  // beside the persistent workgroups of this one)
  int cus = device_cu_count();
  if (const char *v = std::getenv("TFEM_RINGS_RESERVE_CUS")) cus = std::max(8, cus - 8 * std::max(0, std::atoi(v)));
  const int blocks = std::min(per * 8, (cus * per_cu / 8) * 8);
  const dim3 grid{unsigned(blocks)}, block{unsigned(kRingBlock)};
  void *params[] = {&a};
  hipError_t e = hipLaunchKernel(kernel, grid, block, params, lds, L.stream);
  if (e != hipSuccess) return fail(TFEM_ERR_HIP, "ring kernel launch: %s", hipGetErrorString(e));
  if (kmat && z[23] > 0) {  // the rows of the vertices with 8 .. 15 neighbours
    const dim3 lgrid{unsigned((16 * z[23] + kRingBlock - 1) / kRingBlock)};  // sixteen lanes per row
    if (mass)
      hipLaunchKernelGGL((k_p1_long_rows<T, true>), lgrid, block, 0, L.stream, a.coords, a.plan, unsigned(z[22]),
                         int(z[23]), a.vals, a.stiff_w, a.mass_d, a.mass_o);
    else
      hipLaunchKernelGGL((k_p1_long_rows<T, false>), lgrid, block, 0, L.stream, a.coords, a.plan, unsigned(z[22]),
                         int(z[23]), a.vals, a.stiff_w, a.mass_d, a.mass_o);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(TFEM_ERR_HIP, "long-row kernel launch: %s", hipGetErrorString(e));
  }
  return TFEM_OK;
}

// The exported launches (tfem_p1_assemble_rings*): argument checks, the launch description and
// the developer switch TFEM_RINGS_PER_CU (tools/time_rings.py).
static int ring_entry(const void *coords, int real_bytes, int64_t n_verts, int quad_order, double alpha,
                      double beta, const void *plan_device, const int64_t *plan_layout_host, void *vals,
                      int64_t nnz, const void *fq, const tfem_source_program *source, int64_t n_elems,
                      void *fout, int64_t tile_first, int64_t tile_count, void *stream) {
  if (real_bytes != 4 && real_bytes != 8)
    return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host) return fail(TFEM_ERR_INVALID_ARGUMENT, "plan_layout_host is NULL");
  RingLaunch L{coords, quad_order, alpha, beta, static_cast<const unsigned char *>(plan_device),
               plan_layout_host, n_verts, nnz, vals, static_cast<hipStream_t>(stream)};
  L.fq = fq;
  L.source = source;
  L.n_elems = n_elems;
  L.fout = fout;
  L.tile_first = tile_first;
  L.tile_count = tile_count;
  if (const char *v = std::getenv("TFEM_RINGS_PER_CU")) L.blocks_per_cu = std::atoi(v);
  return real_bytes == 8 ? launch_rings<double>(L) : launch_rings<float>(L);
}

}  // namespace tfem

extern "C" {

int tfem_p1_rings_source_ops(const void *coords, int real_bytes, int quad_order, const int64_t *plan_layout_host,
                             const tfem_source_program *source, uint8_t *ops_out) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8) return fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host || !source || !ops_out) return fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  TriTables tables;
  if (!build_tri_tables(quad_order, real_bytes, &tables))
    return fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  return real_bytes == 8 ? ring_src_ops<double>(plan_layout_host, coords, tables.nq, source, ops_out)
                         : ring_src_ops<float>(plan_layout_host, coords, tables.nq, source, ops_out);
}

int tfem_p1_rings_source_route(const void *coords, int real_bytes, int quad_order, const int64_t *plan_layout_host,
                               const tfem_source_program *source) {
  using namespace tfem;
  if (real_bytes != 4 && real_bytes != 8) return -fail(TFEM_ERR_INVALID_ARGUMENT, "real_bytes must be 4 or 8");
  if (!plan_layout_host || !source) return -fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  TriTables tables;
  if (!build_tri_tables(quad_order, real_bytes, &tables))
    return -fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  const int st = src_validate(source);
  if (st != TFEM_OK) return -st;
  return real_bytes == 8 ? ring_src_route<double>(plan_layout_host, coords, tables.nq, source)
                         : ring_src_route<float>(plan_layout_host, coords, tables.nq, source);
}

int tfem_p1_rings_source_weights(const void *coords, int real_bytes, int quad_order, const int64_t *plan_layout_host,
                                 const tfem_source_program *source, double *weights_out) {
  using namespace tfem;
  if (!weights_out) return -fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  const int route = tfem_p1_rings_source_route(coords, real_bytes, quad_order, plan_layout_host, source);
  if (route < 0) return route;
  TriTables tables;
  if (!build_tri_tables(quad_order, real_bytes, &tables))
    return -fail(TFEM_ERR_UNSUPPORTED, "Integration order not implemented");
  double qsym[6] = {};
  if (tables.nq == 4 && real_bytes == 8) {
    if (!ring_rule_structure<double>(tables, qsym))
      return -fail(TFEM_ERR_UNSUPPORTED, "the 4-point rule is not the reference's order-3 rule");
    if (route == 2) ring_separable_weights<double>(source, qsym);
  }
  for (int i = 0; i < 3; ++i) weights_out[i] = qsym[3 + i];
  return route;
}

int tfem_ring_capacity(int what) {
  using namespace tfem;
  switch (what) {
    case 0: return kRingBlock;
    case 1: return kRingVertCap;
    default: return 0;
  }
}

int tfem_p1_assemble_rings(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                           double alpha, double beta, const void *plan_device,
                           const int64_t *plan_layout_host, void *vals, int64_t nnz,
                           const void *fq, int64_t n_elems, void *fout, void *stream) {
  return tfem::ring_entry(coords, real_bytes, n_verts, quad_order, alpha, beta, plan_device, plan_layout_host, vals,
                          nnz, fq, nullptr, n_elems, fout, 0, -1, stream);
}

int tfem_p1_assemble_rings_source(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                                  double alpha, double beta, const void *plan_device,
                                  const int64_t *plan_layout_host, void *vals, int64_t nnz,
                                  const tfem_source_program *source, int64_t n_elems, void *fout,
                                  void *stream) {
  if (!source) return tfem::fail(TFEM_ERR_INVALID_ARGUMENT, "NULL pointer");
  return tfem::ring_entry(coords, real_bytes, n_verts, quad_order, alpha, beta, plan_device, plan_layout_host, vals,
                          nnz, nullptr, source, n_elems, fout, 0, -1, stream);
}

int tfem_p1_assemble_rings_range(const void *coords, int real_bytes, int64_t n_verts, int quad_order,
                                 double alpha, double beta, const void *plan_device,
                                 const int64_t *plan_layout_host, void *vals, int64_t nnz, const void *fq,
                                 const tfem_source_program *source, int64_t n_elems, void *fout,
                                 int64_t tile_first, int64_t tile_count, void *stream) {
  return tfem::ring_entry(coords, real_bytes, n_verts, quad_order, alpha, beta, plan_device, plan_layout_host, vals,
                          nnz, fq, source, n_elems, fout, tile_first, tile_count, stream);
}

}  // extern "C"
