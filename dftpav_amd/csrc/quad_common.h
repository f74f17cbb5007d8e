// quad_common.h -- row-of-16-lanes primitives of the QUAD shapes of the reference order (solver_ref4.hip: one gear segment;
// solver_ref4m.hip: several): a row of a wave is a trajectory, its sixteen lanes are its pieces.  The substitution sweeps with the
// rows in registers (quad_sweep and its two row updates), and the sizes of solver_ref4.hip's LDS.
#pragma once
#include <utility>

#include "ref_order_common.h"

namespace dftpav {
namespace reford {

// acc + v[lane 0 of the row] + v[lane 1] + ... + v[lane 15]: sixteen dependent additions, every lane of a row ends with its
// row's sum.  (fma(v, 1.0, acc) == acc + v rounded once.  A VALU write followed by a DPP read needs two wait states and the asm
// block is opaque to the hazard recogniser: s_nop 1 in front.)
__device__ __forceinline__ double row_chain16(double acc, double v) {
  const double one = 1.0;
  asm volatile("s_nop 1\n\t" DFTPAV_FMAC_BCAST16 : "+v"(acc) : "v"(v), "v"(one));
  return acc;
}
// three such chains, link by link side by side: a0 += v0[lane k], a1 += v1[lane k], a2 += v2[lane k] for k = 0 .. 15.  Each sum takes
// its sixteen additions in row_chain16's order, one rounding per link; a link waits for its own chain's previous one only, so the
// three dependent latencies overlap.  (A -0.0 in v leaves its sum as it is: fma(-0.0, 1.0, a) rounds a + (-0.0) once, which is a for
// every a -- for a = +0.0 too, the sum of +0.0 and -0.0 being +0.0 in round-to-nearest -- and no sum here starts from -0.0.)
#define DFTPAV_FMAC_BCAST3(K)                                                    \
  "v_fmac_f64_dpp %0, %3, %6 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t" \
  "v_fmac_f64_dpp %1, %4, %6 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t" \
  "v_fmac_f64_dpp %2, %5, %6 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void row_chain16x3(double &a0, double &a1, double &a2, double v0, double v1, double v2) {
  const double one = 1.0;
  asm volatile("s_nop 1\n\t" DFTPAV_FMAC_BCAST3(0) DFTPAV_FMAC_BCAST3(1) DFTPAV_FMAC_BCAST3(2) DFTPAV_FMAC_BCAST3(3) DFTPAV_FMAC_BCAST3(4)
               DFTPAV_FMAC_BCAST3(5) DFTPAV_FMAC_BCAST3(6) DFTPAV_FMAC_BCAST3(7) DFTPAV_FMAC_BCAST3(8) DFTPAV_FMAC_BCAST3(9) DFTPAV_FMAC_BCAST3(10)
               DFTPAV_FMAC_BCAST3(11) DFTPAV_FMAC_BCAST3(12) DFTPAV_FMAC_BCAST3(13) DFTPAV_FMAC_BCAST3(14) DFTPAV_FMAC_BCAST3(15)
               : "+v"(a0), "+v"(a1), "+v"(a2)
               : "v"(v0), "v"(v1), "v"(v2), "v"(one));
}
// how many of the row's sixteen values v are <= k (k the lane's own): sixteen compare-adds over row_newbcast, no LDS and no branch
template <int... U> __device__ __forceinline__ int row_count_le_(int v, int k, std::integer_sequence<int, U...>) {
  return (0 + ... + (__builtin_amdgcn_update_dpp(0, v, 0x150 + U, 0xf, 0xf, false) <= k ? 1 : 0));
}
__device__ __forceinline__ int row_count_le(int v, int k) { return row_count_le_(v, k, std::make_integer_sequence<int, 16>{}); }
// acc + v[lane 0 of the row]
__device__ __forceinline__ double row_add_lane0(double acc, double v) {
  const double one = 1.0;
  asm volatile("s_nop 1\n\t" DFTPAV_FMAC_BCAST(0) : "+v"(acc) : "v"(v), "v"(one));
  return acc;
}
// max over the 16 lanes of a row (order-free), the same value in every lane of the row
__device__ __forceinline__ double row_max16(double v) {
  v = fmax(v, mov_dpp<0xB1>(v));
  v = fmax(v, mov_dpp<0x4E>(v));
  v = fmax(v, mov_dpp<0x141>(v));
  v = fmax(v, mov_dpp<0x140>(v));
  return v;
}
// the neighbour's value: lane l - 1 (row_shr:1) / lane l + 1 (row_shl:1) of the same row; 0.0 where there is none
template <int CTRL> __device__ __forceinline__ double nb_dpp(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// ---- BandedSystem::solve / solveAdj (poly_traj_utils.hpp:805-852) with the rows in registers: sweep Q of ref_order_common.h's packed
// tables (0: forward substitution of solve, 1: its back substitution, 2, 3: solveAdj's), a block of six rows per piece.  A lane holds D
// dimensions of a block: R[D rr + d] = natural row rr, dimension d; w[D r + d]: the six previous results in traversal order
// (traversal row r is natural row r in the ascending sweeps, 5 - r in the descending ones); a finished row takes its place in w.
// Traversal row r of a block of the ends (ce: the whole row, four coefficient pairs): every coefficient is tested, as the reference
// does (`if (a != 0.0)`); the row's multiply-subtract pairs in the reference's order
template <int Q, int D>
__device__ __forceinline__ void sweep_row_end(int r, const v2d_t (&ce)[4], double (&w)[6 * D], double (&R)[6 * D]) {
  constexpr bool DESC = Q == 1 || Q == 3, DIV = Q == 1 || Q == 2;
  const int rr = DESC ? 5 - r : r;
#pragma unroll
  for (int d = 0; d < D; d++) {
    double acc = R[D * rr + d];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double ck = (k & 1) ? ce[k >> 1].y : ce[k >> 1].x;
      const double t = ck * w[D * ((r + k) % 6) + d];
      acc = ck != 0.0 ? acc - t : acc;
    }
    if (DIV) acc = div_by_rcp(acc, ce[3].x, ce[3].y);
    w[D * r + d] = acc;
    R[D * rr + d] = acc;
  }
}
// Traversal row r of an interior block (c: the lane's own block of the table): the non-zero terms only, no test
template <int Q, int D>
__device__ __forceinline__ void sweep_row_interior(int r, const v2d_t (&c)[pk_size(Q) / 2], double (&w)[6 * D], double (&R)[6 * D]) {
  constexpr bool DESC = Q == 1 || Q == 3, DIV = Q == 1 || Q == 2;
  auto at = [&](int o) { return (o & 1) ? c[o >> 1].y : c[o >> 1].x; };
  const int rr = DESC ? 5 - r : r;
#pragma unroll
  for (int d = 0; d < D; d++) {
    double acc = R[D * rr + d];
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (pk_mask(Q, r) & (1 << k)) acc = acc - at(pk_off(Q, r, k)) * w[D * ((r + k) % 6) + d];
    if (DIV) acc = div_by_rcp(acc, at(pk_diag0(Q) + 2 * r), at(pk_diag0(Q) + 2 * r + 1));
    w[D * r + d] = acc;
    R[D * rr + d] = acc;
  }
}
// One substitution sweep with a piece per lane, both dimensions (D = 2): bq[2 r + d] = row 6 lp + r, dimension d, of this lane's piece
// (solver_ref.hip: sweep / rows_end / rows_pack -- the same rows, the same order of a row's updates).  Step s of the traversal belongs
// to piece s (ascending sweeps) or N - 1 - s (descending) of every segment on the row, the segments side by side; the six previous
// results it starts from are the finished rows of the previous step's piece, i.e. the neighbour lane's registers; a segment's first
// block starts from zeros, whatever the neighbour lane (another segment's last piece) holds.
// tabq: sweep Q of this lane's segment's tables (blocks in traversal order: whole rows at the two ends, the interior pattern's
// coefficients in between); lp, N: the lane's piece inside its segment, the segment's pieces; piece: the lane has one at all; Nmax: the
// largest segment's pieces.  (One segment, solver_ref4.hip: lp = l, piece = l < N, Nmax = N.)
template <int Q>
__device__ __forceinline__ void quad_sweep(ldscd_t tabq, double (&bq)[12], int lp, int N, bool piece, int Nmax) {
  constexpr bool DESC = Q == 1 || Q == 3;
  ldscd_t ip = tabq + 48;
  // the table of this lane's own block (an interior block: pk_size(Q) doubles), read once, in front of the traversal
  v2d_t c[pk_size(Q) / 2];
  {
    const int sl = DESC ? N - 1 - lp : lp; // the step this lane's piece is taken in
    const int bi = sl >= 1 && sl <= N - 2 ? sl - 1 : 0;
    const ldscv2_t a = (ldscv2_t)(ip + bi * pk_size(Q));
    if (N > 2) {
#pragma unroll
      for (int u = 0; u < pk_size(Q) / 2; u++) c[u] = a[u];
    } else {
#pragma unroll
      for (int u = 0; u < pk_size(Q) / 2; u++) c[u] = v2d_t{0.0, 0.0};
    }
  }
#pragma unroll 1
  for (int s = 0; s < Nmax; s++) {
    const int p = DESC ? N - 1 - s : s;
    double w[12];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int d = 0; d < 2; d++) w[2 * r + d] = DESC ? nb_dpp<0x101>(bq[2 * (5 - r) + d]) : nb_dpp<0x111>(bq[2 * r + d]);
    if (s == 0) { // (uniform) every segment's traversal starts from six zeros, whatever the neighbour lane holds
#pragma unroll
      for (int u = 0; u < 12; u++) w[u] = 0.0;
    }
    const bool mine = piece && s < N && lp == p;
    if (mine && (s == 0 || s == N - 1)) { // a block of the ends, its table rows loaded row by row
      const ldscv2_t a = (ldscv2_t)(s == 0 ? tabq : ip + (N - 2) * pk_size(Q));
#pragma unroll
      for (int r = 0; r < 6; r++) {
        v2d_t ce[4];
#pragma unroll
        for (int u = 0; u < 4; u++) ce[u] = a[4 * r + u];
        sweep_row_end<Q, 2>(r, ce, w, bq);
      }
    } else if (mine) { // an interior block
#pragma unroll
      for (int r = 0; r < 6; r++) sweep_row_interior<Q, 2>(r, c, w, bq);
    }
  }
}

// DENSE emission (round 6): the active terms the lanes of a wave find in the point loop are listed -- (owner lane, point, term, the
// point's running offset s1, the half-plane of a corridor term) -- and evaluated kDense at a time, one per lane, by whichever lanes
// the list numbers: the owner's coefficients come over by ds_bpermute, the point's state is formed again by the same expressions
// (the same bits), what the term adds goes back through LDS and the owner adds its terms in list order = (point, term) order.  In
// place, a lane with k active terms ran k trips of the emission while the other 63 waited: 26-29 trips of ~2.2 k cycles per evaluation
// of four trajectories with three lanes active on average (55-65 k cycles, 15 % of a pass).
// (solver_ref4m.hip, several gear segments: tried and not kept -- its kernel has no registers left for the list's code: 64 bytes of
// scratch per lane and 165 -> 171 ms per step of configs[1]'s stream)
// LDS of the QUAD shape with one gear segment (solver_ref4.hip): the four sweep tables of a workgroup, a row's share (struct Q4 there)
constexpr int kQPool = 64; // parked terms of a trajectory kept in LDS (solver_ref4.hip)
__host__ __device__ constexpr size_t q4_team_doubles(int mem) { return 32 + 32 + 12 + 6 + sNUM + (size_t)mem + kQPool * 3 + kQPool / 8; }
__host__ __device__ constexpr size_t q4_team_bytes(int mem) { return (q4_team_doubles(mem) * sizeof(double) + iNUM * sizeof(int) + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t q4_shared_bytes(int N) { return ((size_t)pk_segment_doubles(N) * sizeof(double) + 15) & ~(size_t)15; }
// A list entry: id 4, s1 8, and 15 doubles that hold the half-plane of a corridor term (4) until the worker has read it and the
// term's result (15) from then on -- the two never coexist.
constexpr size_t kDenseEntryBytes = 4 + 8 + 15 * 8;
__host__ __device__ constexpr size_t q4_dense_bytes_of(int k) { return ((size_t)k * kDenseEntryBytes + 15) & ~(size_t)15; }
// The list is as long as the LDS allows with FOUR single-wave workgroups on a CU (160 KB; solver_ref.hip: quad_shape -- the sum is
// reference_order_quad_supported's) at the largest tables (16 pieces) and the product's history length (capi.cpp: lbfgs_mem_size = 256):
// the largest multiple of 8, a wave's 64 lanes at most (one pass of the flush), 8 at least.
constexpr int kDenseSizedForN = 16, kDenseSizedForMem = 256;
__host__ __device__ constexpr int q4_dense_capacity(int N, int mem) {
  int k = 64;
  while (k > 8 && 4 * (q4_shared_bytes(N) + 4 * q4_team_bytes(mem) + q4_dense_bytes_of(k)) > (size_t)160 * 1024) k -= 8;
  return k;
}
constexpr int kDense = q4_dense_capacity(kDenseSizedForN, kDenseSizedForMem);
static_assert(kDense % 8 == 0 && kDense >= 8 && kDense <= 64, "a lane's slots of the list are the bits of a 64-bit mask (solver_ref4.hip: mine |= 1ull << e)");
static_assert(4 * (q4_shared_bytes(kDenseSizedForN) + 4 * q4_team_bytes(kDenseSizedForMem) + q4_dense_bytes_of(kDense)) <= (size_t)160 * 1024,
              "four workgroups of one wave share a CU's LDS at 16 pieces and a history of 256");
typedef unsigned long long dmask_t; // a lane's / a row's slots of the list
// DenseLds::id packs an entry into an int: the owner lane in bits 0-5 (lane & 63), the term in bits 6-11, the point from bit 12 on.
// Term and point are run-time values: the term is < 5 H + 4 <= 29 (reference_order_quad_supported: H <= 5); the point is <= Kmax + 1,
// which keeps the id positive while Kmax + 1 < 2^19 -- no predicate bounds K.
constexpr int kDenseIdLaneBits = 6, kDenseIdTermBits = 6; // (solver_ref4.hip: flush reads them back with & 63, >> 6 & 63, >> 12)
constexpr int kQuadMaxH = 5;                              // reference_order_quad_supported: H <= 5
static_assert(64 <= (1 << kDenseIdLaneBits), "the owner lane of a wave of 64 fits its field of the id");
static_assert(5 * kQuadMaxH + 4 <= (1 << kDenseIdTermBits), "a point's 5 H + 4 terms fit the term field of the id");
static_assert(kDenseIdLaneBits + kDenseIdTermBits == 12, "the point starts at bit 12 of the id");
struct DenseLds {
  ldsi_t id;   // [kDense] owner lane | term << 6 | point << 12
  ldsd_t s1;   // [kDense]
  ldsd_t out;  // [kDense][15] first the half-plane of a corridor term (4), then gdC (12), gdT, corridor cost, feasibility cost
};
__host__ __device__ constexpr size_t q4_dense_bytes() { return q4_dense_bytes_of(kDense); }
__device__ inline void q4_carve_dense(DenseLds &d, char *base) {
  ldsd_t p = (ldsd_t)reinterpret_cast<double *>(base);
  d.s1 = p; p += kDense;
  d.out = p; p += 15 * kDense;
  d.id = (ldsi_t)p;
}

} // namespace reford
} // namespace dftpav
