// solver_ref4.hip — the reference order in the QUAD shape: FOUR trajectories per wave, one per row of 16 lanes (gfx950).
//
// solver_ref.hip's WAVE shape gives a trajectory a wave of its own.  Its sequential sums are chains of v_fmac_f64_dpp
// row_newbcast:K, and such an instruction costs the same whether one row of the wave wants its result or all four do; its band
// substitutions run on 2 of 64 lanes.  A wave there serves ONE trajectory per instruction, and the kernel is issue-bound
// (profiles/r05_*: 15.0 M vector instructions per solve, two-loop recursion at its issue rate).  Here a row of 16 lanes is a
// trajectory, so every chain instruction, every step of a substitution and every step of the line search serves four:
//
//   * lane l of a row OWNS PIECE l of its trajectory (one gear segment of at most 16 pieces): the piece's six rows of the band
//     system (both dimensions), its coefficients c, its gdC and its adjoint live in that lane's REGISTERS -- no LDS copy of
//     b / c / gdC / adj at all (they were 6.1 of the WAVE shape's 18.2 KB per trajectory);
//   * BandedSystem::solve / solveAdj (poly_traj_utils.hpp:805-852): the row sweeps of solver_ref.hip, piece by piece -- at step s
//     the lane that owns block s takes the six results of the previous block from its neighbour's registers (DPP row_shr / row_shl)
//     and computes its own six rows, both dimensions side by side; the row's multiply-subtract pairs in the reference's order
//     (quad_common.h: quad_sweep, the traversal solver_ref4m.hip runs too, and the two row updates sweep_row_end / sweep_row_interior;
//     16 pieces: the two dimensions of a piece on two lanes, six rows per step -- sweep4_split below, over the same row updates);
//   * addPVAGradCost2CT (traj_optimizer.cpp:486-705): lane l walks the K + 1 constraint points of ITS piece in order (the running
//     s1 += step of :513 is a register), and what an active term adds to gdC goes straight into the lane's own gdC registers --
//     the order a gdC entry receives its additions in is (point, term) order within the piece, which is all the reference's order
//     says about it.  No 16-double records, no chain pass.  Only what the term adds to the segment's gdT and to the two costs
//     (three doubles) is parked -- in one pool per trajectory, in arrival order -- and chained afterwards in (piece, point, term)
//     order through a permutation of the pool's slots (q4_eval: the chain pass).  The active terms themselves are
//     EVALUATED densely packed: listed by the lanes that find them, taken up to kDense = 64 at a time one per lane (a whole wave in one
//     pass: the list is as long as the LDS left beside four workgroups' rows and tables allows, quad_common.h), their results handed
//     back to the owners through LDS in list order (quad_common.h: DenseLds; q4_eval: flush).  An entry's half-plane and its result
//     share their LDS: 132 bytes per entry.  With 24 entries of 164 bytes the list was emptied 3.9 times per evaluation of the bench's
//     batch at some 7 k cycles each (profiles/dense_list_phases.txt);
//   * the corridor is read from a copy laid out [component][j][piece]: the 16 lanes of a row read 128 contiguous bytes; a batch whose
//     corridors are all rectangles (q4_rect_check_kernel) reads a copy of 10 doubles per point instead of 16 (RECT, below);
//   * lbfgs_optimize / line_search_lewisoverton (lbfgs.hpp:276-390, 440-751): lbfgs_control.h's lbfgs_advance, per row (quad_lbfgs.h:
//     the row's vector operations under it, the record of a suspended trajectory and the shape-free pieces of the loop, shared with solver_ref4m.hip;
//     this file: Q4Shape, the recursion and the mirror of the ring's ends); a vector of
//     n <= 32 variables is two registers per lane (elements l and 16 + l), a sequential dot product is the 32-step DPP chain --
//     each row chains its own sixteen lanes, no permlane swap -- and the two-loop recursion (:716-739) runs the four rows' history
//     steps in the same instructions (a row that is still in its line search, or has the shorter history, is masked).
//
// Same bits as the TEAM / WAVE shapes (every sum is the same chain; tests/test_gpu_reference_order.py compares the shapes with one
// another, with the restatement and with the golden vectors).  Scope: one gear segment, N <= 16 pieces, n <= 32, no moving
// obstacles, H <= 5 -- the BASELINE configs[2] / [3] workload; everything else stays with solver_ref.hip.
//
// Residency: ONE wave per SIMD (the kernel takes 460 registers; built for two waves per SIMD it spilled 205 of them and its scratch
// traffic alone was HBM-sized), four waves = 16 trajectories per CU (8 in the WAVE shape), each wave at the speed of a wave that has
// its SIMD to itself; 4.6 KB of LDS per trajectory (x, g, the boundary states, the scalars of the line search, alpha[mem], a pool
// of 64 parked terms and its permutation) and 8.3 KB per wave for the list of active terms (38.7 of the 40 KB a workgroup may take at 16 pieces and a history of 256), workgroups of one wave with a copy of the sweep
// tables each (39 KB; a wave that has nothing
// left to do frees its slot at once).  Scheduling as the WAVE shape: the rows pop trajectories from the batch's ring, run them a
// slice of evaluations and push them back unfinished, so that a wave's rows stay filled until the batch runs out.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>

#include "ref_order_common.h"
#include "quad_lbfgs.h"

namespace dftpav {
namespace reford {

// Parked terms of a trajectory kept in LDS, in one pool filled in arrival order (the rest in global scratch).  A slot's number is a
// bit of a lane's 64-bit mask and a byte of the row's permutation table.  (kQPool = 64: quad_common.h, with the sizes of the LDS)
static_assert(kQPool <= 64 && kQPool % 8 == 0, "a lane's pool slots are the bits of a 64-bit mask; the chain pass reads the permutation eight bytes at a time");
typedef unsigned char __attribute__((address_space(3))) *ldsb_t;
typedef const unsigned long long __attribute__((address_space(3))) *ldscu64_t;
// Waves per SIMD the kernel is built for.  At 2 (256 registers) it spills 205 of them and its scratch traffic alone is HBM-sized
// (measured: the point loop 3 x slower than at 1); at 1 the allocator takes 455 registers, nothing goes to scratch, and four waves
// per CU hold 16 trajectories -- twice the WAVE shape's 8 -- each of them at the speed of a wave that has its SIMD to itself.
#ifndef DFTPAV_Q4_WAVES_PER_EU
#define DFTPAV_Q4_WAVES_PER_EU 1
#endif
constexpr int kQ4WavesPerCU = 4 * DFTPAV_Q4_WAVES_PER_EU;

// LDS of one trajectory (a row)
struct Q4 {
  ldsd_t xs, gs;  // [32] the trial point, the gradient (the interface between the evaluation and the solver)
  ldsd_t bnd;     // [12] iniS [6], finS [6] as uploaded (clamped)
  ldsd_t tw;      // [6] 1 / t^k of the piece duration of the evaluation in progress
  ldsd_t st;      // [sNUM]
  ldsd_t alpha;   // [mem]
  ldsd_t pool;    // [kQPool][3] parked terms in arrival order: what they add to gdT, to the corridor cost, to the feasibility cost
  ldsb_t perm;    // [kQPool] the pool slots in (piece, point, term) order, a byte each
  ldsi_t ist;     // [iNUM]
};
// (q4_team_doubles / q4_team_bytes / q4_shared_bytes: quad_common.h -- the length of the list of active terms follows from them)
__device__ inline void q4_carve(Q4 &q, char *team, int mem) {
  ldsd_t p = (ldsd_t)reinterpret_cast<double *>(team);
  q.xs = p; p += 32;
  q.gs = p; p += 32;
  q.bnd = p; p += 12;
  q.tw = p; p += 6;
  q.st = p; p += sNUM;
  q.alpha = p; p += mem; // (16-byte aligned: q4_first_block stores two doubles at a time)
  q.pool = p; p += kQPool * 3;
  q.perm = (ldsb_t)p; p += kQPool / 8;
  q.ist = (ldsi_t)p;
}

// 0.0 + p[0] + p[1] + ... + p[n-1] for a vector held as (element l, element 16 + l); elements from n on contribute -0.0, and
// x + (-0.0) == x for every x: the second half of the chain is left out when it has nothing but those
__device__ __forceinline__ double row_sum32(double p0, double p1, int n, int l) {
  double acc = row_chain16(0.0, l < n ? p0 : -0.0);
  if (n > 16) acc = row_chain16(acc, 16 + l < n ? p1 : -0.0); // (uniform)
  return acc;
}
// The same sweep for N = 16 with the two DIMENSIONS of a piece on two LANES (round 6).  In quad_sweep (quad_common.h) the lane that owns block s computes its
// twelve rows -- six per dimension, two independent chains -- while fifteen lanes wait; here a lane holds two SETS of six rows:
//   X = (piece l, dimension 0) for l < 8, (piece l - 8, dimension 1) for l >= 8;   Y = (piece l + 8, dimension 1) for l < 8, (piece l, dimension 0) for l >= 8
// so that block p of both dimensions is in one set on the two lanes p mod 8 and p mod 8 + 8, and a step of the traversal is SIX rows of
// one instruction stream for both.  Pieces 0 .. 7 are in X, 8 .. 15 in Y: an ascending sweep runs eight steps on X, then eight on Y (a
// descending one Y, then X); the previous block's results are the neighbour lane's rows of the same set (lanes 7 / 8 and 15 / 0 are not
// neighbours in the chains they split: harmless, a chain's first block starts from zeros), except at the ninth step, which takes them from
// the other set one lane around the row (row_ror).  Per row the same products and differences in the same order: the same bits.
__device__ __forceinline__ void q4_split(const double (&bq)[12], double (&X)[6], double (&Y)[6], int l) {
  const bool lo = (l & 8) == 0;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    const double own = bq[2 * r], far = nb_dpp<0x128>(bq[2 * r + 1]); // dimension 1 of piece (l + 8) mod 16
    X[r] = lo ? own : far;
    Y[r] = lo ? far : own;
  }
}
__device__ __forceinline__ void q4_unsplit(const double (&X)[6], const double (&Y)[6], double (&bq)[12], int l) {
  const bool lo = (l & 8) == 0;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    bq[2 * r] = lo ? X[r] : Y[r];
    bq[2 * r + 1] = nb_dpp<0x128>(lo ? Y[r] : X[r]); // this piece's dimension 1, from the lane eight around the row
  }
}
// The traversal: the first end block, seven interior steps on the first set, seven on the second, the last end block.  The two end
// blocks (24 table reads and a test per coefficient each) stand outside the loops, so a loop's body is one interior step and nothing
// else: 55-64 instructions where the loop that also held the end block had 78-104 per interior step (profiles/sweep_step_static.txt).
template <int Q>
__device__ __forceinline__ void sweep4_split(ldscd_t tab, double (&X)[6], double (&Y)[6], int l) {
  constexpr bool DESC = Q == 1 || Q == 3, DIV = Q == 1 || Q == 2;
  constexpr int N = 16;
  ldscd_t ip = tab + 48;
  const int l8 = l & 7;
  // the previous block's six results, in traversal order: the neighbour lane's rows of the same set
  auto fetch = [&](const double (&R)[6], double (&w)[6]) {
#pragma unroll
    for (int r = 0; r < 6; r++) w[r] = DESC ? nb_dpp<0x101>(R[5 - r]) : nb_dpp<0x111>(R[r]);
  };
  // a block of the ends (step 0 and step N - 1 of the traversal, outside the loops): every coefficient is tested, as the reference
  // does (`if (a != 0.0)`).  Its six table rows are requested together (one wait, not one per row) by whoever is here -- the address
  // is the wave's -- and the rows run for the owner lanes only (the caller's branch).
  auto end_request = [&](v2d_t (&cb)[6][4], ldscv2_t a) {
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int u = 0; u < (DIV ? 4 : 3); u++) cb[r][u] = a[4 * r + u];
    asm volatile("" ::: "memory"); // (keeps the reads where they stand: ahead of the arithmetic, ahead of a loop)
  };
  auto end_rows = [&](double (&R)[6], double (&w)[6], const v2d_t (&cb)[6][4]) {
#pragma unroll
    for (int r = 0; r < 6; r++) sweep_row_end<Q, 1>(r, cb[r], w, R);
  };
  // the seven interior steps s1 .. s1 + 6 of one set: the non-zero terms only, no test.  w: what step s1 starts from; on return,
  // what the step behind the last one starts from (each step ends by fetching for the next).  ahead: what the caller wants requested
  // behind this set's table and in front of the loop.
  // SELECT form: every lane runs every step on its own table block and its own rows, and only the step's owner keeps the result
  // (twelve v_cndmask): no branch and no EXEC write in a step.  What a lane that is not the owner computes is dropped and touches
  // nothing else: it reads registers only, c is a whole interior block of the table for every lane (bi below), R holds right-hand
  // sides or finished rows (zeros where a trajectory has nothing) and w what the neighbour handed over or 0.0, so the operands are
  // finite; no floating-point exception traps in this kernel, no address and no store depends on the values, and w is fetched
  // afresh at the end of the step.  The owner's products, differences and div_by_rcp are sweep_row_interior's, in its order.
  auto interior = [&](double (&R)[6], int s1, double (&w)[6], auto ahead) {
    // the table of this lane's own block of the set (pk_size(Q) doubles), read once
    v2d_t c[pk_size(Q) / 2];
    {
      const int sl = (s1 & 8) + (DESC ? 7 - l8 : l8); // the step this lane's block of the set is taken in
      const int bi = sl >= 1 && sl <= N - 2 ? sl - 1 : 0;
      const ldscv2_t a = (ldscv2_t)(ip + bi * pk_size(Q));
#pragma unroll
      for (int u = 0; u < pk_size(Q) / 2; u++) c[u] = a[u];
    }
    ahead();
#pragma unroll 1
    for (int s = s1; s < s1 + 7; s++) {
      const bool own = l8 == ((DESC ? N - 1 - s : s) & 7);
      double T[6];
#pragma unroll
      for (int r = 0; r < 6; r++) T[r] = R[r];
#pragma unroll
      for (int r = 0; r < 6; r++) sweep_row_interior<Q, 1>(r, c, w, T);
#pragma unroll
      for (int r = 0; r < 6; r++) R[r] = own ? T[r] : R[r];
      fetch(R, w);
    }
  };
  double (&A)[6] = DESC ? Y : X; // the set of the traversal's first eight blocks
  double (&B)[6] = DESC ? X : Y; // and of its last eight
  double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // the traversal starts from six zeros
  if (l8 == (DESC ? 7 : 0)) {
    v2d_t cb[6][4];
    end_request(cb, (ldscv2_t)tab);
    end_rows(A, w, cb);
  }
  fetch(A, w);
  interior(A, 1, w, [] {});
  // the ninth step starts from the eighth block's results: the other set, one lane around the row
#pragma unroll
  for (int r = 0; r < 6; r++)
    w[r] = DESC ? nb_dpp<0x12F>(A[5 - r])  // lane 7 <- lane 8 (piece 8, dimension 0), lane 15 <- lane 0 (piece 8, dimension 1)
                : nb_dpp<0x121>(A[r]);     // lane 8 <- lane 7 (piece 7, dimension 0), lane 0 <- lane 15 (piece 7, dimension 1)
  // the last end block's table rows are requested in front of the second loop, in one request: they have arrived when the loop ends
  // (by every lane that is here, not by the owner lanes alone: no branch in front of the loop.  Measured: without this request the
  // select form gains nothing on the value line, docs/HISTORY.md)
  v2d_t ce[6][4];
  interior(B, 8, w, [&] { end_request(ce, (ldscv2_t)(ip + (N - 2) * pk_size(Q))); });
  if (l8 == (DESC ? 0 : 7)) end_rows(B, w, ce);
}

// ------------------------------------------------ costFunctionCallback (traj_optimizer.cpp:206-350), one gear segment
// x (q.xs) -> g (q.gs), returns f.  The statements are solver_ref.hip's ref_eval, stage by stage; what changes is where a value
// lives.  (The per-piece MINCO steps -- durations, jerk energy, gdtInv sum, the duration gradient's head / tail terms -- are written out
// here although ref_eval and q4m_eval call ref_order_common.h's functions for them: with the calls this kernel kept its registers but
// the headline lost 2 % on the device, docs/HISTORY.md.)  cor: &cor_t[b][0][0][l] (component pitch cpitch = 16 (Kmax + 1), a round's 16 pieces contiguous); ovf: this
// trajectory's global scratch for the parked terms beyond the LDS window.
// FAST: the live path's constants known at compile time -- H = 4 half-planes per point (rectangles, traj_manager.cpp:1225) and
// help_eps = 0.0 (:610): the fifth plane slot and the second reciprocal of the curvature term drop out of the point loop.
// RECT (with FAST): every corridor of the batch is a rectangle whose four normals are (-S, C), (C, S), (S, -C), (-C, -S) with the same
// bits of C and S (q4_rect_check_kernel).  cor: &rect copy[b][0][0][l] in 16-byte units (q4_corridor_rect_kernel: [j][unit 5][piece 16],
// unit 0 = (C, S), units 1-4 = (p_x, p_y) of planes 0-3): five 16-byte loads per round from one base instead of sixteen 8-byte loads
// with an address each.  The normals are rebuilt by sign flips -- negation is exact, so every expression that uses them forms the bits
// it forms from the sixteen doubles.
struct RectSet { // a round's rectangle of one point
  d2_t u[5];
};
__device__ __forceinline__ void load_rect(gcd2_t cor, RectSet &r) {
#pragma unroll
  for (int u = 0; u < 5; u++) r.u[u] = cor[16 * u];
}
__device__ __forceinline__ void rect_planes(const RectSet &r, double (&pl)[20]) {
  const double C = r.u[0].x, S = r.u[0].y;
  pl[0] = -S; pl[1] = C;
  pl[4] = C; pl[5] = S;
  pl[8] = S; pl[9] = -C;
  pl[12] = -C; pl[13] = -S;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    pl[4 * k + 2] = r.u[1 + k].x;
    pl[4 * k + 3] = r.u[1 + k].y;
  }
#pragma unroll
  for (int u = 16; u < 20; u++) pl[u] = 0.0;
}
template <bool FAST, bool RECT>
__device__ __forceinline__ double q4_eval(const DevBatch &D, const Q4 &q, const DenseLds &dl, ldscd_t tab, gcd_t cor, size_t cpitch, gd_t ovf, int l, Prof &pr) {
  const DevLayout &L = D.L;
  const DevParams &P = D.P;
  const int N = L.Ntot, H = FAST ? 4 : L.H, nterm = 5 * H + 4, t0 = 5 * H;
  const double epis = FAST ? 0.0 : D.epis;
  // ---- durations (VirtualT2RealT, :371-379), their powers (poly_traj_utils.hpp:961-966)
  const double vt = q.xs[L.x_tau0];
  const double Tr = vt > 0.0 ? ((0.5 * vt + 1.0) * vt + 1.0) + P.mini_T : 1.0 / ((0.5 * vt - 1.0) * vt + 1.0) + P.mini_T;
  const double t1 = Tr / N, t2 = t1 * t1, t3 = t2 * t1, t4 = t2 * t2, t5 = t4 * t1;
  pr.tick(10); // (what a pass of the kernel's loop does around the evaluation)
  // ---- right-hand sides (poly_traj_utils.hpp:968-977): the rows of this lane's piece
  double bq[12];
#pragma unroll
  for (int u = 0; u < 12; u++) bq[u] = 0.0;
  if (l == 0) {
#pragma unroll
    for (int d = 0; d < 2; d++) {
      bq[0 + d] = q.bnd[d];
      bq[2 + d] = q.bnd[2 + d] * t1;
      bq[4 + d] = q.bnd[4 + d] * t2;
    }
  }
  if (l == N - 1) {
#pragma unroll
    for (int d = 0; d < 2; d++) {
      bq[6 + d] = q.bnd[6 + d];
      bq[8 + d] = q.bnd[8 + d] * t1;
      bq[10 + d] = q.bnd[10 + d] * t2;
    }
  } else if (l < N - 1) {
    bq[10] = q.xs[2 * l];
    bq[11] = q.xs[2 * l + 1];
  }
  // ---- BandedSystem::solve (poly_traj_utils.hpp:805-826)
  if (N == 16) { // (uniform)
    double X[6], Y[6];
    q4_split(bq, X, Y, l);
    sweep4_split<0>(tab, X, Y, l);
    sweep4_split<1>(tab + pk_sweep_offset(1, 16), X, Y, l);
    q4_unsplit(X, Y, bq, l);
  } else {
    quad_sweep<0>(tab, bq, l, N, l < N, N);
    quad_sweep<1>(tab + pk_sweep_offset(1, N), bq, l, N, l < N, N);
  }
  pr.tick(0);
  // ---- c = b * tInv (:979-984)
  double cc[12];
  {
    const double tI[6] = {1.0 / 1.0, 1.0 / t1, 1.0 / t2, 1.0 / t3, 1.0 / t4, 1.0 / t5};
#pragma unroll
    for (int u = 0; u < 12; u++) cc[u] = bq[u] * tI[u >> 1];
    if (l == 0) {
#pragma unroll
      for (int u = 0; u < 6; u++) q.tw[u] = tI[u]; // kept for calGrads_PT (six divisions, not six registers across the point loop)
    }
  }
  // ---- initSmGradCost / getTrajJerkCost per piece (poly_traj_utils.hpp:998-1035)
  double gdC[12], pE, pG;
  {
    const double *c = cc;
    const double t[6] = {1.0, t1, t2, t3, t4, t5};
    const double n33 = c[6] * c[6] + c[7] * c[7], n44 = c[8] * c[8] + c[9] * c[9], n55 = c[10] * c[10] + c[11] * c[11];
    const double d43 = c[8] * c[6] + c[9] * c[7], d53 = c[10] * c[6] + c[11] * c[7], d54 = c[10] * c[8] + c[11] * c[9];
    pE = 36.0 * n33 * t[1] + 144.0 * d43 * t[2] + 192.0 * n44 * t[3] + 240.0 * d53 * t[3] + 720.0 * d54 * t[4] + 720.0 * n55 * t[5];
    pG = 36.0 * n33 + 288.0 * d43 * t[1] + 576.0 * n44 * t[2] + 720.0 * d53 * t[2] + 2880.0 * d54 * t[3] + 3600.0 * n55 * t[4];
#pragma unroll
    for (int d = 0; d < 2; d++) {
      const double c3 = c[6 + d], c4 = c[8 + d], c5 = c[10 + d];
      gdC[10 + d] = 240.0 * c3 * t[3] + 720.0 * c4 * t[4] + 1440.0 * c5 * t[5];
      gdC[8 + d] = 144.0 * c3 * t[2] + 384.0 * c4 * t[3] + 720.0 * c5 * t[4];
      gdC[6 + d] = 72.0 * c3 * t[1] + 144.0 * c4 * t[2] + 240.0 * c5 * t[3];
      gdC[d] = 0.0;
      gdC[2 + d] = 0.0;
      gdC[4 + d] = 0.0;
    }
  }
  pr.tick(1);
  // ---- the constraint points of this lane's piece, in order (traj_optimizer.cpp:486-705)
  const bool piece = l < N;
  const int Kl = (l == 0 || l == N - 1) ? L.Kd : L.K;
  const int pt0 = l == 0 ? 0 : (L.Kd + 1) + (l - 1) * (L.K + 1); // the piece's first constraint point
  const double step = t1 / Kl;
  const int singul_ = L.singuls[0];
  double s1 = 0.0;
  int cnt = 0;                     // parked terms of this lane's piece
  int rcnt = 0;                    // parked terms of the row so far (the same in its sixteen lanes): the next pool slot
  unsigned long long pmask = 0ull; // the pool slots that hold terms of this lane's piece
  const gd_t ovf_l = ovf + (size_t)pt0 * nterm * 3;
  // a round's half-planes are requested one round ahead (the copy holds zeros where a piece has no such point: every lane
  // loads, whatever its piece): 33 rounds of a dependent HBM round trip each were 3/4 of this kernel's time
  double pl[20];
  RectSet rs; // RECT: the round's rectangle as loaded; pl is rebuilt from it at the head of a round
  const gcd2_t rcor = (gcd2_t)cor;
  if constexpr (RECT) load_rect(rcor, rs);
  else load_planes(cor, cpitch, H, pl);
  // (the first round's half-planes are waited for HERE: left pending into the loop, they make the compiler wait for ALL vector loads in front of
  // every round's first use of a half-plane -- its count of the loads in flight merges to zero at the loop's head -- and that includes the
  // next round's, requested a few hundred instructions earlier: the request ahead bought half a round instead of a whole one)
  __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
  // what an active term adds: to the lane's gdC in place, to gdT and to its cost parked (the other cost gets -0.0: x + (-0.0) == x)
  // slot: the term's number among its row's terms in arrival order -- (round, lane, term) order, so a piece's slots ascend in (point,
  // term) order, and its terms in the pool all arrive before its terms beyond it (those go to the piece's own place in global scratch)
  auto take = [&](const double (&r12)[12], double e0, double e1, double e2, int slot) {
#pragma unroll
    for (int u = 0; u < 12; u++) gdC[u] += r12[u];
    if (slot < kQPool) {
      ldsd_t e = q.pool + slot * 3;
      e[0] = e0;
      e[1] = e1;
      e[2] = e2;
      pmask |= 1ull << slot;
    } else {
      gd_t e = ovf_l + (size_t)cnt * 3;
      e[0] = e0;
      e[1] = e1;
      e[2] = e2;
    }
    cnt++;
  };
  // the list of the wave
  const int lane64 = (int)(threadIdx.x & 63);
  int listed = 0;       // (uniform) entries in the list
  dmask_t mine = 0ull;  // the list's slots that hold terms of this lane's piece
  // (the rows of a wave that have no trajectory are not here: EXEC holds whole rows of 16 lanes, any of the four)
  const unsigned long long here = __builtin_amdgcn_ballot_w64(true);
  const int row_here[4] = {(int)(here & 1ull), (int)((here >> 16) & 1ull), (int)((here >> 32) & 1ull), (int)((here >> 48) & 1ull)};
  const int my_row = lane64 >> 4;
  const int rank = ((my_row > 0 ? row_here[0] : 0) + (my_row > 1 ? row_here[1] : 0) + (my_row > 2 ? row_here[2] : 0)) * 16 + l; // among the lanes here
  const int n_here = 16 * (row_here[0] + row_here[1] + row_here[2] + row_here[3]);
  // inclusive prefix sum of c over the lanes that are here, and its total (wave_incl_scan_i32 wants all 64 lanes)
  // (row_incl: the prefix within the lane's own row, which numbers the pool slots of a round taken in place)
  auto scan_here = [&](int c, int &total, int &row_incl) {
    int v = c;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    row_incl = v;
    const int t0_ = row_here[0] ? __builtin_amdgcn_readlane(v, 15) : 0, t1_ = row_here[1] ? __builtin_amdgcn_readlane(v, 31) : 0;
    const int t2_ = row_here[2] ? __builtin_amdgcn_readlane(v, 47) : 0, t3_ = row_here[3] ? __builtin_amdgcn_readlane(v, 63) : 0;
    total = t0_ + t1_ + t2_ + t3_;
    return v + (my_row > 0 ? t0_ : 0) + (my_row > 1 ? t1_ : 0) + (my_row > 2 ? t2_ : 0);
  };
  auto flush = [&]() {
    for (int first = 0; first < listed; first += n_here) { // (uniform; a pass serves the n_here lanes that are here: one pass of a full wave, up to kDense / 16 where a single row is here)
    const int slot = first + rank;
    const bool work = slot < listed;
    const int id = dl.id[work ? slot : 0];
    const int o = id & 63, t = (id >> 6) & 63, jo = id >> 12;
    // the owner's piece: its coefficients and the piece duration of its row come over from the owner's registers
    double cco[12];
#pragma unroll
    for (int u = 0; u < 12; u++) cco[u] = __shfl(cc[u], o);
    const double t1o = __shfl(t1, o);
    const int lo = o & 15;
    const int Ko = (lo == 0 || lo == N - 1) ? L.Kd : L.K;
    const double stepo = t1o / Ko; // (the owner's expression: the same bits)
    if (work) {
      const double nopl[20] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      PtState ps;
      // the state of the owner's point by the expressions that found the term (its tests are not needed again: no half-planes)
      (void)point_masks<false>(P, cco, lo, N, jo, Ko, stepo, dl.s1[slot], singul_, epis, H, nopl, (gd_t) nullptr, D.sur, 0.0, 0.0, 0, 0.0, ps);
      double r_[16];
      // the entry's half-plane lies where its result goes: read whole, here, in front of the writes below
      ldsd_t w = dl.out + 15 * slot;
      const double pk[4] = {w[0], w[1], w[2], w[3]};
      point_emit_pf(P, ps, t, H, t0, [&](int, double &on0, double &on1, double &q0, double &q1) { on0 = pk[0]; on1 = pk[1]; q0 = pk[2]; q1 = pk[3]; },
                    (double *)r_);
      const bool corr = t < t0;
#pragma unroll
      for (int u = 0; u < 13; u++) w[u] = r_[u];
      w[13] = corr ? r_[13] : -0.0;
      w[14] = corr ? -0.0 : r_[13];
    }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    // the list's slots that hold terms of this lane's ROW (an OR around the row): list order is arrival order, so an entry's pool
    // slot is the row's count plus the row's entries in front of it
    unsigned rlo = (unsigned)mine, rhi = (unsigned)(mine >> 32); // (the two halves of the 64 slots, a DPP each)
    rlo |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rlo, 0x121, 0xf, 0xf, false);
    rhi |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rhi, 0x121, 0xf, 0xf, false);
    rlo |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rlo, 0x122, 0xf, 0xf, false);
    rhi |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rhi, 0x122, 0xf, 0xf, false);
    rlo |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rlo, 0x124, 0xf, 0xf, false);
    rhi |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rhi, 0x124, 0xf, 0xf, false);
    rlo |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rlo, 0x128, 0xf, 0xf, false);
    rhi |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)rhi, 0x128, 0xf, 0xf, false);
    const dmask_t rowm = ((dmask_t)rhi << 32) | rlo;
    for (dmask_t mm = mine; mm;) { // the owner adds its terms in list order: (point, term) order
      const int i = __builtin_ctzll(mm);
      mm &= mm - 1;
      ldscd_t w = dl.out + 15 * i;
      double r12[12];
#pragma unroll
      for (int u = 0; u < 12; u++) r12[u] = w[u];
      take(r12, w[12], w[13], w[14], rcnt + __builtin_popcountll(rowm & ((1ull << i) - 1ull)));
    }
    rcnt += __builtin_popcountll(rowm);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // the list is written again below
    listed = 0;
    mine = 0ull;
  };
  // (one more round than the pieces have points -- it only empties the list: the emission's code exists once)
#pragma unroll 1
  for (int j = 0; j <= L.Kmax + 1; j++) {
    const bool extra = j > L.Kmax; // (uniform)
    unsigned m = 0u;
    PtState pst;
    double nx[20];
    RectSet nr;
    if constexpr (RECT) {
      load_rect(rcor + (size_t)(j < L.Kmax ? j + 1 : L.Kmax) * 80, nr);
      rect_planes(rs, pl);
    } else {
      load_planes(cor + (size_t)(j < L.Kmax ? j + 1 : L.Kmax) * 16, cpitch, H, nx);
    }
    if (piece && j <= Kl && !extra)
      m = (unsigned)point_masks<false>(P, cc, l, N, j, Kl, step, s1, singul_, epis, H, pl, (gd_t) nullptr, D.sur, 0.0, 0.0, 0, 0.0, pst);
    const double s1_pt = s1;
    s1 += step; // the running sum of traj_optimizer.cpp:513
    [[maybe_unused]] long long emit_t0 = 0;
    if (D.prof != nullptr) { // (profiling only) trips of the loop below for the wave: the longest list of active terms among its 64 points;
      // DFTPAV_PROF_EMIT_CYCLES (a build flag): the cycles of that loop instead -- the clock behind it is read when the wave has reconverged
      // DFTPAV_PROF_FLUSH_CYCLES (a build flag): the cycles of the list's flushes alone, read where the flush is called
      // DFTPAV_PROF_CHAIN_CYCLES (a build flag): the cycles of the parked-term chains (pr.tick(2) to pr.tick(3)) of the evaluations
      // on the slow path alone, read in front of pr.tick(3); slot 3 less these is the other evaluations'
#if defined(DFTPAV_PROF_EMIT_CYCLES)
      emit_t0 = clock64();
#elif defined(DFTPAV_PROF_FLUSH_CYCLES) || defined(DFTPAV_PROF_CHAIN_CYCLES)
#else
      const int pc = __builtin_popcount(m);
      int trips = 0;
      while (__builtin_amdgcn_ballot_w64(pc > trips) != 0ull) trips++;
      pr.count(11, trips);
#endif
    }
    auto plane_of = [&](int k, double &on0, double &on1, double &q0, double &q1) { // the planes point_masks tested, still in registers
      on0 = pl[0]; on1 = pl[1]; q0 = pl[2]; q1 = pl[3];
#pragma unroll
      for (int u = 1; u < 5; u++) {
        on0 = k == u ? pl[4 * u] : on0;
        on1 = k == u ? pl[4 * u + 1] : on1;
        q0 = k == u ? pl[4 * u + 2] : q0;
        q1 = k == u ? pl[4 * u + 3] : q1;
      }
    };
    bool in_place = false;
    const int c = __builtin_popcount(m);
    const bool any = __builtin_amdgcn_ballot_w64(c != 0) != 0ull; // (uniform) some point of this round has active terms
    int incl = 0, total = 0, row_incl = 0;
    if (any) incl = scan_here(c, total, row_incl);
    // the list is emptied when this round's terms do not fit behind what it holds, and by the extra round
    if (listed > 0 && (extra || listed + total > kDense)) { // (uniform)
#ifdef DFTPAV_PROF_FLUSH_CYCLES
      const long long flush_t0 = D.prof != nullptr ? clock64() : 0;
#endif
      flush();
      if (D.prof != nullptr) { // (profiling only) flushes of the wave: the upper half of slot 9; the clock is read when the wave has reconverged
        pr.count(9, 1ll << 32);
#ifdef DFTPAV_PROF_FLUSH_CYCLES
        pr.count(11, clock64() - flush_t0);
#endif
      }
    }
    if (any && total > kDense) { // (uniform, rare) more than a list's worth in one round: in place, behind the earlier points' terms
      in_place = true;
    } else if (any) {
      int e = listed + incl - c;
      for (unsigned mm = m; mm;) {
        const int t = __builtin_ctz(mm);
        mm &= mm - 1;
        dl.id[e] = lane64 | (t << 6) | (j << 12);
        dl.s1[e] = s1_pt;
        if (t < t0) { // a corridor term: vertex v against half-plane k = t - v H
          int v = 0;
#pragma unroll
          for (int qv = 1; qv < 5; qv++) v += t >= qv * H ? 1 : 0;
          double on0, on1, q0, q1;
          plane_of(t - v * H, on0, on1, q0, q1);
          ldsd_t w = dl.out + 15 * e; // (where the term's result will go: the worker reads it first)
          w[0] = on0;
          w[1] = on1;
          w[2] = q0;
          w[3] = q1;
        }
        mine |= 1ull << e;
        e++;
      }
      listed += total;
    }
    if (in_place) { // (the list is empty here: the row's count is up to date)
      int slot = rcnt + row_incl - c;
      rcnt += __builtin_amdgcn_update_dpp(0, row_incl, 0x15F, 0xf, 0xf, false); // the row's terms of this round (lane 15's prefix)
      for (unsigned mm = m; mm;) {
        const int t = __builtin_ctz(mm);
        mm &= mm - 1;
        double r_[16];
        point_emit_pf(P, pst, t, H, t0, plane_of, (double *)r_);
        const bool corr = t < t0;
        double r12[12];
#pragma unroll
        for (int u = 0; u < 12; u++) r12[u] = r_[u];
        take(r12, r_[12], corr ? r_[13] : -0.0, corr ? -0.0 : r_[13], slot++);
      }
    }
#ifdef DFTPAV_PROF_EMIT_CYCLES
    if (D.prof != nullptr) pr.count(11, clock64() - emit_t0);
#endif
    if constexpr (RECT) {
      rs = nr;
    } else {
#pragma unroll
      for (int u = 0; u < 20; u++) pl[u] = nx[u];
    }
  }
  __threadfence_block(); // the parked terms are read by the other lanes of the row: the pool, and what went beyond it to global memory
  pr.tick(2);
  // ---- the per-segment chains: `gdT +=`, `energy +=` over the pieces in order from 0.0, then the parked terms in (piece, point,
  // term) order (every lane of the row forms them for itself: the same bits)
  double gdT = row_chain16(0.0, piece ? pG : -0.0);
  const double en = row_chain16(0.0, piece ? pE : -0.0);
  double cost0 = 0.0, cost2 = 0.0;
#ifdef DFTPAV_PROF_CHAIN_CYCLES
  bool chain_slow = false; // (uniform)
#endif
  // (round 6, measured and taken out: the first three terms of a piece kept in the lane's registers and chained by DPP when no piece of the
  // row has more -- on this workload a piece that has terms has more than three)
  {
    // a piece's start in (piece, point, term) order: the prefix sum of the counts along the row; lane 15's is the row's total
    const int pc = piece ? cnt : 0;
    int incl = pc;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false);
    const int total = __builtin_amdgcn_update_dpp(0, incl, 0x15F, 0xf, 0xf, false);
    pr.count(9, total);
    int kmax = 0; // (uniform) the largest total among the rows of the wave
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (row_here[r]) kmax = max(kmax, __builtin_amdgcn_readlane(incl, 16 * r + 15));
    // a row's terms are all in its pool unless it has more than the pool holds
    const bool slow = kmax > kQPool; // (uniform)
    if (D.prof != nullptr) pr.count(11, slow ? 1ll << 32 : 0ll); // (profiling only) evaluations on the slow path: the upper half of slot 11
#ifdef DFTPAV_PROF_CHAIN_CYCLES
    chain_slow = slow;
#endif
    if (kmax > 0 && !slow) {
      // the row's permutation: its pool slots in chain order (a lane's slots ascend in (point, term) order)
      {
        int at = incl - pc;
        for (unsigned long long mm = pmask; mm;) {
          q.perm[at++] = (unsigned char)__builtin_ctzll(mm);
          mm &= mm - 1;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      // eight terms at a time: their slots, then their 24 doubles with the reads in flight together, then the additions in order.
      // The four rows of the wave run in step; what lies beyond a row's total adds -0.0 (x + (-0.0) == x for every x)
      for (int k0 = 0; k0 < kmax; k0 += 8) {
        const unsigned long long pb = *(ldscu64_t)(q.perm + k0);
        double e[8][3];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int sl = k0 + u < total ? (int)((pb >> (8 * u)) & 255ull) : 0;
#pragma unroll
          for (int w = 0; w < 3; w++) e[u][w] = q.pool[sl * 3 + w];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const bool in = k0 + u < total;
          gdT += in ? e[u][0] : -0.0;
          cost0 += in ? e[u][1] : -0.0;
          cost2 += in ? e[u][2] : -0.0;
        }
      }
    } else if (slow) {
      // some row of the wave overflowed its pool.  Piece p's terms stand in the chain as its pool entries in slot order, then its
      // entries in global scratch in count order (they all arrived behind the pool's): positions start_p .. start_p + cnt_p - 1, the
      // first a_p = popcount(pmask_p) of them in the pool.  The sixteen lanes of a row fetch sixteen consecutive positions at once
      // and the row adds them in order by its DPP chain; the four rows run in step, as on the dense arm.
      // The table, as on the dense arm: a row's pool slots in piece order, a piece's slots ascending.  A piece's first entry is not
      // at its start in the chain here (pieces in front of it have entries in scratch) but at the count of the pool entries in
      // front of it; a row's pool holds kQPool entries at most, and so does its table.
      const int a = __builtin_popcountll(pmask);
      int pin = a;
      pin += __builtin_amdgcn_update_dpp(0, pin, 0x111, 0xf, 0xf, false);
      pin += __builtin_amdgcn_update_dpp(0, pin, 0x112, 0xf, 0xf, false);
      pin += __builtin_amdgcn_update_dpp(0, pin, 0x114, 0xf, 0xf, false);
      pin += __builtin_amdgcn_update_dpp(0, pin, 0x118, 0xf, 0xf, false);
      const int pstart = pin - a;
      {
        int at = pstart;
        for (unsigned long long mm = pmask; mm;) {
          q.perm[at++] = (unsigned char)__builtin_ctzll(mm);
          mm &= mm - 1;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      const int start = incl - pc;        // (a lane beyond the last piece: the row's total, which no position reaches)
      const int ap = a | (pstart << 8);   // (both kQPool at most)
      for (int k0 = 0; k0 < kmax; k0 += 16) {
        const int k = k0 + l; // this lane's position of the block
        // its piece: the last one that starts at or in front of k (a piece without terms starts where the next one does)
        const int p = row_count_le(start, k) - 1;
        const int src = (lane64 & 48) | p; // the lane of this row that owns piece p
        const int i = k - __shfl(start, src), apo = __shfl(ap, src);
        const bool in = k < total, pooled = in && i < (apo & 255);
        // the block's loads, all requested in front of its first addition; what lies beyond a row's total adds -0.0
        double e0 = -0.0, e1 = -0.0, e2 = -0.0;
        if (in && !pooled) {
          const int pp0 = p == 0 ? 0 : (L.Kd + 1) + (p - 1) * (L.K + 1);
          const gcd_t og = (gcd_t)(ovf + (size_t)pp0 * nterm * 3) + (size_t)i * 3;
          e0 = og[0];
          e1 = og[1];
          e2 = og[2];
        }
        // (every lane reads: one that has no pool entry reads the table's first byte and drops what it finds; & (kQPool - 1) keeps
        // a byte of a table that was not written inside the pool)
        ldscd_t pe = q.pool + ((int)q.perm[pooled ? (apo >> 8) + i : 0] & (kQPool - 1)) * 3;
        const double p0 = pe[0], p1 = pe[1], p2 = pe[2];
        e0 = pooled ? p0 : e0;
        e1 = pooled ? p1 : e1;
        e2 = pooled ? p2 : e2;
        row_chain16x3(gdT, cost0, cost2, e0, e1, e2);
      }
    }
  }
#ifdef DFTPAV_PROF_CHAIN_CYCLES
  if (D.prof != nullptr && chain_slow && pr.on) pr.count(11, clock64() - pr.last); // (pr.last: the clock of pr.tick(2))
#endif
  pr.tick(3);
  // ---- calGrads_PT (poly_traj_utils.hpp:1037-1066): adj = gdC * tInv, solveAdj, the duration gradient
  double pA;
  double tI[6];
#pragma unroll
  for (int u = 0; u < 6; u++) tI[u] = q.tw[u];
  {
    const double gdtInv[6] = {0.0, -1.0 * tI[2], -2.0 * tI[3], -3.0 * tI[4], -4.0 * tI[5], -5.0 * tI[5] * tI[1]};
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double gdcol = gdC[2 * k] * bq[2 * k] + gdC[2 * k + 1] * bq[2 * k + 1];
      acc += gdtInv[k] * gdcol;
    }
    pA = acc;
  }
  double adj[12];
#pragma unroll
  for (int u = 0; u < 12; u++) adj[u] = gdC[u] * tI[u >> 1];
  if (N == 16) { // (uniform)
    double X[6], Y[6];
    q4_split(adj, X, Y, l);
    sweep4_split<2>(tab + pk_sweep_offset(2, 16), X, Y, l);
    sweep4_split<3>(tab + pk_sweep_offset(3, 16), X, Y, l);
    q4_unsplit(X, Y, adj, l);
  } else {
    quad_sweep<2>(tab + pk_sweep_offset(2, N), adj, l, N, l < N, N);
    quad_sweep<3>(tab + pk_sweep_offset(3, N), adj, l, N, l < N, N);
  }
  pr.tick(4);
  // ---- gradient and cost (traj_optimizer.cpp:299-344)
  if (l < N - 1) { // gdP: rows 6 i + 5 of the adjoint
    q.gs[2 * l] = adj[10];
    q.gs[2 * l + 1] = adj[11];
  }
  {
    // the duration gradient (poly_traj_utils.hpp:1050-1064, VirtualTGradCost :405-419): the head terms live in lane 0, the tail
    // terms in lane N - 1 (every other lane hands the chain a -0.0)
    double hv[6], tv[6];
#pragma unroll
    for (int u = 0; u < 6; u++) {
      hv[u] = q.bnd[u];
      tv[u] = q.bnd[6 + u];
    }
    const double h1 = hv[2] * adj[2] + hv[3] * adj[3];
    const double h2 = (hv[4] * adj[4] + hv[5] * adj[5]) * 2.0 * t1;
    const double g1 = tv[2] * adj[8] + tv[3] * adj[9];
    const double g2 = (tv[4] * adj[10] + tv[5] * adj[11]) * 2.0 * t1;
    gdT = row_add_lane0(gdT, h1);
    gdT = row_add_lane0(gdT, h2);
    gdT = row_chain16(gdT, l == N - 1 ? g1 : -0.0);
    gdT = row_chain16(gdT, l == N - 1 ? g2 : -0.0);
    gdT = row_chain16(gdT, piece ? pA : -0.0);
    double gdVT2Rt;
    if (vt > 0) {
      gdVT2Rt = vt + 1.0;
    } else {
      const double denSqrt = (0.5 * vt - 1.0) * vt + 1.0;
      gdVT2Rt = (1.0 - vt) / (denSqrt * denSqrt);
    }
    if (l == 0) q.gs[L.x_tau0] = (gdT / N + P.wei_time) * gdVT2Rt;
  }
  double total_smcost = 0.0, total_timecost = 0.0, penalty_cost = 0.0;
  total_smcost += en;
  penalty_cost += (cost0 + 0.0) + cost2; // (the moving-obstacle cost of a segment without obstacles is its start value 0.0)
  total_timecost += Tr * P.wei_time;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // g is read by other lanes of the row
  pr.tick(5);
  return total_smcost + total_timecost + penalty_cost;
}

// ------------------------------------------------ L-BFGS, per row: the state machine is lbfgs_control.h's; the recursion is this file's

// The two-loop recursion (lbfgs.hpp:716-739) over `bound` stored pairs of this row's trajectory, the newest in slot ne - 1;
// d = -g on entry (elements from n on: 0.0).  The four rows run their steps in the same instructions; bound, the ring position
// and the division mode belong to the row.  History rows: (s, y) interleaved per element at pitch kQNpad; (ys, 1 / ys) per pair.
//
// What a step does besides its chain is kept short:
//   * a block of kQB pairs is kQB CONSECUTIVE rows from one address, the pairs at compile-time offsets.  A block that crosses the
//     end of the ring is read from the MIRROR (DevBatch::histM, 2 kQB rows per trajectory: the ring's rows m - kQB .. m - 1, then its
//     rows 0 .. kQB - 1), in which those rows are consecutive too; q4_store_pair writes a pair of either end to both places.  The
//     wrap is decided once per block.  The ring itself lies where the WAVE shape expects it (a hand-over resumes from it).
//   * n <= 31 (Y3 = false): element 31 of a row is no variable, and the pair's (ys, 1 / ys) sit there -- they arrive with lane 15's
//     second load and go to the row by DPP; histR is written as before (the WAVE shape reads it) but not read here.  n = 32 (Y3):
//     they are loaded from histR.
//   * alpha is kept by step number, not by ring slot: a compile-time offset from the block's first step.
//   * a row's bound falls inside at most one block per loop.  A block in which no row's bound falls (q4_blk_partial) runs its kQB steps
//     as one body under one mask, with no test between them: lane 0 of the row stores the block's alphas behind its last step in
//     16-byte writes (first loop), they are read at the block's head (second loop), and n > 16 is decided in front of the body.
//     Only a block with a bound inside it asks step by step.  Same products, same chains, same order in both forms.
constexpr int kQB = 8;     // stored pairs per register block (the next block is in flight while one is worked on)
constexpr int kQNpad = 64; // pitch of a history row: DevLayout::npad of every layout in scope (n <= 32; reference_order_quad_supported)
static_assert(kQuadMirrorRows == 2 * kQB, "DevBatch::histM holds kQB rows of either end of a ring");
static_assert((32 + 32 + 12 + 6 + sNUM) % 2 == 0 && kQB % 2 == 0, "a block's alphas start at a multiple of 16 bytes (q4_carve, q4_team_bytes)");
template <bool Y3> struct QBlk {
  d2_t a[kQB], b[kQB];    // (s, y) of elements l and 16 + l
  d2_t yr[Y3 ? kQB : 1];  // Y3: (ys, 1 / ys)
};
typedef double __attribute__((ext_vector_type(2))) qd2_t;

// 0.0 + p[0] + ... + p[n-1] in the recursion: row_sum32 without its selects.  The elements from n on of d are +-0.0 wherever this is
// called (quad_lbfgs.h: quad_state_io, quad_take and QuadRowVec set them to 0.0, and a step adds coefficient * 0.0 to them: the
// elements from n on of every stored s and y are +0.0 -- the buffers are cleared when they are allocated and no lane >= n stores),
// so their products are +-0.0 as long as the coefficients are finite.  The chain starts from +0.0, and a sum rounded to nearest is
// -0.0 only if both operands are: the accumulator is never -0.0, and adding +0.0 or -0.0 leaves it as it is -- what row_sum32's
// -0.0 does.  Y3 = false: lane 15's second element is (ys, 1 / ys), not zero -- the chain's last link, which would read it, is left
// out (n <= 31: it would add -0.0).
#define DFTPAV_FMAC_BCAST15 \
  DFTPAV_FMAC_BCAST(0) DFTPAV_FMAC_BCAST(1) DFTPAV_FMAC_BCAST(2) DFTPAV_FMAC_BCAST(3) DFTPAV_FMAC_BCAST(4) DFTPAV_FMAC_BCAST(5) DFTPAV_FMAC_BCAST(6) \
  DFTPAV_FMAC_BCAST(7) DFTPAV_FMAC_BCAST(8) DFTPAV_FMAC_BCAST(9) DFTPAV_FMAC_BCAST(10) DFTPAV_FMAC_BCAST(11) DFTPAV_FMAC_BCAST(12) \
  DFTPAV_FMAC_BCAST(13) DFTPAV_FMAC_BCAST(14)
__device__ __forceinline__ double row_chain15(double acc, double v) {
  const double one = 1.0;
  asm volatile("s_nop 1\n\t" DFTPAV_FMAC_BCAST15 : "+v"(acc) : "v"(v), "v"(one));
  return acc;
}
template <bool Y3> __device__ __forceinline__ double q4_rec_sum(double p0, double p1, bool wide) { // wide: n > 16
  // both products in front of the first chain: without this the compiler forms the second behind the first chain, in the step's
  // dependent path (in both block forms; where n <= 16 the product is formed and not used, one v_mul_f64 per step)
  asm volatile("" : "+v"(p1));
  double acc = row_chain16(0.0, p0);
  if (wide) acc = Y3 ? row_chain16(acc, p1) : row_chain15(acc, p1); // (uniform)
  return acc;
}

// the block of kQB pairs that starts in slot jl and walks downwards (DIR = -1) or upwards; jl: the next block's first slot.
// Unconditional loads from always-valid addresses (ring or mirror, both cleared at allocation); m >= kQB.
template <int DIR, bool Y3>
__device__ __forceinline__ void q4_load_blk(QBlk<Y3> &R, gcd2_t hS, gcd2_t hM, gcd2_t hR, int m, int l, int &jl) {
  // mirror row of ring row r: r - (m - kQB) for the last kQB rows, kQB + r for the first kQB
  const bool wrap = DIR < 0 ? jl < kQB - 1 : jl > m - kQB;
  const int mr = DIR < 0 ? kQB + jl : jl - (m - kQB);
  const gcd2_t row = (wrap ? hM + mr * kQNpad : hS + jl * kQNpad) + l;
#pragma unroll
  for (int u = 0; u < kQB; u++) {
    R.a[u] = row[DIR * u * kQNpad];
    R.b[u] = row[DIR * u * kQNpad + 16]; // (element 16 + l)
  }
  if (Y3) {
    int jr = jl;
#pragma unroll
    for (int u = 0; u < kQB; u++) {
      R.yr[Y3 ? u : 0] = hR[jr];
      if (DIR < 0) jr = jr == 0 ? m - 1 : jr - 1;
      else jr = jr == m - 1 ? 0 : jr + 1;
    }
  }
  if (DIR < 0) {
    jl -= kQB;
    jl = jl < 0 ? jl + m : jl;
  } else {
    jl += kQB;
    jl = jl >= m ? jl - m : jl;
  }
}
template <bool Y3> __device__ __forceinline__ void q4_pin_blk(QBlk<Y3> &R) {
#pragma unroll
  for (int u = 0; u < kQB; u++) {
    asm volatile("" : "+v"(R.a[u].x), "+v"(R.a[u].y), "+v"(R.b[u].x), "+v"(R.b[u].y));
    if (Y3) asm volatile("" : "+v"(R.yr[Y3 ? u : 0].x), "+v"(R.yr[Y3 ? u : 0].y));
  }
}
// (ys, 1 / ys) of pair u of a block: every lane of the row gets lane 15's second element (row_newbcast:15)
template <bool Y3> __device__ __forceinline__ d2_t q4_blk_yr(const QBlk<Y3> &R, int u) {
  if (Y3) return R.yr[Y3 ? u : 0];
  d2_t yr;
  yr.x = mov_dpp<0x15F>(R.b[u].x);
  yr.y = mov_dpp<0x15F>(R.b[u].y);
  return yr;
}
// One step of the first loop with pair u of a block; returns its alpha
template <bool EXACT, bool Y3>
__device__ __forceinline__ double q4_first_step(const QBlk<Y3> &R, int u, d2_t yr, bool wide, bool exact, double &d0, double &d1) {
  const double dot = q4_rec_sum<Y3>(R.a[u].x * d0, R.b[u].x * d1, wide);
  // lm_alpha[j] = lm_s.col(j).dot(d) / lm_ys[j]  (EXACT: some row of the wave divides -- only its lanes take the division's result)
  const double a = EXACT && exact ? dot / yr.x : div_by_rcp<false>(dot, yr.x, yr.y);
  const double na = -a;
  d0 = d0 + na * R.a[u].y; // d += (-alpha) * lm_y.col(j)
  d1 = d1 + na * R.b[u].y;
  return a;
}
// One step of the second loop with pair u of a block; av: the pair's alpha
template <bool EXACT, bool Y3>
__device__ __forceinline__ void q4_second_step(const QBlk<Y3> &R, int u, d2_t yr, double av, bool wide, bool exact, double &d0, double &d1) {
  const double dot = q4_rec_sum<Y3>(R.a[u].y * d0, R.b[u].y * d1, wide);
  const double beta = EXACT && exact ? dot / yr.x : div_by_rcp<false>(dot, yr.x, yr.y);
  const double cf = av - beta;
  d0 = d0 + cf * R.a[u].x; // d += (alpha - beta) * lm_s.col(j)
  d1 = d1 + cf * R.b[u].x;
}
// Does the bound of a row that is here fall INSIDE the block of steps i0 .. i0 + kQB - 1?  (uniform: rows that are not in the recursion,
// or have left its loop, have no lane in the ballot.)  Where it does not, a row takes all of the block's steps or none, and the block
// runs as one body under one mask; else every step asks for itself, as each of them did before.
__device__ __forceinline__ bool q4_blk_partial(int i0, int bound) {
  return __builtin_amdgcn_ballot_w64(i0 < bound && bound < i0 + kQB) != 0ull;
}
// The full-block bodies: all kQB steps of a block under the mask of the rows that take them, no test between the steps.
// wide: n > 16 (uniform), a constant where these are called.  al as in q4_first_steps / q4_second_steps.
template <bool EXACT, bool Y3>
__device__ __forceinline__ void q4_first_block(const QBlk<Y3> &R, ldsd_t al, bool wide, int l, bool exact, double &d0, double &d1) {
  double a[kQB];
#pragma unroll
  for (int u = 0; u < kQB; u++) a[u] = q4_first_step<EXACT>(R, u, q4_blk_yr<Y3>(R, u), wide, exact, d0, d1);
  // the block's alphas behind its last step, 16 bytes at a time (al is 16-byte aligned: q4_carve, i0 a multiple of kQB)
  if (l == 0) {
#pragma unroll
    for (int u = 0; u < kQB; u += 2) {
      qd2_t v;
      v.x = a[u];
      v.y = a[u + 1];
      *(__attribute__((address_space(3))) qd2_t *)(al + u) = v;
    }
  }
}
template <bool EXACT, bool Y3>
__device__ __forceinline__ void q4_second_block(const QBlk<Y3> &R, ldscd_t al, bool wide, bool exact, double &d0, double &d1) {
  double av[kQB]; // the block's alphas at its head (all kQB steps are taken: al .. al + kQB - 1 lie inside alpha)
#pragma unroll
  for (int u = 0; u < kQB; u++) av[u] = al[kQB - 1 - u];
#pragma unroll
  for (int u = 0; u < kQB; u++) q4_second_step<EXACT>(R, u, q4_blk_yr<Y3>(R, u), av[u], wide, exact, d0, d1);
}
// al: alpha of step i0 (first loop: step i of the recursion takes the i-th newest pair)
template <bool EXACT, bool Y3>
__device__ __forceinline__ void q4_first_steps(const QBlk<Y3> &R, ldsd_t al, int i0, int bound, int n, int l, bool exact, double &d0, double &d1) {
  if (!q4_blk_partial(i0, bound)) { // (uniform)
    if (i0 < bound) {               // (row-uniform) all kQB steps
      if (Y3 || n > 16) q4_first_block<EXACT>(R, al, true, l, exact, d0, d1); // (uniform)
      else q4_first_block<EXACT>(R, al, false, l, exact, d0, d1);
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < kQB; u++) {
    if (i0 + u < bound) { // (row-uniform)
      const double a = q4_first_step<EXACT>(R, u, q4_blk_yr<Y3>(R, u), n > 16, exact, d0, d1);
      if (l == 0) al[u] = a;
    }
  }
}
// al: alpha of the pair of this block's LAST step (the second loop takes the pairs in the opposite order: step u reads al[kQB - 1 - u])
template <bool EXACT, bool Y3>
__device__ __forceinline__ void q4_second_steps(const QBlk<Y3> &R, ldscd_t al, int i0, int bound, int n, int l, bool exact, double &d0, double &d1) {
  if (!q4_blk_partial(i0, bound)) { // (uniform)
    if (i0 < bound) {               // (row-uniform) all kQB steps
      if (Y3 || n > 16) q4_second_block<EXACT>(R, al, true, exact, d0, d1); // (uniform)
      else q4_second_block<EXACT>(R, al, false, exact, d0, d1);
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < kQB; u++) {
    if (i0 + u < bound) // (row-uniform)
      q4_second_step<EXACT>(R, u, q4_blk_yr<Y3>(R, u), al[kQB - 1 - u], n > 16, exact, d0, d1);
  }
}
// (the block loop of solver_ref.hip's two_loop / q4m_two_loop, except: alpha by step number, the second loop's first slot from ne - bound)
template <bool EXACT, bool Y3>
__device__ __forceinline__ void q4_two_loop(const Q4 &q, gcd2_t hS, gcd2_t hM, gcd2_t hR, int m, int n, int l, int bound, int ne, bool exact, double sc0, double &d0,
                                            double &d1) {
  QBlk<Y3> A, B;
  int jl = ne == 0 ? m - 1 : ne - 1;
  q4_load_blk<-1>(A, hS, hM, hR, m, l, jl);
#pragma unroll 1
  for (int i0 = 0; i0 < bound; i0 += 2 * kQB) {
    q4_pin_blk(A);
    q4_load_blk<-1>(B, hS, hM, hR, m, l, jl);
    q4_first_steps<EXACT>(A, q.alpha + i0, i0, bound, n, l, exact, d0, d1);
    q4_pin_blk(B);
    q4_load_blk<-1>(A, hS, hM, hR, m, l, jl);
    q4_first_steps<EXACT>(B, q.alpha + (i0 + kQB), i0 + kQB, bound, n, l, exact, d0, d1);
  }
  d0 = d0 * sc0;
  d1 = d1 * sc0;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // alpha written by lane 0 of the row, read by all below
  jl = ne - bound; // the oldest pair's slot
  jl = jl < 0 ? jl + m : jl;
  q4_load_blk<+1>(A, hS, hM, hR, m, l, jl);
#pragma unroll 1
  for (int i0 = 0; i0 < bound; i0 += 2 * kQB) {
    // (step i0 + u takes the pair of first-loop step bound - 1 - i0 - u; the pointer may lie in front of alpha where the steps that
    // would read there are masked)
    const ldscd_t al = (ldscd_t)(q.alpha + (bound - kQB - i0));
    q4_pin_blk(A);
    q4_load_blk<+1>(B, hS, hM, hR, m, l, jl);
    q4_second_steps<EXACT>(A, al, i0, bound, n, l, exact, d0, d1);
    q4_pin_blk(B);
    q4_load_blk<+1>(A, hS, hM, hR, m, l, jl);
    q4_second_steps<EXACT>(B, al - kQB, i0 + kQB, bound, n, l, exact, d0, d1);
  }
}
// One 16-byte unit of ring row `end` (element e: (s, y), or (ys, 1 / ys) in element 31), and of the mirror's copies of that row
__device__ __forceinline__ void q4_store_pair(gd_t hS, gd_t hM, int m, int end, int e, d2_t v) {
  ((gd2_t)hS)[(size_t)end * kQNpad + e] = v;
  if (end < kQB) ((gd2_t)hM)[(kQB + end) * kQNpad + e] = v;
  if (end >= m - kQB) ((gd2_t)hM)[(end - (m - kQB)) * kQNpad + e] = v;
}

// What quad_lbfgs.h's QuadRowVec needs to know of this kernel: a vector in two registers, the 32-step chain, a pair stored to
// the ring and to the mirror, the recursion above.  hS, hM, hR: the history of the row's trajectory.
struct Q4Shape {
  static constexpr int NV = 2;
  typedef Q4 Row;
  gd_t hS, hM, hR;
  __device__ __forceinline__ double row_sum(const double (&p)[2], int n, int l) const { return row_sum32(p[0], p[1], n, l); }
  __device__ __forceinline__ void store_pair(int m, int end, int e, d2_t sy) const { q4_store_pair(hS, hM, m, end, e, sy); }
  // histR as the WAVE shape reads it; n <= 31: (ys, 1 / ys) travel in the row too, as its element 31 (q4_two_loop)
  __device__ __forceinline__ void store_ys(int m, int end, int n, int l, d2_t yr) const {
    if (l == 0) ((gd2_t)hR)[end] = yr;
    if (l == 15 && n <= 31) q4_store_pair(hS, hM, m, end, 31, yr);
  }
  template <bool EXACT>
  __device__ __forceinline__ void two_loop(const Q4 &q, int m, int n, int l, int bound, int ne, bool exact, double sc0, double (&d)[2]) const {
    const gcd2_t cS = (gcd2_t)hS, cM = (gcd2_t)hM, cR = (gcd2_t)hR;
    if (n > 31) q4_two_loop<EXACT, true>(q, cS, cM, cR, m, n, l, bound, ne, exact, sc0, d[0], d[1]); // (uniform) element 31 is a variable
    else q4_two_loop<EXACT, false>(q, cS, cM, cR, m, n, l, bound, ne, exact, sc0, d[0], d[1]);
  }
};

// ------------------------------------------------ the kernel
// source, hand: quad_lbfgs.h (quad_take, quad_end_slice).  slice: evaluations of a wave after which its unfinished trajectories go
// back to the ring.
template <bool FAST, bool RECT>
__global__ void __launch_bounds__(256, DFTPAV_Q4_WAVES_PER_EU)
    ref4_kernel(const DevBatch *__restrict__ Dp, int mode, const double *__restrict__ tabs, const double *__restrict__ cor_t, double *__restrict__ scratch, int source,
                int slice, int hand) {
  extern __shared__ double lds_raw[];
  const DevBatch &D = *Dp;
  const DevLayout &L = D.L;
  const int tidb = threadIdx.x, Tb = blockDim.x, lane = tidb & 63, wv = tidb >> 6, W = Tb >> 6, row = lane >> 4, l = lane & 15;
  const int n = L.n, N = L.Ntot, H = L.H, mem = D.P.mem_size;
  Q4 q;
  q4_carve(q, reinterpret_cast<char *>(lds_raw) + q4_shared_bytes(N) + (size_t)(wv * 4 + row) * q4_team_bytes(mem), mem);
  DenseLds dl; // the wave's list of active terms (behind the rows of all waves)
  q4_carve_dense(dl, reinterpret_cast<char *>(lds_raw) + q4_shared_bytes(N) + (size_t)W * 4 * q4_team_bytes(mem) + (size_t)wv * q4_dense_bytes());
  const ldscd_t tab = (ldscd_t)lds_raw;
  for (int i = tidb; i < pk_segment_doubles(N); i += Tb) ((ldsd_t)lds_raw)[i] = tabs[i];
  __syncthreads(); // the only time the waves of the workgroup meet
  const bool ring = mode == kModeSolve && (source & 1) != 0;
  const bool force_exact_div = (source & 2) != 0;
  const int nterm = 5 * H + 4, JP = L.Kmax + 1;
  const size_t cpitch = (size_t)JP * 16;
  const size_t scratch_per_traj = (size_t)L.Npts * nterm * kRec + (size_t)L.Npts * nterm; // reference_order_scratch_per_traj, no obstacles
  Prof pr;
  pr.on = false;
  pr.acc = nullptr;
  pr.last = 0;
  QuadVec<2> v{};
  QuadRun r{-1, false, false, 0};
  int steps = 0;

  for (int pass = 0;; pass++) {
    if (!r.act && quad_take(D, q, v, r, mode, ring, force_exact_div, pass, pr)) {
      if (l < 12) q.bnd[l] = l < 6 ? D.iniS[(size_t)r.b * 6 + l] : D.finS[(size_t)r.b * 6 + (l - 6)];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    if (__builtin_amdgcn_ballot_w64(r.act) == 0ull) break; // (uniform) this wave has nothing left to do
    if (r.act) {
      const int b = r.b;
      // (RECT: the copy of 16-byte units [b][j][unit 5][piece 16], q4_corridor_rect_kernel)
      const gcd_t cor = RECT ? (gcd_t)(cor_t + ((size_t)b * JP * 80 + l) * 2) : (gcd_t)(cor_t + (size_t)b * L.H * 4 * cpitch + l);
      const gd_t ovf = (gd_t)(scratch + (size_t)b * scratch_per_traj);
      const double f = q4_eval<FAST, RECT>(D, q, dl, tab, cor, cpitch, ovf, l, pr);
      if (mode == kModeEval) {
        for (int h = 0; h < 2; h++) {
          const int e = 16 * h + l;
          if (e < n) D.g_out[(size_t)b * n + e] = q.gs[e];
        }
        if (l == 0) D.f_eval[b] = f;
        r.act = false;
      } else {
        const Q4Shape sh{(gd_t)(D.histS + (size_t)b * mem * kQNpad * 2), (gd_t)(D.histM + (size_t)b * kQuadMirrorRows * kQNpad * 2),
                         (gd_t)(D.histR + (size_t)b * mem * 2)};
        QuadRowVec<Q4Shape> rv(sh, q, v);
        lbfgs_advance(D, rv, f, l, pr);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (q.ist[iACTION] == kActDone) quad_results<2>(D, q, r, ring);
      }
    }
    if (!ring) {
      if (mode == kModeEval) break;
      continue;
    }
    steps++;
    if (slice > 0 && steps >= slice) { // (uniform)
      steps = 0;
      if (quad_end_slice(D, q, v, r, hand)) break;
    }
  }
}

// the corridor of a batch [B][4 H][NptsPad] -> [B][4 H][Kmax + 1][16]: element (j, p) = the value at constraint point j of piece p
// (0.0 where the piece has no such point), so that the 16 lanes of a row read a round's half-planes as 128 contiguous bytes
__global__ void q4_corridor_kernel(const double *__restrict__ cor, double *__restrict__ out, int B, int H4, int NptsPad, int N, int K, int Kd, int JP) {
  const size_t total = (size_t)B * H4 * JP * 16;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int p = (int)(i & 15);
    const size_t r = i >> 4;
    const int j = (int)(r % JP);
    const size_t bc = r / JP; // b * H4 + component
    double v = 0.0;
    if (p < N) {
      const int Kp = (p == 0 || p == N - 1) ? Kd : K;
      const int pt0 = p == 0 ? 0 : (Kd + 1) + (p - 1) * (K + 1);
      if (j <= Kp) v = cor[bc * NptsPad + pt0 + j];
    }
    out[i] = v;
  }
}

// Whether every corridor of a batch is a rectangle in the sense of RECT (q4_eval): H = 4 and, at every point, the four normals are
// (-S, C), (C, S), (S, -C), (-C, -S) with (C, S) the normal of plane 1 -- compared as 64-bit patterns, so a +0.0 where the relation
// wants -0.0 does not pass, and neither does a NaN.  cor: the solver's layout [B][16][NptsPad]; *flag (zero before the launch) is set
// to 1 by every point that does not satisfy the relations.
__global__ void q4_rect_check_kernel(const double *__restrict__ cor, int B, int Npts, int NptsPad, int *__restrict__ flag) {
  const size_t total = (size_t)B * Npts;
  const unsigned long long sign = 0x8000000000000000ull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / Npts;
    const int pt = (int)(i % Npts);
    const double *c = cor + b * 16 * NptsPad + pt;
    unsigned long long n[4][2];
    for (int k = 0; k < 4; k++)
      for (int q = 0; q < 2; q++) n[k][q] = (unsigned long long)__double_as_longlong(c[(size_t)(4 * k + q) * NptsPad]);
    const unsigned long long C = n[1][0], S = n[1][1];
    const bool nan = (C & ~sign) > 0x7ff0000000000000ull || (S & ~sign) > 0x7ff0000000000000ull;
    const bool ok = !nan && n[0][0] == (S ^ sign) && n[0][1] == C && n[2][0] == S && n[2][1] == (C ^ sign) && n[3][0] == (C ^ sign) && n[3][1] == (S ^ sign);
    if (!ok) *flag = 1;
  }
}

// the corridor of such a batch [B][16][NptsPad] -> 16-byte units [B][Kmax + 1][5][16]: unit 0 of (j, p) = (C, S), units 1-4 = (p_x, p_y)
// of planes 0-3 at constraint point j of piece p (zeros where the piece has no such point): the 16 lanes of a row read a unit as 256
// contiguous bytes, a round is 1280 bytes from one base.  10 / 16 of the size of q4_corridor_kernel's copy.
__global__ void q4_corridor_rect_kernel(const double *__restrict__ cor, d2_t *__restrict__ out, int B, int NptsPad, int N, int K, int Kd, int JP) {
  const size_t total = (size_t)B * JP * 80;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int p = (int)(i & 15);
    const int u = (int)((i >> 4) % 5);
    const size_t r = i / 80;
    const int j = (int)(r % JP);
    const size_t b = r / JP;
    d2_t v = {0.0, 0.0};
    if (p < N) {
      const int Kp = (p == 0 || p == N - 1) ? Kd : K;
      const int pt0 = p == 0 ? 0 : (Kd + 1) + (p - 1) * (K + 1);
      if (j <= Kp) {
        const int c0 = u == 0 ? 4 : 4 * (u - 1) + 2; // (C, S): the normal of plane 1; else the point of plane u - 1
        const double *src = cor + (b * 16 + c0) * NptsPad + pt0 + j;
        v.x = src[0];
        v.y = src[NptsPad];
      }
    }
    out[i] = v;
  }
}

} // namespace reford

// ---- host side
// what the layout must satisfy for the QUAD shape (header)
bool reference_order_quad_supported(const DevLayout &L, const DevParams &P, int S) {
  // (H <= 5: a point's 5 H + 4 <= 29 terms fit the 6-bit term field of the dense list's ids, quad_common.h)
  if (L.M != 1 || S != 0 || L.n > 32 || L.Ntot > 16 || L.Ntot < 2 || L.H < 1 || L.H > 5) return false;
  // (the recursion reads blocks of kQB consecutive history rows at pitch kQNpad, the ring's ends from a mirror of 2 kQB rows)
  if (L.npad != reford::kQNpad || P.mem_size < reford::kQB) return false;
  // (a workgroup of one wave must fit; the list's length kDense is what leaves room for FOUR of them at 16 pieces and a history of 256 --
  // quad_common.h: q4_dense_capacity, the same sum, asserted there)
  return reford::q4_shared_bytes(L.Ntot) + 4 * reford::q4_team_bytes(P.mem_size) + reford::q4_dense_bytes() <= 160 * 1024;
}
// Test hook: kDense, the entries of a wave's list of active terms (tests/test_gpu_quad_dense_list.py builds its cases round it)
extern "C" int dftpav_debug_quad_list_capacity(void) { return reford::kDense; }
size_t reference_order_quad_corridor_doubles(const DevLayout &L, int B) { return (size_t)B * L.H * 4 * (L.Kmax + 1) * 16; }
// the QUAD shape's LDS (a row: its part of a wave and a quarter of the wave's list of active terms), eight waves per CU at most
// (256 registers); a batch alone on the device hands its last 768 trajectories to the WAVE shape
QuadSizes reference_order_quad_sizes(const DevLayout &L, const DevParams &P) {
  return {reford::q4_shared_bytes(L.Ntot), reford::q4_team_bytes(P.mem_size) + (reford::q4_dense_bytes() + 3) / 4, reford::kQ4WavesPerCU, 768};
}
// rect: the copy of a batch of rectangles (q4_corridor_rect_kernel; it fits the same allocation)
hipError_t launch_quad_corridor(const DevBatch &D, double *cor_t, bool rect, hipStream_t stream) {
  const DevLayout &L = D.L;
  const size_t total = rect ? (size_t)D.B * (L.Kmax + 1) * 80 : reference_order_quad_corridor_doubles(L, D.B);
  const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
  if (rect)
    hipLaunchKernelGGL(reford::q4_corridor_rect_kernel, dim3(grid), dim3(256), 0, stream, D.corridor, reinterpret_cast<reford::d2_t *>(cor_t), D.B, D.NptsPad, L.Ntot, L.K,
                       L.Kd, L.Kmax + 1);
  else
    hipLaunchKernelGGL(reford::q4_corridor_kernel, dim3(grid), dim3(256), 0, stream, D.corridor, cor_t, D.B, L.H * 4, D.NptsPad, L.Ntot, L.K, L.Kd, L.Kmax + 1);
  return hipGetLastError();
}
// *d_flag = 1 if some corridor of the batch (H = 4, the solver's layout) is not a rectangle in the sense of RECT, else 0
hipError_t launch_quad_rect_check(const double *corridor, int B, int Npts, int NptsPad, int *d_flag, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(int), stream);
  if (e != hipSuccess) return e;
  const size_t total = (size_t)B * Npts;
  const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(reford::q4_rect_check_kernel, dim3(grid), dim3(256), 0, stream, corridor, B, Npts, NptsPad, d_flag);
  return hipGetLastError();
}
QuadKernel ref4_kernel_for(bool fast, bool rect) {
  if (fast && rect) return &reford::ref4_kernel<true, true>;
  return fast ? &reford::ref4_kernel<true, false> : &reford::ref4_kernel<false, false>;
}

} // namespace dftpav
