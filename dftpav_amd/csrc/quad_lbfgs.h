// quad_lbfgs.h -- what the two QUAD kernels of the reference order (solver_ref4.hip: ref4_kernel, one gear segment;
// solver_ref4m.hip: ref4m_kernel, several) do alike, stated once: the vector operations of a row of 16 lanes under the L-BFGS state
// machine every solve shape runs (lbfgs_control.h: lbfgs_advance; QuadRowVec below, the solver's vectors in registers), the record
// of a suspended trajectory, and the three pieces of the kernels' persistent loops that do not depend on the shape.
//
// A vector of n <= 16 NV variables is NV registers per lane: element 16 h + l is register h of lane l (elements from n on: 0.0).
// Every array below is indexed by fully unrolled loops only, so it lives in registers.
//
// What a kernel supplies is its SHAPE, a small object (solver_ref4.hip: Q4Shape, solver_ref4m.hip: Q4MShape<TAIL>):
//   NV                                          registers per vector (2 or 3)
//   Row                                         the LDS of a row; the state machine uses st [sNUM], ist [iNUM], its vectors xs, gs [16 NV]
//   row_sum(p, n, l)                            0.0 + p[0] + ... + p[n - 1], the sequential sum as the row's DPP chain
//   store_pair(m, end, e, sy)                   element e of the new pair (s, y) into ring row `end` of the history
//   store_ys(m, end, n, l, yr)                  the new pair's (ys, 1 / ys)
//   two_loop<EXACT>(q, m, n, l, bound, ne, exact, sc0, d)   the shape's own two-loop recursion (lbfgs.hpp:716-739)
// The recursions differ for measured reasons (blocks of 8 with a mirror of the ring's ends and (ys, 1 / ys) travelling in the row;
// blocks of 4 with the n == 33 tail load) and stay with their kernels, as do the evaluations.
#pragma once
#include "quad_common.h"
#include "lbfgs_control.h"

namespace dftpav {
namespace reford {

template <int NV> struct QuadVec { // the solver's vectors that live in registers
  double xp[NV], gp[NV], d[NV];
};
template <int NV> __device__ __forceinline__ void quad_read(ldscd_t a, int n, int l, double (&o)[NV]) {
#pragma unroll
  for (int h = 0; h < NV; h++) o[h] = 16 * h + l < n ? a[16 * h + l] : 0.0;
}
// max |a[i]| over a row's vector (order-free), the same value in every lane of the row
template <int NV> __device__ __forceinline__ double quad_absmax(const double (&a)[NV]) {
  double mx = fabs(a[0]);
#pragma unroll
  for (int h = 1; h < NV; h++) mx = fmax(mx, fabs(a[h]));
  return row_max16(mx);
}

// The QUAD policy of lbfgs_control.h's state machine: the vector operations of a row of 16 lanes over the kernel's shape object, with
// xp, gp, d in registers (v) and x, g in the row's LDS.  `lane` is the lane of the row, 0 .. 15.  The row chains run under the EXEC
// mask the control flow of lbfgs_advance leaves.
template <class Shape> struct QuadRowVec {
  static constexpr int NV = Shape::NV;
  const Shape &sh;
  const typename Shape::Row &q;
  QuadVec<NV> &v;
  ldsd_t st;
  ldsi_t ist;
  double x[NV], g[NV]; // the point the stop tests read, for the new pair
  __device__ __forceinline__ QuadRowVec(const Shape &sh_, const typename Shape::Row &q_, QuadVec<NV> &v_) : sh(sh_), q(q_), v(v_), st(q_.st), ist(q_.ist) {}
  __device__ __forceinline__ bool leader(int l) const { return l == 0; }
  __device__ __forceinline__ void first_direction(int n, int l, double &gmax, double &xmax, double &dd) {
    double sq[NV];
    quad_read(q.gs, n, l, g);
    quad_read(q.xs, n, l, x);
#pragma unroll
    for (int h = 0; h < NV; h++) {
      v.d[h] = 16 * h + l < n ? -g[h] : 0.0;
      sq[h] = (-g[h]) * (-g[h]);
    }
    gmax = quad_absmax(g), xmax = quad_absmax(x);
    dd = sh.row_sum(sq, n, l);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  __device__ __forceinline__ double save_point(int n, int l) {
    quad_read(q.xs, n, l, v.xp);
    quad_read(q.gs, n, l, v.gp);
    double gd[NV];
#pragma unroll
    for (int h = 0; h < NV; h++) gd[h] = v.gp[h] * v.d[h];
    return sh.row_sum(gd, n, l);
  }
  __device__ __forceinline__ void trial_point(int n, int l, double stp) {
#pragma unroll
    for (int h = 0; h < NV; h++)
      if (16 * h + l < n) q.xs[16 * h + l] = v.xp[h] + stp * v.d[h];
  }
  __device__ __forceinline__ double slope(int n, int l) {
    double gt[NV], gd[NV];
    quad_read(q.gs, n, l, gt);
#pragma unroll
    for (int h = 0; h < NV; h++) gd[h] = gt[h] * v.d[h];
    return sh.row_sum(gd, n, l);
  }
  __device__ __forceinline__ void revert(int n, int l) {
#pragma unroll
    for (int h = 0; h < NV; h++)
      if (16 * h + l < n) {
        q.xs[16 * h + l] = v.xp[h];
        q.gs[16 * h + l] = v.gp[h];
      }
  }
  __device__ __forceinline__ void absmax(int n, int l, double &gmax, double &xmax) {
    quad_read(q.xs, n, l, x);
    quad_read(q.gs, n, l, g);
    gmax = quad_absmax(g), xmax = quad_absmax(x);
  }
  // (s, y) interleaved per element; the four dot products of lbfgs.hpp:683-694
  __device__ __forceinline__ void new_pair(int m, int end, int n, int l, double &ys, double &yy, double &ss, double &gpgp) {
    double sv[NV], yv[NV], pys[NV], pyy[NV], pss[NV], pgg[NV];
#pragma unroll
    for (int h = 0; h < NV; h++) {
      const bool in = 16 * h + l < n;
      sv[h] = in ? x[h] - v.xp[h] : 0.0;
      yv[h] = in ? g[h] - v.gp[h] : 0.0;
      if (in) {
        d2_t sy;
        sy.x = sv[h];
        sy.y = yv[h];
        sh.store_pair(m, end, 16 * h + l, sy);
      }
      v.d[h] = in ? -g[h] : 0.0;
      pys[h] = yv[h] * sv[h];
      pyy[h] = yv[h] * yv[h];
      pss[h] = sv[h] * sv[h];
      pgg[h] = v.gp[h] * v.gp[h];
    }
    ys = sh.row_sum(pys, n, l);
    yy = sh.row_sum(pyy, n, l);
    ss = sh.row_sum(pss, n, l);
    gpgp = sh.row_sum(pgg, n, l);
    d2_t yr;
    yr.x = ys;
    yr.y = 1.0 / ys;
    sh.store_ys(m, end, n, l, yr); // (every lane of the row holds ys)
    if (l == 0 && !rcp_route_ok(ys)) ist[iSLOWDIV] = 1; // from here on the recursion divides (see div_by_rcp)
  }
  __device__ __forceinline__ void two_loop(int m, int n, int l, int bound, int ne, double sc0) {
    const bool exact = ist[iSLOWDIV] != 0;
    double d[NV];
#pragma unroll
    for (int h = 0; h < NV; h++) d[h] = v.d[h];
    // (the division mode is a wave-level choice of code: the reciprocal route has no branch in its steps)
    if (__builtin_amdgcn_ballot_w64(exact) != 0ull) sh.template two_loop<true>(q, m, n, l, bound, ne, exact, sc0, d);
    else sh.template two_loop<false>(q, m, n, l, bound, ne, exact, sc0, d);
#pragma unroll
    for (int h = 0; h < NV; h++) v.d[h] = 16 * h + l < n ? d[h] : 0.0;
  }
};

// solver state of a suspended trajectory <-> its record in DevBatch::state (the layout of solver_ref.hip's state_io: five vectors at
// pitch npad -- x, xp, g, gp, d --, the scalars, the integers; a hand-over to the WAVE shape resumes from it)
template <int NV, class Row>
__device__ inline void quad_state_io(const DevBatch &D, const Row &q, QuadVec<NV> &v, int b, int l, bool save) {
  const int n = D.L.n, npad = D.L.npad;
  double *rec = D.state + (size_t)b * D.state_stride;
#pragma unroll
  for (int h = 0; h < NV; h++) {
    const int e = 16 * h + l;
    if (e >= n) {
      if (!save) {
        q.xs[e] = 0.0;
        q.gs[e] = 0.0;
        v.xp[h] = v.gp[h] = v.d[h] = 0.0;
      }
      continue;
    }
    if (save) {
      rec[0 * npad + e] = q.xs[e];
      rec[1 * npad + e] = v.xp[h];
      rec[2 * npad + e] = q.gs[e];
      rec[3 * npad + e] = v.gp[h];
      rec[4 * npad + e] = v.d[h];
    } else {
      q.xs[e] = rec[0 * npad + e];
      v.xp[h] = rec[1 * npad + e];
      q.gs[e] = rec[2 * npad + e];
      v.gp[h] = rec[3 * npad + e];
      v.d[h] = rec[4 * npad + e];
    }
  }
  double *r2 = rec + 5 * npad;
  for (int w = l; w < sNUM; w += 16) {
    if (save) r2[w] = q.st[w];
    else q.st[w] = r2[w];
  }
  int *ri = reinterpret_cast<int *>(r2 + 24);
  for (int w = l; w < iNUM; w += 16) {
    if (save) ri[w] = q.ist[w];
    else q.ist[w] = ri[w];
  }
}

// ------------------------------------------------ the persistent loop of a QUAD kernel: what does not depend on the shape
// source bit 0 (ring): the rows pop trajectories from the batch's ring (solves; DevBatch::queue as solver_ref.hip uses it) --
// otherwise row r of wave w of workgroup i takes trajectory (i W + w) 4 + r; bit 1 (force_exact_div): test hook, true divisions in
// the recursion from the start.
struct QuadRun { // the trajectory a row serves
  int b;
  bool act, resumed;
  long long tick0;
};

// A row without a trajectory takes one: pops it from the ring (or takes its index in the first pass), resumes it from its record
// or starts it from x0 / x_in.  Returns whether the row has one now; its boundary states are the kernel's to load.
template <int NV, class Row>
__device__ __forceinline__ bool quad_take(const DevBatch &D, const Row &q, QuadVec<NV> &v, QuadRun &r, int mode, bool ring, bool force_exact_div, int pass,
                                          Prof &pr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6, row = lane >> 4, l = lane & 15;
  const int n = D.L.n;
  int id = -1;
  if (ring) {
    for (int k = 0; k < 4; k++) // one row after the other (the rows of a wave would otherwise race each other for the head)
      if (row == k && l == 0) id = ring_pop(D.qctl, D.queue, D.qcap);
    id = __shfl(id, lane & 48);
  } else if (pass == 0) {
    id = ((int)blockIdx.x * W + wv) * 4 + row;
    if (id >= D.B) id = -1;
  }
  if (id < 0) return false;
  r.b = id;
  r.act = true;
  r.resumed = ring && D.sflag[id] == 1;
  if (r.resumed) {
    quad_state_io(D, q, v, id, l, false);
  } else {
    const double *xsrc = (mode == kModeSolve) ? D.x0 : D.x_in;
#pragma unroll
    for (int h = 0; h < NV; h++) {
      const int e = 16 * h + l;
      q.xs[e] = e < n ? xsrc[(size_t)id * n + e] : 0.0;
      q.gs[e] = 0.0;
      v.xp[h] = v.gp[h] = v.d[h] = 0.0;
    }
    q.ist[l] = (l == iSLOWDIV && force_exact_div) ? 1 : 0; // (iNUM == 16 lanes)
  }
  r.tick0 = wall_clock64();
  pr.start(D.prof != nullptr && mode == kModeSolve && l == 0, D.prof + (size_t)id * 12, r.resumed);
  return true;
}

// The results of a finished trajectory (the epilogue of solver_ref.hip)
template <int NV, class Row> __device__ __forceinline__ void quad_results(const DevBatch &D, const Row &q, QuadRun &r, bool ring) {
  const int l = threadIdx.x & 15, n = D.L.n;
#pragma unroll
  for (int h = 0; h < NV; h++) {
    const int e = 16 * h + l;
    if (e < n) D.x_out[(size_t)r.b * n + e] = q.xs[e];
  }
  if (l == 0) write_results(D, r.b, q.st, q.ist, r.resumed, wall_clock64() - r.tick0, ring);
  r.act = false;
}

// End of a slice: the wave's unfinished trajectories go back to the ring (all four rows together, so that the rows of a wave are
// refilled together and the last trajectories of a batch gather in few waves).  Returns whether the wave LEAVES: once no more than
// `hand` trajectories of the batch are unfinished, the waves put theirs back and leave -- the host has a launch of the WAVE shape
// (solver_ref.hip: a wave per trajectory, 2-3 x faster per iteration on a device that is emptying) queued behind this one, which pops
// them from the same ring and resumes them from the same records.
template <int NV, class Row> __device__ __forceinline__ bool quad_end_slice(const DevBatch &D, const Row &q, QuadVec<NV> &v, QuadRun &r, int hand) {
  const int row = (threadIdx.x & 63) >> 4, l = threadIdx.x & 15;
  const bool leave = hand > 0 && __hip_atomic_load(&D.qctl[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (unsigned)hand;
  if (r.act) {
    quad_state_io(D, q, v, r.b, l, true);
    __threadfence(); // the record and the history rows of this slice are out before the id is handed on
    if (l == 0) {
      D.ticks[r.b] = (r.resumed ? D.ticks[r.b] : 0) + (wall_clock64() - r.tick0);
      D.sflag[r.b] = 1;
    }
  }
  for (int k = 0; k < 4; k++)
    if (r.act && row == k && l == 0) ring_push(D.qctl, D.queue, D.qcap, r.b);
  r.act = false;
  return leave;
}

} // namespace reford
} // namespace dftpav
