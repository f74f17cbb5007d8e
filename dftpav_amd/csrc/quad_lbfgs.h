// quad_lbfgs.h -- what the two QUAD kernels of the reference order (solver_ref4.hip: ref4_kernel, one gear segment;
// solver_ref4m.hip: ref4m_kernel, several) do alike, stated once: lbfgs_optimize / line_search_lewisoverton (lbfgs.hpp:276-390,
// 440-751) as a state machine per row of 16 lanes -- solver_ref.hip's lbfgs_advance with the solver's vectors in registers --, the
// record of a suspended trajectory, and the three pieces of the kernels' persistent loops that do not depend on the shape.
//
// A vector of n <= 16 NV variables is NV registers per lane: element 16 h + l is register h of lane l (elements from n on: 0.0).
// Every array below is indexed by fully unrolled loops only, so it lives in registers.
//
// What a kernel supplies is its SHAPE, a small object (solver_ref4.hip: Q4Shape, solver_ref4m.hip: Q4MShape<TAIL>):
//   NV                                          registers per vector (2 or 3)
//   Row                                         the LDS of a row; the state machine uses xs, gs [16 NV], st [sNUM], ist [iNUM]
//   row_sum(p, n, l)                            0.0 + p[0] + ... + p[n - 1], the sequential sum as the row's DPP chain
//   store_pair(m, end, e, sy)                   element e of the new pair (s, y) into ring row `end` of the history
//   store_ys(m, end, n, l, yr)                  the new pair's (ys, 1 / ys)
//   two_loop<EXACT>(q, m, n, l, bound, ne, exact, sc0, d)   the shape's own two-loop recursion (lbfgs.hpp:716-739)
// The recursions differ for measured reasons (blocks of 8 with a mirror of the ring's ends and (ys, 1 / ys) travelling in the row;
// blocks of 4 with the n == 33 tail load) and stay with their kernels, as do the evaluations.
#pragma once
#include "quad_common.h"

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

// Start of an outer iteration (lbfgs.hpp:559-574, 290-315): xp = x, gp = g, dginit = gp . d, first trial point
template <class Shape>
__device__ __forceinline__ bool quad_begin_iteration(const DevParams &P, const Shape &sh, const typename Shape::Row &q, QuadVec<Shape::NV> &v, int n, int l) {
  constexpr int NV = Shape::NV;
  quad_read(q.xs, n, l, v.xp);
  quad_read(q.gs, n, l, v.gp);
  double gd[NV];
#pragma unroll
  for (int h = 0; h < NV; h++) gd[h] = v.gp[h] * v.d[h];
  const double dginit = sh.row_sum(gd, n, l);
  const double step = q.st[sSTEP];
  if (!(step > 0.0)) {
    if (l == 0) q.ist[iRET] = -1006;
    return false;
  }
  if (0.0 < dginit) {
    if (l == 0) q.ist[iRET] = -1005;
    return false;
  }
  if (l == 0) {
    q.st[sFINIT] = q.st[sFX];
    q.st[sDGINIT] = dginit;
    q.st[sDGTEST] = P.f_dec_coeff * dginit;
    q.st[sDSTEST] = P.s_curv_coeff * dginit;
    q.st[sMU] = 0.0;
    q.st[sNU] = P.max_step;
    q.st[sSTP] = step;
    q.ist[iCOUNT] = 0;
    q.ist[iBRACKT] = 0;
    q.ist[iTOUCHED] = 0;
  }
#pragma unroll
  for (int h = 0; h < NV; h++)
    if (16 * h + l < n) q.xs[16 * h + l] = v.xp[h] + step * v.d[h];
  return true;
}

// Everything lbfgs_optimize does between two evaluations (lbfgs.hpp:524-745 with the line search of :312-389 unrolled into it):
// solver_ref.hip's lbfgs_advance for the trajectory of this row; f: the cost of the evaluation just made; sets iACTION.
// The row chains run under the EXEC mask this control flow leaves: the fences, the early returns and the ticks are where they are
// for that.
template <class Shape>
__device__ __forceinline__ void quad_advance(const DevBatch &D, const Shape &sh, const typename Shape::Row &q, QuadVec<Shape::NV> &v, double f, int l, Prof &pr) {
  constexpr int NV = Shape::NV;
  const DevParams &P = D.P;
  const int n = D.L.n, m = P.mem_size;
  int action = kActEval;
  if (q.ist[iPHASE] == 0) { // after the first evaluation: lbfgs.hpp:524-551
    double g[NV], x[NV], sq[NV];
    quad_read(q.gs, n, l, g);
    quad_read(q.xs, n, l, x);
#pragma unroll
    for (int h = 0; h < NV; h++) {
      v.d[h] = 16 * h + l < n ? -g[h] : 0.0;
      sq[h] = (-g[h]) * (-g[h]);
    }
    const double gmax = quad_absmax(g), xmax = quad_absmax(x);
    const double dd = sh.row_sum(sq, n, l);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (l == 0) {
      q.st[sFX] = f;
      q.st[sPF0] = f;
      q.ist[iEVALS] = 1;
      q.ist[iEND] = 0;
      q.ist[iBOUND] = 0;
      q.ist[iHISTLO] = 0;
      q.ist[iHISTHI] = 0;
      q.ist[iPHASE] = 1;
    }
    if (gmax / fmax(1.0, xmax) < P.g_epsilon) {
      if (l == 0) {
        q.ist[iRET] = 0;
        q.ist[iK] = 0;
      }
      action = kActDone;
    } else {
      if (l == 0) {
        q.st[sSTEP] = 1.0 / sqrt(dd);
        q.ist[iK] = 1;
      }
      __threadfence_block();
      if (!quad_begin_iteration(P, sh, q, v, n, l)) action = kActDone;
    }
    if (l == 0) q.ist[iACTION] = action;
    return;
  }

  // ---- after a line-search trial: lbfgs.hpp:317-389
  const double fx = f;
  const double finit = q.st[sFINIT];
  double stp = q.st[sSTP];
  const int count = q.ist[iCOUNT] + 1;
  int ls = 0;
  bool decided = false;
  const int evals_before = q.ist[iEVALS];
  __threadfence_block();
  if (l == 0) {
    q.st[sFX] = fx;
    q.ist[iEVALS] = evals_before + 1;
    q.ist[iCOUNT] = count;
  }
  if (isinf(fx) || isnan(fx)) {
    ls = -1012;
    decided = true;
  } else if (P.past > 0 && fabs(finit - fx) / (fabs(finit) + 1.0) < P.delta / P.past) { // lbfgs.hpp:326-329
    ls = count;
    decided = true;
  } else {
    double mu = q.st[sMU], nu = q.st[sNU];
    bool brackt = q.ist[iBRACKT] != 0;
    const int touched = q.ist[iTOUCHED];
    if (fx > finit + stp * q.st[sDGTEST]) {
      nu = stp;
      brackt = true;
    } else {
      double g[NV], gd[NV];
      quad_read(q.gs, n, l, g);
#pragma unroll
      for (int h = 0; h < NV; h++) gd[h] = g[h] * v.d[h];
      const double gs = sh.row_sum(gd, n, l);
      if (gs < q.st[sDSTEST]) {
        mu = stp;
      } else {
        ls = count;
        decided = true;
      }
    }
    bool touch_now = false;
    if (!decided) {
      if (P.max_linesearch <= count) {
        ls = -1009;
        decided = true;
      } else if (brackt && (nu - mu) < P.machine_prec * nu) {
        ls = -1007;
        decided = true;
      } else {
        if (brackt) stp = 0.5 * (mu + nu);
        else stp *= 2.0;
        if (stp < P.min_step) {
          ls = -1011;
          decided = true;
        } else if (stp > P.max_step) {
          if (touched) {
            ls = -1010;
            decided = true;
          } else {
            touch_now = true;
            stp = P.max_step;
          }
        }
      }
    }
    __threadfence_block();
    if (l == 0) {
      q.st[sMU] = mu;
      q.st[sNU] = nu;
      q.ist[iBRACKT] = brackt ? 1 : 0;
      q.st[sSTP] = stp;
      if (touch_now) q.ist[iTOUCHED] = 1;
    }
    if (!decided) {
#pragma unroll
      for (int h = 0; h < NV; h++)
        if (16 * h + l < n) q.xs[16 * h + l] = v.xp[h] + stp * v.d[h];
      if (l == 0) q.ist[iACTION] = kActEval;
      pr.tick(6);
      return;
    }
  }
  if (l == 0) q.st[sSTEP] = stp; // lbfgs.hpp:574 passes `step` by reference
  if (ls < 0) { // lbfgs.hpp:604-611: x, g reverted; fx is not
#pragma unroll
    for (int h = 0; h < NV; h++)
      if (16 * h + l < n) {
        q.xs[16 * h + l] = v.xp[h];
        q.gs[16 * h + l] = v.gp[h];
      }
    if (l == 0) {
      q.ist[iRET] = ls;
      q.ist[iACTION] = kActDone;
    }
    return;
  }

  // ---- convergence / stopping tests (lbfgs.hpp:628-666)
  double x[NV], g[NV];
  quad_read(q.xs, n, l, x);
  quad_read(q.gs, n, l, g);
  int k = q.ist[iK];
  {
    const double gmax = quad_absmax(g), xmax = quad_absmax(x);
    const int kGoOn = 12345;
    int ret = kGoOn;
    if (gmax / fmax(1.0, xmax) < P.g_epsilon) {
      ret = 0;
    } else {
      if (0 < P.past) {
        const int slot = k % P.past;
        const double pf = q.st[sPF0 + slot];
        __threadfence_block();
        if (P.past <= k) {
          const double rate = fabs(pf - fx) / fmax(1.0, fabs(fx));
          if (rate < P.delta) ret = 1;
        }
        if (ret == kGoOn && l == 0) q.st[sPF0 + slot] = fx;
      }
      if (ret == kGoOn && P.max_iterations != 0 && P.max_iterations <= k) ret = -1008;
    }
    if (ret != kGoOn) {
      if (l == 0) {
        q.ist[iRET] = ret;
        q.ist[iACTION] = kActDone;
      }
      return;
    }
  }
  ++k;
  pr.tick(6);
  const int end = q.ist[iEND];
  int bound = q.ist[iBOUND];
  __threadfence_block();
  if (l == 0) q.ist[iK] = k;

  // ---- history update + two-loop recursion (lbfgs.hpp:676-740); (s, y) interleaved per element
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
  // the four dot products of lbfgs.hpp:683-694
  const double ys = sh.row_sum(pys, n, l);
  const double yy = sh.row_sum(pyy, n, l);
  const double ss = sh.row_sum(pss, n, l);
  const double gpgp = sh.row_sum(pgg, n, l);
  {
    d2_t yr;
    yr.x = ys;
    yr.y = 1.0 / ys;
    sh.store_ys(m, end, n, l, yr); // (every lane of the row holds ys)
  }
  if (l == 0 && !rcp_route_ok(ys)) q.ist[iSLOWDIV] = 1; // from here on the recursion divides (see div_by_rcp)
  const double cau = ss * sqrt(gpgp) * P.cautious_factor;
  pr.tick(7);
  if (ys > cau) {
    ++bound;
    bound = m < bound ? m : bound;
    const int ne = end + 1 == m ? 0 : end + 1;
    __threadfence_block(); // the newest pair's row and (ys, 1 / ys) are read back below
    const bool exact = q.ist[iSLOWDIV] != 0;
    double d[NV];
#pragma unroll
    for (int h = 0; h < NV; h++) d[h] = v.d[h];
    // (the division mode is a wave-level choice of code: the reciprocal route has no branch in its steps)
    if (__builtin_amdgcn_ballot_w64(exact) != 0ull) sh.template two_loop<true>(q, m, n, l, bound, ne, exact, ys / yy, d);
    else sh.template two_loop<false>(q, m, n, l, bound, ne, exact, ys / yy, d);
#pragma unroll
    for (int h = 0; h < NV; h++) v.d[h] = 16 * h + l < n ? d[h] : 0.0;
    if (l == 0) {
      q.ist[iEND] = ne;
      q.ist[iBOUND] = bound;
      long long hs = ((long long)q.ist[iHISTHI] << 32) | (unsigned int)q.ist[iHISTLO];
      hs += bound;
      q.ist[iHISTLO] = (int)(hs & 0xffffffffLL);
      q.ist[iHISTHI] = (int)(hs >> 32);
    }
  }
  if (l == 0) q.st[sSTEP] = 1.0; // lbfgs.hpp:743
  pr.tick(8);
  __threadfence_block();
  const bool ok = quad_begin_iteration(P, sh, q, v, n, l);
  if (l == 0) q.ist[iACTION] = ok ? kActEval : kActDone;
  pr.tick(6);
}

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
