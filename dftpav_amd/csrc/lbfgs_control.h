// lbfgs_control.h -- the L-BFGS control of the reference order, stated once for every solve shape: what lbfgs_optimize does between
// two evaluations (lbfgs.hpp:524-745, with line_search_lewisoverton of :276-390 unrolled into it) as a state machine over the scalars
// st [sNUM] / ist [iNUM] of one trajectory.  Everything that DECIDES is here -- the first-evaluation block, the line search's tests
// and step update, the negative exits, the revert, the stop tests, the cautious update, the ring bookkeeping, the hist_sum carry --
// and so is every access to st / ist, every fence, every tick and every early return, in one order for all shapes (a QUAD kernel's
// row chains run under the EXEC mask this control flow leaves).
//
// How a VECTOR operation is carried out is the shape's, a policy V (solver_ref.hip: LaneVec<CAP>, one variable per lane and a DPP
// chain; StridedVec, a strided loop and a chain read back from LDS; quad_lbfgs.h: QuadRowVec<Shape>, NV registers per lane and a
// row chain):
//   st, ist                                     the trajectory's scalars (LDS)
//   leader(lane)                                the one lane that writes them
//   first_direction(n, lane, gmax, xmax, dd)    d = -g; max |g|, max |x|, dd = d . d                           (lbfgs.hpp:524-551)
//   save_point(n, lane)                         xp = x, gp = g; returns dginit = gp . d                         (:559-574, 290-315)
//   trial_point(n, lane, stp)                   x = xp + stp d
//   slope(n, lane)                              g . d
//   revert(n, lane)                             x = xp, g = gp                                                  (:604-611)
//   absmax(n, lane, gmax, xmax)                 max |g|, max |x|                                                (:628-632)
//   new_pair(m, end, n, lane, ys, yy, ss, gpgp) s = x - xp, y = g - gp into ring row `end` with (ys, 1 / ys), d = -g, the four dot
//                                               products; notes a ys that rules out the reciprocal route        (:676-694)
//   two_loop(m, n, lane, bound, ne, sc0)        d through the two-loop recursion, H0 = sc0                      (:716-739)
// Every sum is the sequential one, 0.0 + p[0] + p[1] + ..., and every lane that takes part ends with the same bits.
#pragma once
#include "ref_order_common.h"

namespace dftpav {
namespace reford {

// Start of an outer iteration (lbfgs.hpp:559-574, 290-315): xp = x, gp = g, dginit = gp . d, first trial point
template <class V> __device__ __forceinline__ bool lbfgs_begin_iteration(const DevParams &P, V &v, int n, int lane) {
  const double dginit = v.save_point(n, lane);
  const double step = v.st[sSTEP];
  if (!(step > 0.0)) {
    if (v.leader(lane)) v.ist[iRET] = -1006;
    return false;
  }
  if (0.0 < dginit) {
    if (v.leader(lane)) v.ist[iRET] = -1005;
    return false;
  }
  if (v.leader(lane)) {
    v.st[sFINIT] = v.st[sFX];
    v.st[sDGINIT] = dginit;
    v.st[sDGTEST] = P.f_dec_coeff * dginit;
    v.st[sDSTEST] = P.s_curv_coeff * dginit;
    v.st[sMU] = 0.0;
    v.st[sNU] = P.max_step;
    v.st[sSTP] = step;
    v.ist[iCOUNT] = 0;
    v.ist[iBRACKT] = 0;
    v.ist[iTOUCHED] = 0;
  }
  v.trial_point(n, lane, step);
  return true;
}

// Everything lbfgs_optimize does between two evaluations; f: the cost of the evaluation just made; sets iACTION.
template <class V> __device__ __forceinline__ void lbfgs_advance(const DevBatch &D, V &v, double f, int lane, Prof &pr) {
  const DevParams &P = D.P;
  const int n = D.L.n, m = P.mem_size;
  const bool lead = v.leader(lane);
  int action = kActEval;
  if (v.ist[iPHASE] == 0) { // after the first evaluation: lbfgs.hpp:524-551
    double gmax, xmax, dd;
    v.first_direction(n, lane, gmax, xmax, dd);
    if (lead) {
      v.st[sFX] = f;
      v.st[sPF0] = f;
      v.ist[iEVALS] = 1;
      v.ist[iEND] = 0;
      v.ist[iBOUND] = 0;
      v.ist[iHISTLO] = 0;
      v.ist[iHISTHI] = 0;
      v.ist[iPHASE] = 1;
    }
    if (gmax / fmax(1.0, xmax) < P.g_epsilon) {
      if (lead) {
        v.ist[iRET] = 0;
        v.ist[iK] = 0;
      }
      action = kActDone;
    } else {
      if (lead) {
        v.st[sSTEP] = 1.0 / sqrt(dd);
        v.ist[iK] = 1;
      }
      __threadfence_block();
      if (!lbfgs_begin_iteration(P, v, n, lane)) action = kActDone;
    }
    if (lead) v.ist[iACTION] = action;
    return;
  }

  // ---- after a line-search trial: lbfgs.hpp:317-389
  const double fx = f;
  const double finit = v.st[sFINIT];
  double stp = v.st[sSTP];
  const int count = v.ist[iCOUNT] + 1;
  int ls = 0;
  bool decided = false;
  const int evals_before = v.ist[iEVALS];
  __threadfence_block();
  if (lead) {
    v.st[sFX] = fx;
    v.ist[iEVALS] = evals_before + 1;
    v.ist[iCOUNT] = count;
  }
  if (isinf(fx) || isnan(fx)) {
    ls = -1012;
    decided = true;
  } else if (P.past > 0 && fabs(finit - fx) / (fabs(finit) + 1.0) < P.delta / P.past) { // lbfgs.hpp:326-329
    ls = count;
    decided = true;
  } else {
    double mu = v.st[sMU], nu = v.st[sNU];
    bool brackt = v.ist[iBRACKT] != 0;
    const int touched = v.ist[iTOUCHED];
    if (fx > finit + stp * v.st[sDGTEST]) {
      nu = stp;
      brackt = true;
    } else {
      const double gs = v.slope(n, lane);
      if (gs < v.st[sDSTEST]) {
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
    if (lead) {
      v.st[sMU] = mu;
      v.st[sNU] = nu;
      v.ist[iBRACKT] = brackt ? 1 : 0;
      v.st[sSTP] = stp;
      if (touch_now) v.ist[iTOUCHED] = 1;
    }
    if (!decided) {
      v.trial_point(n, lane, stp);
      if (lead) v.ist[iACTION] = kActEval;
      pr.tick(6);
      return;
    }
  }
  if (lead) v.st[sSTEP] = stp; // lbfgs.hpp:574 passes `step` by reference
  if (ls < 0) { // lbfgs.hpp:604-611: x, g reverted; fx is not
    v.revert(n, lane);
    if (lead) {
      v.ist[iRET] = ls;
      v.ist[iACTION] = kActDone;
    }
    return;
  }

  // ---- convergence / stopping tests (lbfgs.hpp:628-666)
  double gmax, xmax;
  v.absmax(n, lane, gmax, xmax);
  int k = v.ist[iK];
  {
    const int kGoOn = 12345;
    int ret = kGoOn;
    if (gmax / fmax(1.0, xmax) < P.g_epsilon) {
      ret = 0;
    } else {
      if (0 < P.past) {
        const int slot = k % P.past;
        const double pf = v.st[sPF0 + slot];
        __threadfence_block();
        if (P.past <= k) {
          const double rate = fabs(pf - fx) / fmax(1.0, fabs(fx));
          if (rate < P.delta) ret = 1;
        }
        if (ret == kGoOn && lead) v.st[sPF0 + slot] = fx;
      }
      if (ret == kGoOn && P.max_iterations != 0 && P.max_iterations <= k) ret = -1008;
    }
    if (ret != kGoOn) {
      if (lead) {
        v.ist[iRET] = ret;
        v.ist[iACTION] = kActDone;
      }
      return;
    }
  }
  ++k;
  pr.tick(6);
  const int end = v.ist[iEND];
  int bound = v.ist[iBOUND];
  __threadfence_block();
  if (lead) v.ist[iK] = k;

  // ---- history update + two-loop recursion (lbfgs.hpp:676-740)
  double ys, yy, ss, gpgp;
  v.new_pair(m, end, n, lane, ys, yy, ss, gpgp);
  const double cau = ss * sqrt(gpgp) * P.cautious_factor;
  pr.tick(7);
  if (ys > cau) {
    ++bound;
    bound = m < bound ? m : bound;
    const int ne = end + 1 == m ? 0 : end + 1;
    __threadfence_block(); // the newest pair's row and (ys, 1 / ys) are read back by the recursion
    v.two_loop(m, n, lane, bound, ne, ys / yy);
    if (lead) {
      v.ist[iEND] = ne;
      v.ist[iBOUND] = bound;
      long long hs = ((long long)v.ist[iHISTHI] << 32) | (unsigned int)v.ist[iHISTLO];
      hs += bound;
      v.ist[iHISTLO] = (int)(hs & 0xffffffffLL);
      v.ist[iHISTHI] = (int)(hs >> 32);
    }
  }
  if (lead) v.st[sSTEP] = 1.0; // lbfgs.hpp:743
  pr.tick(8);
  __threadfence_block();
  const bool ok = lbfgs_begin_iteration(P, v, n, lane);
  if (lead) v.ist[iACTION] = ok ? kActEval : kActDone;
  pr.tick(6);
}

} // namespace reford
} // namespace dftpav
