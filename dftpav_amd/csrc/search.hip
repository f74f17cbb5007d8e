// Hybrid A* front-end search on the device: the step that turns a start pose and a goal into the searched path.
//
//   KinoAstar::search                              traj_planner/src/kino_astar.cpp:37-301
//   KinoAstar::stateTransit                        kino_astar.cpp:21-36
//   KinoAstar::is_shot_sucess / computeShotTraj    kino_astar.cpp:304-345 (ReedsSheppStateSpace: rs_math.h)
//   KinoAstar::retrievePath                        kino_astar.cpp:351-363
//   KinoAstar::getKinoNode, up to SampleTraj       kino_astar.cpp:554-612
//   KinoAstar::posToIndex / yawToIndex, getHeu     kino_astar.cpp:804-816, kino_astar.h:221-226
//   NodeHashTable, the open set (priority_queue)   kino_astar.h:67-126, 136 (kino_heap.h)
//   TrajPlanner::getKinoPath (3D, then 2D retry)   traj_manager.cpp:69-117
//   CheckCollisionUsingPosAndYaw                   semantic_map_manager.cc:639-662, shapes.cc:110-149 (as validate.hip)
//
// One workgroup of 256 threads per query, looping until the query ends.  What is parallel: the Reeds-Shepp shot (every lane
// solves the word; the sample offsets l = 0, checkl, checkl + checkl, ... are the reference's running sum, tabulated on the
// host) with one lane per sample walking the vehicle outline, OR-reduced; and, per expansion, the n_inputs x check_num
// intermediate poses with their outline walks, reduced to one collision flag per input, together with each input's
// propagated state, grid indices and heuristic.  What is serial, on lane 0 and in input order: the hash find, the closed and
// same-voxel tests, the cost, and the create / push or in-place update -- a later input sees what an earlier one inserted.
// The node pool, an open-addressing hash table of node indices and the heap live in an HBM workspace the handle owns.
//
// Documented deviation: the reference's wall-clock budget max_seach_time (1.0 s) is a deterministic iteration budget
// max_iters here; when iter_num_ reaches it at the budget check the reference's time-out branch is taken (:115-132).
// fp64, no contraction, correctly rounded tan / sin / cos (cr_trig.h): bit-identical to oracle_search/ in order 2.
//
// The heuristic.  getHeu (kino_astar.h:221-226) is tie_breaker * |p - goal|.  The kernel is a template on FIELD: without a field
// (the default) it is the code above and nothing else; with the goal field F_q of the query's goal (goalfield.hip,
// dftpav_set_search_heuristic) both places that form a heuristic -- the start node and every input -- take
//   lambda_heu * fmax(tie_breaker * |p - goal|, (double)F_q[cell of p] * unit),
// the term of kino_astar.cpp:247's commented-out line as a maximum with getHeu; the cell by grid_occupied's rounding, 0 for a point
// outside the grid or an unreached cell.  The 3D search and its 2D retry read the same field.
//
// The second template flag, TABLE, adds the non-holonomic, obstacle-free term (dftpav_set_search_rs_heuristic): the Reeds-Shepp
// cost-to-go table T of rstable.hip, read at the nearest cell of the state in the goal's frame.  Per query, once: c = cos(goal
// yaw), s = sin(goal yaw), correctly rounded.  For a state (x, y, yaw): lx = c (x - gx) + s (y - gy), ly = c (y - gy) - s (x - gx),
// fi = round(lx / cell) + half, fj = round(ly / cell) + half as doubles; outside [0, n) in either (or NaN) the term is 0; the yaw
// slice is k = (int)round((yaw - goal yaw) / dth) reduced into [0, n_yaw) by integer remainder; the term is scale * T[k][fj][fi].
// The heuristic is then lambda_heu * fmax(fmax(tie_breaker * |p - goal|, the field's term where there is one), the table's term).
// search_kernel<false, false> and <true, false> are the kernels of before; launch_search picks the instance.
//
// FIELD has a third value, kFieldWindow (dftpav_set_search_heuristic_window, docs/NEXT_ROWS.md §4.22): the query's field covers a
// window (X0, Y0, WX, WY) of the grid only and is stored [WY][WX].  The cell (cx, cy) is rounded as above; outside the window the
// term is 0, as outside the grid; inside it the value is read at (cx - X0) + WX * (cy - Y0).  Nothing else differs, the maximum
// with the table's term included.  The instances with FIELD = kFieldNone and kFieldMap are the four of before, their code unchanged.
#include <hip/hip_runtime.h>

#include "../../include/dftpav_hip.h"
#include "device_types.h"
#include "kino_heap.h"
#include "rs_math.h"
#include "search_args.h"

namespace dftpav {

constexpr char kInClose = 'a', kInOpen = 'b'; // kino_astar.h:36-38
constexpr int kReachEnd = 2, kNoPath = 3;

// stateTransit, kino_astar.cpp:21-36 (psi != 0 takes the curved branch, however small psi is)
__device__ inline void sr_transit(const SearchArgs &A, double x0, double y0, double yaw0, double psi, double s, double *o) {
  if (psi != 0) {
    const double k = A.sp.wheel_base / crt::tan(psi);
    o[0] = x0 + k * (crt::sin(yaw0 + s / k) - crt::sin(yaw0));
    o[1] = y0 - k * (crt::cos(yaw0 + s / k) - crt::cos(yaw0));
    o[2] = yaw0 + s / k;
  } else {
    o[0] = x0 + s * crt::cos(yaw0);
    o[1] = y0 + s * crt::sin(yaw0);
    o[2] = yaw0;
  }
}
// CheckIfCollisionUsingPosAndYaw with the search's vehicle (A.fp: vp_ + 0.2 m, kino_astar.cpp:426-427)
__device__ inline bool sr_collides(const SearchArgs &A, double px, double py, double yaw) {
  double cs, sn;
  crt::sincos(yaw, sn, cs);
  return footprint_hits(A.grid, A.fp, px, py, cs, sn);
}
__device__ inline int sr_yaw_index(const SearchArgs &A, double yaw) { // yawToIndex, kino_astar.cpp:811-816
  yaw = pe::normalize_angle(yaw);
  return (int)floor((yaw - (-3.14159265358979323846)) * A.inv_yaw_res);
}
__device__ inline unsigned sr_hash(int ix, int iy, int iyaw) {
  unsigned h = (unsigned)ix * 73856093u ^ (unsigned)iy * 19349663u ^ (unsigned)iyaw * 83492791u;
  h ^= h >> 15;
  h *= 0x2c1b3c6du;
  h ^= h >> 12;
  return h;
}
// NodeHashTable::find: the node of (ix, iy[, iyaw]) or -1
__device__ inline int sr_find(const SearchArgs &A, const int *table, const SearchNode *pool, int ix, int iy, int iyaw, bool use3d) {
  const unsigned mask = (unsigned)A.hcap - 1u;
  unsigned s = sr_hash(ix, iy, use3d ? iyaw : 0) & mask;
  for (int probe = 0; probe < A.hcap; probe++, s = (s + 1u) & mask) {
    const int n = table[s];
    if (n < 0) return -1;
    const SearchNode &o = pool[n];
    if (o.ix == ix && o.iy == iy && (!use3d || o.yaw_idx == iyaw)) return n;
  }
  return -1;
}
__device__ inline void sr_insert(const SearchArgs &A, int *table, int ix, int iy, int iyaw, bool use3d, int node) {
  const unsigned mask = (unsigned)A.hcap - 1u;
  unsigned s = sr_hash(ix, iy, use3d ? iyaw : 0) & mask;
  for (int probe = 0; probe < A.hcap; probe++, s = (s + 1u) & mask)
    if (table[s] < 0) {
      table[s] = node;
      return;
    }
}

struct SShared {
  // the Reeds-Shepp shot
  int cnt, hit, overflow;
  // the node being expanded
  double cur[3];
  int cur_node;
  // per input of the expansion
  double pro[kSearchMaxIn][3];
  double heu[kSearchMaxIn];
  int ix[kSearchMaxIn], iy[kSearchMaxIn], yid[kSearchMaxIn], occ[kSearchMaxIn], in_range[kSearchMaxIn];
  int n_in, which;
  // control
  int go, status, shot, budget, iters, used, terminal;
  double last[3];
};

// all lanes: is the shot from `from` to the goal free (is_shot_sucess)?  1 free, 0 not, -1 more samples than the table holds
// (the host sizes the table for the longest shot the 15 m radius allows, so this does not happen)
__device__ int sr_shot_free(const SearchArgs &A, SShared &S, const double *from, const double *to, int lane) {
  typedef rs::Solver<CrMath> RS;
  if (lane == 0) {
    S.cnt = 0;
    S.hit = 0;
  }
  __syncthreads();
  const rs::Path path = RS::between(from, to, A.rho);
  const double len = A.rho * path.total; // ReedsSheppStateSpace::distance
  int c = 0;
  for (int k = lane; k < A.n_l; k += kSearchThreads) c += A.l_tab[k] <= len ? 1 : 0; // for (l = 0; l <= len; l += checkl)
  if (c) atomicAdd(&S.cnt, c);
  __syncthreads();
  const int cnt = S.cnt;
  if (cnt >= A.n_l) return -1;
  for (int k = lane; k < cnt; k += kSearchThreads) {
    double s[3];
    const double t = A.l_tab[k] / len;
    if (t >= 1.0) {
      s[0] = to[0]; s[1] = to[1]; s[2] = to[2];
    } else if (t <= 0.0) {
      s[0] = from[0]; s[1] = from[1]; s[2] = from[2];
    } else {
      RS::interpolate(from, path, A.rho, t, s);
    }
    if (sr_collides(A, s[0], s[1], s[2])) atomicOr(&S.hit, 1);
  }
  __syncthreads();
  return S.hit == 0 ? 1 : 0;
}

enum { kFieldNone = 0, kFieldMap = 1, kFieldWindow = 2 }; // the template parameter FIELD

// a windowed goal field: its cells [wy][wx] and the window's corner in the grid; F == nullptr: the query has none
struct SrWindowField {
  const int *F;
  int x0, y0, wx, wy;
  __device__ explicit operator bool() const { return F != nullptr; }
};
// what a search carries as its query's field: the whole-map field's cells, or a windowed field
template <int FIELD> struct SrFieldOf { typedef const int *type; };
template <> struct SrFieldOf<kFieldWindow> { typedef SrWindowField type; };

// the goal field's term of the heuristic at (x, y), in metres: 0 outside the grid and where the field did not reach
__device__ inline double sr_field_heu(const SearchArgs &A, const int *Fq, double x, double y) {
  const DevGrid &g = A.grid;
  const double cx = round((x - g.origin_x) / g.resolution), cy = round((y - g.origin_y) / g.resolution);
  if (!(cx >= 0.0 && cx < (double)g.size_x && cy >= 0.0 && cy < (double)g.size_y)) return 0.0;
  const int v = Fq[(size_t)(int)cx + (size_t)g.size_x * (size_t)(int)cy];
  return v == DFTPAV_FIELD_UNREACHED ? 0.0 : (double)v * A.unit;
}

// the same of a windowed field: 0 outside the window (which lies inside the grid) and where the field did not reach
__device__ inline double sr_field_heu(const SearchArgs &A, const SrWindowField &W, double x, double y) {
  const DevGrid &g = A.grid;
  const double cx = round((x - g.origin_x) / g.resolution), cy = round((y - g.origin_y) / g.resolution);
  if (!(cx >= (double)W.x0 && cx < (double)(W.x0 + W.wx) && cy >= (double)W.y0 && cy < (double)(W.y0 + W.wy))) return 0.0;
  const int v = W.F[(size_t)((int)cx - W.x0) + (size_t)W.wx * (size_t)((int)cy - W.y0)];
  return v == DFTPAV_FIELD_UNREACHED ? 0.0 : (double)v * A.unit;
}

// the Reeds-Shepp table's term of the heuristic at (x, y, yaw), in metres: 0 outside the table's extent (and for a NaN).
// gc / gs: cos / sin of the goal's yaw
__device__ inline double sr_rs_heu(const RsLookup &R, const double *en, double gc, double gs, double x, double y, double yaw) {
  const RsGeometry &g = R.g;
  const double ddx = x - en[0], ddy = y - en[1];
  const double lx = gc * ddx + gs * ddy, ly = gc * ddy - gs * ddx;
  const double fi = round(lx / g.cell) + (double)g.half, fj = round(ly / g.cell) + (double)g.half;
  if (!(fi >= 0.0 && fi < (double)g.n && fj >= 0.0 && fj < (double)g.n)) return 0.0;
  const double kd = round((yaw - en[2]) / g.dth);
  if (!(fabs(kd) < 9.0e18)) return 0.0; // (a yaw that is not finite, or beyond any int: nothing to read)
  int k = (int)((long long)kd % (long long)g.n_yaw);
  if (k < 0) k += g.n_yaw;
  return R.scale * R.tab[((size_t)k * g.n + (size_t)(int)fj) * g.n + (size_t)(int)fi];
}

// the heuristic of a state: getHeu, and the maximum with the terms the instance has
template <int FIELD, bool TABLE>
__device__ inline double sr_heu(const SearchArgs &A, const double *en, typename SrFieldOf<FIELD>::type Fq, double gc, double gs, double x,
                                double y, double yaw) {
  const dftpav_search_params &P = A.sp;
  const double dx = fabs(x - en[0]), dy = fabs(y - en[1]);
  if constexpr (TABLE) {
    double m = P.tie_breaker * sqrt(dx * dx + dy * dy);
    if constexpr (FIELD) m = fmax(m, Fq ? sr_field_heu(A, Fq, x, y) : 0.0);
    return P.lambda_heu * fmax(m, sr_rs_heu(A.rs, en, gc, gs, x, y, yaw));
  } else if constexpr (FIELD) {
    return P.lambda_heu * fmax(P.tie_breaker * sqrt(dx * dx + dy * dy), Fq ? sr_field_heu(A, Fq, x, y) : 0.0);
  } else {
    return P.lambda_heu * (P.tie_breaker * sqrt(dx * dx + dy * dy));
  }
}

// one call of KinoAstar::search(start, ctrl, end, use3d) after reset(); result in S.status / shot / budget / iters / used / terminal
template <int FIELD, bool TABLE>
__device__ void sr_search(const SearchArgs &A, SShared &S, SearchNode *pool, KinoHeap &heap, int *table, const double *st,
                          const double *en, bool use3d, int lane, typename SrFieldOf<FIELD>::type Fq, double gc, double gs) {
  const dftpav_search_params &P = A.sp;
  for (int s = lane; s < A.hcap; s += kSearchThreads) table[s] = -1;
  if (lane == 0) {
    S.status = 0;
    S.shot = 0;
    S.budget = 0;
    S.iters = 0;
    S.used = 0;
    S.terminal = -1;
    S.go = 1;
    S.occ[0] = 0;
    S.occ[1] = 0;
  }
  __syncthreads();
  // early exits, kino_astar.cpp:43-52
  if (lane < 2) {
    const double *p = lane == 0 ? st : en;
    S.occ[lane] = sr_collides(A, p[0], p[1], p[2]) ? 1 : 0;
  }
  __syncthreads();
  if (S.occ[0] || S.occ[1]) {
    if (lane == 0) S.status = kNoPath;
    __syncthreads();
    return;
  }
  // the start node, kino_astar.cpp:59-76
  bool initsearch = false;
  int singul0 = 0;
  if (fabs(st[3]) > 1e-2) singul0 = st[3] >= 0.0 ? 1 : -1; // getSingularity, kino_astar.h:210-219
  if (singul0 == 0) initsearch = true;
  if (lane == 0) {
    SearchNode &n0 = pool[0];
    n0.parent = -1;
    n0.x = st[0];
    n0.y = st[1];
    n0.yaw = st[2];
    n0.ix = (int)round((st[0] - A.origin_sx) / P.map_resl);
    n0.iy = (int)round((st[1] - A.origin_sy) / P.map_resl);
    n0.yaw_idx = sr_yaw_index(A, st[2]);
    n0.g = 0.0;
    n0.steer = 0.0;
    n0.arc = 0.0;
    n0.singul = singul0;
    n0.f = sr_heu<FIELD, TABLE>(A, en, Fq, gc, gs, st[0], st[1], st[2]);
    n0.state = kInOpen;
    heap.size = 0;
    heap.push(0, n0.f);
    S.used = 1;
    sr_insert(A, table, n0.ix, n0.iy, n0.yaw_idx, use3d, 0);
  }
  __syncthreads();
  for (;;) {
    // top of the open set (an empty set: "open set empty, no path", :298-300).  The empty set is told by cur_node, not by go:
    // other waves may still be reading go after the barrier that ended the last expansion
    if (lane == 0) {
      if (heap.empty()) {
        S.status = kNoPath;
        S.cur_node = -1;
      } else {
        const int t = heap.top();
        S.cur_node = t;
        S.cur[0] = pool[t].x;
        S.cur[1] = pool[t].y;
        S.cur[2] = pool[t].yaw;
      }
    }
    __syncthreads();
    if (S.cur_node < 0) break;
    const double cur[3] = {S.cur[0], S.cur[1], S.cur[2]};
    // the shot, :90-114
    int shot = 0;
    if (initsearch) {
      const double dx = cur[0] - en[0], dy = cur[1] - en[1];
      if (sqrt(dx * dx + dy * dy) < 15.0) shot = sr_shot_free(A, S, cur, en, lane);
    }
    if (shot < 0) {
      if (lane == 0) S.overflow = 1;
      break;
    }
    if (shot) {
      if (lane == 0) {
        S.status = kReachEnd;
        S.shot = 1;
        S.terminal = S.cur_node;
      }
      break;
    }
    // the budget, :115-132 (max_iters for the wall clock)
    if (S.iters >= P.max_iters) {
      if (lane == 0) {
        S.budget = 1;
        S.terminal = S.cur_node;
        S.status = pool[S.cur_node].parent < 0 ? kNoPath : kReachEnd;
      }
      break;
    }
    // pop, close, count, :134-136; the inputs, :143-171
    const int which = !initsearch ? (st[3] > 0 ? 0 : 1) : 2;
    initsearch = true;
    const int n_in = A.n_in[which];
    const double *tab = A.in_tab + (size_t)which * kSearchMaxIn * 2;
    __syncthreads();
    if (lane == 0) {
      heap.pop();
      pool[S.cur_node].state = kInClose;
      S.iters++;
    }
    if (lane < n_in) S.occ[lane] = 0;
    __syncthreads();
    // every input's state, indices and heuristic; every intermediate pose's collision (k = 1 .. check_num, :212-224)
    if (lane < n_in) {
      double o[3];
      sr_transit(A, cur[0], cur[1], cur[2], tab[2 * lane], tab[2 * lane + 1], o);
      S.pro[lane][0] = o[0];
      S.pro[lane][1] = o[1];
      S.pro[lane][2] = o[2];
      S.in_range[lane] = !(o[0] <= A.origin_sx || o[0] >= A.half_size_x || o[1] <= A.origin_sy || o[1] >= A.half_size_y);
      S.ix[lane] = (int)round((o[0] - A.origin_sx) / P.map_resl);
      S.iy[lane] = (int)round((o[1] - A.origin_sy) / P.map_resl);
      S.yid[lane] = sr_yaw_index(A, o[2]);
      S.heu[lane] = sr_heu<FIELD, TABLE>(A, en, Fq, gc, gs, o[0], o[1], o[2]);
    }
    if (lane < n_in * P.check_num) {
      const int i = lane / P.check_num, k = lane % P.check_num + 1;
      const double tmparc = tab[2 * i + 1] * double(k) / double(P.check_num);
      double o[3];
      sr_transit(A, cur[0], cur[1], cur[2], tab[2 * i], tmparc, o);
      if (sr_collides(A, o[0], o[1], o[2])) atomicOr(&S.occ[i], 1);
    }
    __syncthreads();
    // the serial commit, in input order (:173-295)
    if (lane == 0) {
      const int cn = S.cur_node;
      const SearchNode c = pool[cn];
      for (int i = 0; i < n_in; i++) {
        if (!S.in_range[i]) continue;
        const int ix = S.ix[i], iy = S.iy[i], yid = S.yid[i];
        int pn = sr_find(A, table, pool, ix, iy, yid, use3d);
        if (pn >= 0 && pool[pn].state == kInClose) continue;
        if (ix == c.ix && iy == c.iy && (!use3d || yid == c.yaw_idx)) continue;
        if (S.occ[i]) continue;
        const double steer = tab[2 * i], arc = tab[2 * i + 1];
        const int singul = arc > 0 ? 1 : -1;
        double g = 0.0;
        if (singul > 0) g += fabs(arc) * P.traj_forward_penalty;
        else g += fabs(arc) * P.traj_back_penalty;
        if (singul * c.singul < 0) g += P.traj_gear_switch_penalty;
        g += P.traj_steer_penalty * fabs(steer) * fabs(arc);
        g += P.traj_steer_change_penalty * fabs(steer - c.steer);
        g += c.g;
        const double f = g + S.heu[i];
        if (pn < 0) {
          pn = S.used;
          SearchNode &o = pool[pn];
          o.ix = ix;
          o.iy = iy;
          o.x = S.pro[i][0];
          o.y = S.pro[i][1];
          o.yaw = S.pro[i][2];
          o.yaw_idx = yid;
          o.f = f;
          o.g = g;
          o.steer = steer;
          o.arc = arc;
          o.parent = cn;
          o.state = kInOpen;
          o.singul = singul;
          heap.push(pn, f);
          sr_insert(A, table, ix, iy, yid, use3d, pn);
          S.used++;
          if (S.used == P.allocate_num) { // "run out of memory"
            S.status = kNoPath;
            S.go = 0;
            break;
          }
        } else if (pool[pn].state == kInOpen) {
          if (g < pool[pn].g) {
            SearchNode &o = pool[pn];
            o.ix = ix;
            o.iy = iy;
            o.x = S.pro[i][0];
            o.y = S.pro[i][1];
            o.yaw = S.pro[i][2];
            o.yaw_idx = yid;
            o.f = f;
            o.g = g;
            o.steer = steer;
            o.arc = arc;
            o.parent = cn;
            o.singul = singul;
            heap.set_key(pn, f);
          }
        }
      }
    }
    __syncthreads();
    if (!S.go) break;
  }
  __syncthreads();
}

template <int FIELD, bool TABLE> __global__ void __launch_bounds__(kSearchThreads) search_kernel(SearchArgs A) {
  __shared__ SShared S;
  const int slot = blockIdx.x, q = A.q0 + blockIdx.x, lane = threadIdx.x;
  if (q >= A.n) return;
  const dftpav_search_params &P = A.sp;
  SearchNode *pool = A.pool + (size_t)slot * P.allocate_num;
  int *table = A.table + (size_t)slot * A.hcap;
  KinoHeap heap{A.h_node + (size_t)slot * P.allocate_num, A.h_key + (size_t)slot * P.allocate_num,
                A.h_pos + (size_t)slot * P.allocate_num, 0};
  int *pidx = A.path_idx + (size_t)slot * P.allocate_num;
  double st[4], en[4];
  for (int k = 0; k < 4; k++) {
    st[k] = A.start[4 * (size_t)q + k];
    en[k] = A.end[4 * (size_t)q + k];
  }
  typename SrFieldOf<FIELD>::type Fq{}; // the goal field of this query's goal
  if constexpr (FIELD == kFieldWindow) {
    const int f = A.field_of[q];
    if (f >= 0) {
      const int *w = A.field_win + 4 * (size_t)f;
      Fq = SrWindowField{A.fields + A.field_off[f], w[0], w[1], w[2], w[3]};
    }
  } else if constexpr (FIELD) {
    const int f = A.field_of[q];
    if (f >= 0) Fq = A.fields + (size_t)f * A.grid.size_x * A.grid.size_y;
  }
  double gc = 1.0, gs = 0.0; // cos / sin of the goal's yaw: the goal's frame, in which the table is read
  if constexpr (TABLE) {
    gc = crt::cos(en[2]);
    gs = crt::sin(en[2]);
  }
  if (lane == 0) S.overflow = 0;
  __syncthreads();
  // getKinoPath, traj_manager.cpp:85-103: the first pass, then (NO_PATH, 3D) the 2D retry
  bool use3d = P.use3d != 0;
  sr_search<FIELD, TABLE>(A, S, pool, heap, table, st, en, use3d, lane, Fq, gc, gs);
  if (!S.overflow && S.status == kNoPath && use3d && P.retry_2d) {
    __syncthreads();
    use3d = false;
    sr_search<FIELD, TABLE>(A, S, pool, heap, table, st, en, false, lane, Fq, gc, gs);
  }
  __syncthreads();
  const dftpav_search_out &O = A.out;
  if (S.overflow) {
    if (lane == 0) {
      O.status[q] = 0;
      O.n_nodes[q] = 0;
      O.path_len[q] = 0;
    }
    return;
  }
  const int status = S.status;
  if (lane == 0) {
    O.status[q] = status;
    O.shot_success[q] = S.shot;
    O.used_3d[q] = use3d ? 1 : 0;
    O.budget_hit[q] = S.budget;
    O.iters[q] = S.iters;
    O.nodes_used[q] = S.used;
  }
  if (status != kReachEnd) {
    if (lane == 0) {
      O.n_nodes[q] = 0;
      O.path_len[q] = 0;
    }
    return;
  }
  // retrievePath (:351-363): the chain from the start to the terminal node
  if (lane == 0) {
    int m = 0;
    for (int n = S.terminal; n >= 0 && m < P.allocate_num; n = pool[n].parent) pidx[m++] = n;
    for (int a = 0, b = m - 1; a < b; a++, b--) {
      const int t = pidx[a];
      pidx[a] = pidx[b];
      pidx[b] = t;
    }
    S.cnt = m;
    O.n_nodes[q] = m;
    // the last rough sample: the terminal node's k = check_num pose, or the start (kino_astar.cpp:568-583)
    if (m > 1) {
      const SearchNode &nd = pool[pidx[m - 1]], &pa = pool[nd.parent];
      double o[3];
      sr_transit(A, pa.x, pa.y, pa.yaw, nd.steer, nd.arc * double(P.check_num) / double(P.check_num), o);
      S.last[0] = o[0];
      S.last[1] = o[1];
      S.last[2] = pe::normalize_angle(o[2]);
    } else {
      S.last[0] = st[0];
      S.last[1] = st[1];
      S.last[2] = pe::normalize_angle(st[2]);
    }
  }
  __syncthreads();
  const int m = S.cnt;
  for (int j = lane; j < m && j < O.max_nodes; j += kSearchThreads) {
    const SearchNode &nd = pool[pidx[j]];
    double *o = O.nodes + ((size_t)q * O.max_nodes + j) * 6;
    o[0] = nd.x;
    o[1] = nd.y;
    o[2] = nd.yaw;
    o[3] = nd.steer;
    o[4] = nd.arc;
    o[5] = (double)nd.singul;
  }
  // SampleTraj (:568-612): the start, check_num poses per node, then the shot to the goal and the goal
  double *path = O.paths + (size_t)q * O.max_path * 3;
  const int cn = P.check_num, base = 1 + (m - 1) * cn;
  if (lane == 0 && O.max_path > 0) {
    path[0] = st[0];
    path[1] = st[1];
    path[2] = pe::normalize_angle(st[2]);
  }
  for (int w = lane; w < (m - 1) * cn; w += kSearchThreads) {
    const int idx = 1 + w;
    if (idx >= O.max_path) break;
    const int j = 1 + w / cn, k = w % cn + 1;
    const SearchNode &nd = pool[pidx[j]], &pa = pool[nd.parent];
    double o[3];
    sr_transit(A, pa.x, pa.y, pa.yaw, nd.steer, nd.arc * double(k) / double(cn), o);
    path[3 * idx] = o[0];
    path[3 * idx + 1] = o[1];
    path[3 * idx + 2] = pe::normalize_angle(o[2]);
  }
  int len = base;
  if (S.shot) {
    typedef rs::Solver<CrMath> RS;
    const double from[3] = {S.last[0], S.last[1], S.last[2]};
    const rs::Path sp = RS::between(from, en, A.rho);
    const double shotLength = A.rho * sp.total;
    __syncthreads();
    if (lane == 0) S.cnt = 0;
    __syncthreads();
    int c = 0; // for (l = checkl; l < shotLength; l += checkl)
    for (int k = 1 + lane; k < A.n_l; k += kSearchThreads) c += A.l_tab[k] < shotLength ? 1 : 0;
    if (c) atomicAdd(&S.cnt, c);
    __syncthreads();
    const int n2 = S.cnt;
    if (1 + n2 >= A.n_l) { // (as in sr_shot_free: not reached with the host's table)
      if (lane == 0) {
        O.status[q] = 0;
        O.path_len[q] = 0;
      }
      return;
    }
    for (int k = lane; k < n2; k += kSearchThreads) {
      const int idx = base + k;
      if (idx >= O.max_path) break;
      double s[3];
      const double t = A.l_tab[k + 1] / shotLength;
      if (t >= 1.0) {
        s[0] = en[0]; s[1] = en[1]; s[2] = en[2];
      } else if (t <= 0.0) {
        s[0] = from[0]; s[1] = from[1]; s[2] = from[2];
      } else {
        RS::interpolate(from, sp, A.rho, t, s);
      }
      path[3 * idx] = s[0];
      path[3 * idx + 1] = s[1];
      path[3 * idx + 2] = pe::normalize_angle(s[2]);
    }
    if (lane == 0 && base + n2 < O.max_path) {
      path[3 * (base + n2)] = en[0];
      path[3 * (base + n2) + 1] = en[1];
      path[3 * (base + n2) + 2] = pe::normalize_angle(en[2]);
    }
    len = base + n2 + 1;
  }
  if (lane == 0) O.path_len[q] = len;
}

hipError_t launch_search(const SearchArgs &A, int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kSearchThreads);
  if (A.fields && A.field_win) { // windowed fields
    if (A.rs.tab) hipLaunchKernelGGL((search_kernel<kFieldWindow, true>), grid, block, 0, stream, A);
    else hipLaunchKernelGGL((search_kernel<kFieldWindow, false>), grid, block, 0, stream, A);
  } else if (A.rs.tab && A.fields) hipLaunchKernelGGL((search_kernel<kFieldMap, true>), grid, block, 0, stream, A);
  else if (A.rs.tab) hipLaunchKernelGGL((search_kernel<kFieldNone, true>), grid, block, 0, stream, A);
  else if (A.fields) hipLaunchKernelGGL((search_kernel<kFieldMap, false>), grid, block, 0, stream, A);
  else hipLaunchKernelGGL((search_kernel<kFieldNone, false>), grid, block, 0, stream, A);
  return hipGetLastError();
}

} // namespace dftpav
