// The DP coarse planner for a batch of scenes (C-ABI: cilqr_dp_plan_batch): DpPlanner::Plan
// (algorithm/planner/dp_planner.cpp:135-281) + ComputePathProfile (algorithm/utils/discrete_points_math.cc:27-176)
// with the arithmetic of include/cilqr/dp_planner.hpp (dp_core.hpp); what is new here is the schedule.
//
// Scenes share nothing but the road, so ONE WORKGROUP PLANS ONE SCENE; inside it the work of a layer is the
// 70 x 70 (parent, child) transitions, each a loop over the 10-20 samples of its path segment with two collision discs
// held against every obstacle -- independent of each other, dealt to the 256 lanes (consecutive lanes take consecutive
// children of one parent: neighbouring lateral offsets, similar trip counts).  A lane leaves its loop at the first
// blocked sample, as the host does: "blocked" is a boolean over the samples.  The step costs of a layer land in LDS;
// then 70 lanes -- one per child -- scan their 70 candidates IN THE HOST'S ORDER (parents si-major / li-minor) with its
// strict '<' on from.cost + step_cost, so a child keeps the first parent that reaches it most cheaply.  The leaf pick,
// the walk back and the running chord length are serial and done by one lane; the knots of the chosen path are again
// one lane each.  Every index is bounded by the max_* the call was given; counts outside them mark the scene invalid.
//
//   k_dp_place   pre-pass, one lane per (scene, path sample, dynamic obstacle): the time of a path sample depends on
//                (layer, i) alone, so the polygon a dynamic obstacle shows to ANY transition at that sample is one
//                polygon -- picked, placed and boxed (scene_core.hpp) once, instead of once per collision test.  The
//                pick is a bisection: on the non-decreasing sample times cilqr.h declares, the index of the host's scan.
//   k_dp_plan    the planner.
// The centre line and the x-sorted road-barrier table are built on the host once per call by the host planner's own
// code and read by all workgroups through L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dp_core.hpp"

namespace cilqr {

namespace {

constexpr int kDpBlock = 256;
constexpr int kDpMaxQ = 256;   // CILQR_DP_MAX_KNOTS: path samples of the five layers together

}  // namespace

// placed [n_scenes][nq][max_dynamic][4 + 2 max_vertices], placed_n [n_scenes][nq][max_dynamic]; scene = first + local index
__global__ __launch_bounds__(kDpBlock) void k_dp_place(DpParams P, int first, int n_scenes,
                                                       const double* __restrict__ dyn_poly,
                                                       const int* __restrict__ dyn_poly_counts,
                                                       const double* __restrict__ dyn_traj,
                                                       const int* __restrict__ dyn_traj_counts,
                                                       double* __restrict__ placed, int* __restrict__ placed_n) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)n_scenes * P.nq * P.max_dynamic;
  if (t >= total) return;
  const int d = (int)(t % P.max_dynamic);
  const int q = (int)((t / P.max_dynamic) % P.nq);
  const int local = (int)(t / ((long long)P.max_dynamic * P.nq));
  const int b = first + local;
  const int rec = 4 + 2 * P.max_vertices;
  double* out = placed + (size_t)t * rec;
  const int m = dyn_poly_counts[(size_t)b * P.max_dynamic + d], T = dyn_traj_counts[(size_t)b * P.max_dynamic + d];
  // an unused slot, an obstacle without samples (AddDynamic drops it), or counts the planner refuses anyway
  if (m < 1 || m > P.max_vertices || T < 1 || T > P.max_samples) {
    placed_n[t] = 0;
    return;
  }
  int layer = 0;
  while (layer + 1 < kDpLayers && q >= P.qoff[layer + 1]) ++layer;
  const int i = q - P.qoff[layer];
  const double from_time = layer == 0 ? 0.0 : P.time[layer - 1];
  const double when = from_time + i * (P.unit_time / P.nseg[layer]);
  const double* traj = dyn_traj + ((size_t)b * P.max_dynamic + d) * P.max_samples * 4;
  const int k = scene_sample<false>(traj, T, when);
  if (k < 0) {
    placed_n[t] = 0;
    return;
  }
  const double* tp = traj + (size_t)k * 4;
  scene_place(dyn_poly + ((size_t)b * P.max_dynamic + d) * P.max_vertices * 2, m, tp[1], tp[2], cos(tp[3]), sin(tp[3]), out + 4);
  dp_bounding_box(out + 4, m, out);
  placed_n[t] = m;
}

__global__ __launch_bounds__(kDpBlock) void k_dp_plan(DpParams P, int first, const double* __restrict__ start3,
                                                      const double* __restrict__ static_points,
                                                      const int* __restrict__ static_counts,
                                                      const int* __restrict__ dyn_poly_counts,
                                                      const int* __restrict__ dyn_traj_counts,
                                                      const double* __restrict__ placed, const int* __restrict__ placed_n,
                                                      double* __restrict__ coarse9, double* __restrict__ coarse6,
                                                      double* __restrict__ knots3, double* __restrict__ station,
                                                      int* __restrict__ found, int* __restrict__ n_not_found) {
  const int tid = threadIdx.x;
  const int local = blockIdx.x, b = first + local;
  const int K = P.n_knots, nq = P.nq;

  __shared__ double s_static[CILQR_DP_MAX_STATIC * kDpRec];
  __shared__ int s_static_n[CILQR_DP_MAX_STATIC];
  __shared__ double s_cost[kDpLayers][kDpCells], s_reach[kDpLayers][kDpCells];   // Cell::cost, Cell::current_s
  __shared__ short s_parent[kDpLayers][kDpCells];                                  // parent cell (si * 10 + li), -1 = none
  __shared__ DpOrigin s_origin[kDpCells];
  // step costs of a layer's 4900 transitions; before and after the relaxation the same words hold the reduction of the
  // projection and the arrays of the chosen path
  __shared__ double s_work[kDpCells * kDpCells];
  __shared__ double s_start[2];   // station and lateral offset of the start
  __shared__ int s_chosen[kDpLayers];
  __shared__ int s_flag[2];       // counts valid, found

  // ---- the scene: counts, static polygons with their boxes
  if (tid == 0)
    s_flag[0] = scene_counts_valid(b, P.max_static, P.max_dynamic, P.max_vertices, P.max_samples, static_counts,
                                   dyn_poly_counts, dyn_traj_counts) ? 1 : 0;
  __syncthreads();
  if (s_flag[0] == 0) {   // (uniform) rows of zeros, not found
    for (int k = tid; k < K; k += kDpBlock) {
      const size_t row = (size_t)b * K + k;
      if (coarse9) for (int e = 0; e < CILQR_COARSE_FIELDS; ++e) coarse9[row * CILQR_COARSE_FIELDS + e] = 0.0;
      if (coarse6) for (int e = 0; e < 6; ++e) coarse6[row * 6 + e] = 0.0;
      if (knots3) for (int e = 0; e < 3; ++e) knots3[row * 3 + e] = 0.0;
      if (station) station[row] = 0.0;
    }
    if (tid == 0) {
      found[b] = 0;
      atomicAdd(n_not_found, 1);
    }
    return;
  }
  if (tid < P.max_static) {
    const int n = static_counts[(size_t)b * P.max_static + tid];
    s_static_n[tid] = n;
    if (n > 0) scene_stage_static(static_points + ((size_t)b * P.max_static + tid) * P.max_vertices * 2, n, s_static + tid * kDpRec);
  }
  DpScene S;
  S.statics = s_static;
  S.static_n = s_static_n;
  S.placed = placed + (size_t)local * nq * P.max_dynamic * (4 + 2 * P.max_vertices);
  S.placed_n = placed_n + (size_t)local * nq * P.max_dynamic;

  // ---- GetProjection (discretized_trajectory.cpp:165-197): the FIRST nearest centre point, so the minimum is taken over
  // (squared distance, index); a lane that saw nothing smaller than the initial bound reports index 0, as the host's
  // loop leaves it
  const double px = start3[(size_t)b * 3], py = start3[(size_t)b * 3 + 1];
  {
    double* red_v = s_work;
    int* red_i = reinterpret_cast<int*>(s_work + kDpBlock);
    double nearest = DBL_MAX;
    int idx = INT32_MAX;
    for (int i = tid; i < P.n_center; i += kDpBlock) {
      const double dx = P.center[(size_t)i * 7 + 1] - px, dy = P.center[(size_t)i * 7 + 2] - py;
      const double d = dx * dx + dy * dy;
      if (d < nearest) {
        idx = i;
        nearest = d;
      }
    }
    red_v[tid] = nearest;
    red_i[tid] = idx;
    __syncthreads();
    for (int w = kDpBlock / 2; w > 0; w >>= 1) {
      if (tid < w) {
        const double v2 = red_v[tid + w];
        const int i2 = red_i[tid + w];
        if (v2 < red_v[tid] || (v2 == red_v[tid] && i2 < red_i[tid])) {
          red_v[tid] = v2;
          red_i[tid] = i2;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int n = P.n_center;
      const int at = red_i[0] == INT32_MAX ? 0 : red_i[0];
      DpRef proj = dp_center_point(P, at);
      const int i0 = at > 0 ? at - 1 : 0;
      const int i1 = min(n - 1, at + 1);
      if (i0 < i1) {
        const DpRef p0 = dp_center_point(P, i0), p1 = dp_center_point(P, i1);
        const double v0x = px - p0.x, v0y = py - p0.y;
        const double v1x = p1.x - p0.x, v1y = p1.y - p0.y;
        const double v1_norm = sqrt(v1x * v1x + v1y * v1y);
        const double dot = v0x * v1x + v0y * v1y;
        const double delta_s = dot / v1_norm;
        proj = dp_interpolate(p0, p1, p0.s + delta_s);
      }
      const double nr_x = px - proj.x, nr_y = py - proj.y;
      double sn, cs;
      lean_sincos(proj.theta, &sn, &cs);   // the sign of the side alone
      s_start[0] = proj.s;
      s_start[1] = copysign(hypot_ref(nr_x, nr_y), nr_y * cs - nr_x * sn);
    }
    __syncthreads();
  }
  const double start_s = s_start[0], start_l = s_start[1];

  // ---- Relax (dp_planner.cpp:144-184).  First layer from the start state: assigned, not compared
  if (tid < kDpCells) {
    const DpOrigin o{start_s, start_l, start_s, start_l, start_s, start_l, 0.0};
    const int si = tid / kDpLaterals, li = tid % kDpLaterals;
    s_cost[0][tid] = dp_transition(P, S, o, 0, si, li);
    s_reach[0][tid] = o.s + P.station[si];
    s_parent[0][tid] = -1;
  }
  __syncthreads();
  for (int t = 0; t + 1 < kDpLayers; ++t) {
    // every cell of layer t as the origin of its 70 transitions (OriginOf): worked out once per parent
    if (tid < kDpCells) {
      const int si = tid / kDpLaterals, li = tid % kDpLaterals;
      DpOrigin o;
      o.cost = s_cost[t][tid];
      o.s = s_reach[t][tid];
      o.l = dp_lateral_at(P, o.s, li);
      o.before_s = start_s;
      o.before_l = start_l;
      if (t >= 1) {
        // (a cell without a parent exists only where every cost is NaN -- a non-finite start; the host reads outside its
        // table there, this reads cell 0)
        const int par = max((int)s_parent[t][tid], 0);
        o.before_s = s_reach[t - 1][par];
        o.before_l = dp_lateral_at(P, o.before_s, par % kDpLaterals);
      }
      const int n_own = P.nseg[t];
      const double end_s = o.before_s + P.station[si];
      const double end_l = dp_lateral_at(P, end_s, li);
      const double step_s = P.station[si] / n_own;
      const double step_l = (end_l - o.before_l) / n_own;
      o.tail_s = o.before_s + (n_own - 1) * step_s;
      o.tail_l = o.before_l + (n_own - 1) * step_l;
      s_origin[tid] = o;
    }
    __syncthreads();
    for (int tr = tid; tr < kDpCells * kDpCells; tr += kDpBlock) {
      const int par = tr / kDpCells, child = tr - par * kDpCells;
      const DpOrigin o = s_origin[par];
      s_work[tr] = dp_transition(P, S, o, t + 1, child / kDpLaterals, child % kDpLaterals);
    }
    __syncthreads();
    if (tid < kDpCells) {   // Expand, seen from the child: parents in the host's loop order, strict '<'
      double cost = DBL_MAX, reach = DBL_MIN;
      int parent = -1;
      const int si = tid / kDpLaterals;
      for (int par = 0; par < kDpCells; ++par) {
        const double total = s_origin[par].cost + s_work[par * kDpCells + tid];
        if (total < cost) {
          cost = total;
          reach = s_origin[par].s + P.station[si];
          parent = par;
        }
      }
      s_cost[t + 1][tid] = cost;
      s_reach[t + 1][tid] = reach;
      s_parent[t + 1][tid] = (short)parent;
    }
    __syncthreads();
  }

  // ---- Backtrack (dp_planner.cpp:187-215): the first cheapest leaf and its ancestors
  if (tid == 0) {
    double best = DBL_MAX;
    int at = 0;
    for (int c = 0; c < kDpCells; ++c)
      if (s_cost[kDpLayers - 1][c] < best) {
        at = c;
        best = s_cost[kDpLayers - 1][c];
      }
    for (int t = kDpLayers - 1; t >= 0; --t) {
      s_chosen[t] = at;
      at = max((int)s_parent[t][at], 0);
    }
    const int ok = best < P.w_obstacle ? 1 : 0;
    s_flag[1] = ok;
    found[b] = ok;
    if (!ok) atomicAdd(n_not_found, 1);
  }
  __syncthreads();

  // ---- Sample (dp_planner.cpp:217-275): the nq samples of the chosen polyline, then ComputePathProfile on their x / y
  double* q_s = s_work;                 // (s, l) of every path sample
  double* q_l = q_s + kDpMaxQ;
  double* q_x = q_l + kDpMaxQ;
  double* q_y = q_x + kDpMaxQ;
  double* q_th = q_y + kDpMaxQ;
  double* acc = q_th + kDpMaxQ;         // chord lengths, then the accumulated s
  double* vel = acc + kDpMaxQ;
  double* accel = vel + kDpMaxQ;
  double* d1x = accel + kDpMaxQ;
  double* d1y = d1x + kDpMaxQ;
  double* kap = d1y + kDpMaxQ;
  static_assert(11 * kDpMaxQ <= kDpCells * kDpCells, "the path's arrays live in the step-cost block");
  for (int k = tid; k < nq; k += kDpBlock) {   // SegmentSamples of the layer the sample belongs to
    int t = 0;
    while (t + 1 < kDpLayers && k >= P.qoff[t + 1]) ++t;
    const int i = k - P.qoff[t];
    const int cell = s_chosen[t], si = cell / kDpLaterals, li = cell % kDpLaterals;
    const int par = s_parent[t][cell];
    double p_s = start_s, p_l = start_l;
    if (par >= 0) {
      p_s = t > 0 ? s_reach[t - 1][s_chosen[t - 1]] : start_s;
      p_l = dp_lateral_at(P, p_s, par % kDpLaterals);
    }
    const int n = P.nseg[t];
    const double end_s = p_s + P.station[si];
    const double end_l = dp_lateral_at(P, end_s, li);
    const double step_s = P.station[si] / n;
    const double step_l = (end_l - p_l) / n;
    q_s[k] = p_s + i * step_s;
    q_l[k] = p_l + i * step_l;
  }
  __syncthreads();
  for (int k = tid; k < nq; k += kDpBlock) {
    const double seen_s = k > 0 ? q_s[k - 1] : start_s, seen_l = k > 0 ? q_l[k - 1] : start_l;
    const double rise = q_l[k] - seen_l;
    const double run = dp_max(q_s[k] - seen_s, kDpEps);
    const DpRef r = dp_evaluate_station(P, q_s[k]);
    double sn, cs;
    lean_sincos(r.theta, &sn, &cs);
    q_x[k] = r.x - q_l[k] * sn;   // GetCartesian
    q_y[k] = r.y + q_l[k] * cs;
    q_th[k] = r.theta + atan((rise / run) / (1 - r.kappa * q_l[k]));
  }
  __syncthreads();
  for (int k = tid; k < nq; k += kDpBlock) {
    double chord = 0.0;
    if (k > 0) {
      const double ex = q_x[k - 1] - q_x[k], ey = q_y[k - 1] - q_y[k];
      chord = sqrt(ex * ex + ey * ey);
    }
    acc[k] = chord;
  }
  __syncthreads();
  if (tid == 0)   // the running chord length is a serial sum: s[i] = sqrt(..) + s[i - 1]
    for (int k = 1; k < nq; ++k) acc[k] = acc[k] + acc[k - 1];
  __syncthreads();
  auto lo_of = [](int i) { return i > 0 ? i - 1 : 0; };
  auto hi_of = [nq](int i) { return i + 1 < nq ? i + 1 : nq - 1; };
  for (int k = tid; k < nq; k += kDpBlock) {   // forward differences in time; the last knot repeats its predecessor
    const int i = k + 1 < nq ? k : nq - 2;
    vel[k] = (acc[i + 1] - acc[i]) / P.delta_t;
    const int lo = lo_of(k), hi = hi_of(k);     // first derivative over s
    d1x[k] = (q_x[hi] - q_x[lo]) / (acc[hi] - acc[lo]);
    d1y[k] = (q_y[hi] - q_y[lo]) / (acc[hi] - acc[lo]);
  }
  __syncthreads();
  for (int k = tid; k < nq; k += kDpBlock) {
    const int i = k + 1 < nq ? k : nq - 2;
    accel[k] = (vel[i + 1] - vel[i]) / P.delta_t;
    const int lo = lo_of(k), hi = hi_of(k);     // second derivative: the same operator on its own output
    const double d2x = (d1x[hi] - d1x[lo]) / (acc[hi] - acc[lo]);
    const double d2y = (d1y[hi] - d1y[lo]) / (acc[hi] - acc[lo]);
    const double g2 = d1x[k] * d1x[k] + d1y[k] * d1y[k];
    kap[k] = (d1x[k] * d2y - d1y[k] * d2x) / (sqrt(g2) * g2 + 1e-6);
  }
  __syncthreads();
  for (int k = tid; k < K; k += kDpBlock) {
    double row[CILQR_COARSE_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // knots past the path's samples stay as constructed
    if (k < nq) {
      row[0] = P.delta_t * k;
      row[1] = q_s[k];
      row[2] = q_x[k];
      row[3] = q_y[k];
      row[4] = q_th[k];
      row[5] = kap[k];
      row[6] = vel[k];
      row[7] = accel[k];
      row[8] = atan(kap[k] * P.wheel_base);
    }
    const size_t at = (size_t)b * K + k;
    if (coarse9) for (int e = 0; e < CILQR_COARSE_FIELDS; ++e) coarse9[at * CILQR_COARSE_FIELDS + e] = row[e];
    if (coarse6) {
      double* o = coarse6 + at * 6;
      o[0] = row[2]; o[1] = row[3]; o[2] = row[4]; o[3] = row[6]; o[4] = row[7]; o[5] = row[8];
    }
    if (knots3) {
      double* o = knots3 + at * 3;
      o[0] = row[2]; o[1] = row[3]; o[2] = row[4];
    }
    if (station) station[at] = row[1];
  }
}

void launch_dp_place(const DpParams& P, const cilqr_scene_batch& dv, int first, int n_scenes, double* placed, int* placed_n,
                     hipStream_t st) {
  const long long total = (long long)n_scenes * P.nq * P.max_dynamic;
  if (total <= 0) return;
  hipLaunchKernelGGL(k_dp_place, dim3((unsigned)((total + kDpBlock - 1) / kDpBlock)), dim3(kDpBlock), 0, st, P, first,
                     n_scenes, dv.dynamic_polygon_points, dv.dynamic_polygon_counts, dv.dynamic_trajectories,
                     dv.dynamic_trajectory_counts, placed, placed_n);
}

void launch_dp_plan(const DpParams& P, const cilqr_scene_batch& dv, int first, int n_scenes, const double* start3,
                    const double* placed, const int* placed_n, double* coarse9, double* coarse6, double* knots3,
                    double* station, int* found, int* n_not_found, hipStream_t st) {
  hipLaunchKernelGGL(k_dp_plan, dim3(n_scenes), dim3(kDpBlock), 0, st, P, first, start3, dv.static_points, dv.static_counts,
                     dv.dynamic_polygon_counts, dv.dynamic_trajectory_counts, placed, placed_n, coarse9, coarse6, knots3,
                     station, found, n_not_found);
}

}  // namespace cilqr
