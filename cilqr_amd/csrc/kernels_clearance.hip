// How close every knot of a batch of trajectories comes to the obstacles of its scene (C-ABI: cilqr_clearance_rows_batch;
// the rule is stated once, in include/cilqr.h under "clearance"): Polygon2d::DistanceTo(Vec2d) (polygon2d.cpp:43-52) from
// the two disc centres to every static polygon and to every dynamic polygon present at the knot's time, as
// DpEnvironment::Clearance (include/cilqr/dp_planner.hpp) states it.  The point-in-polygon test and the bounding box are
// dp_core.hpp's, hypot is dev_model.hpp's libm-identical hypot_ref; the steps on the scene's arrays (counts, staging, sample
// choice, placement, disc centres, area sign) are scene_core.hpp's.
//
// ONE WORKGROUP PER SCENE, and everything a scene's knots share stays in LDS:
//   * one lane per static slot normalises its polygon once -- reversed if the area sum is negative, boxed after that -- and
//     leaves box, vertices and the (unit vector, length) of every edge in LDS; the body-frame polygons of the dynamic
//     obstacles are staged as they are;
//   * one lane per knot reads the pose from the row (time, x, y, theta) and leaves the time and the two disc centres in LDS;
//   * the lanes stride over the (knot, dynamic slot) pairs: a pair's lane picks the sample, places the polygon into its own
//     record in LDS (so nothing is indexed in registers and nothing goes to scratch), normalises it there, and measures it
//     against both discs, edge by edge;
//   * the same lanes stride over the (knot, static slot) pairs;
//   * THE MINIMUM OVER THE SLOTS OF A KNOT uses no atomic and does not depend on the order of the lanes.  The slots are
//     padded to a power of two G <= 32, pair p = knot * G + slot, so the G lanes of a knot are neighbours in one wavefront
//     and every round of the stride loop has the same trip count in every lane: log2 G butterfly steps (__shfl_xor) on
//     (distance, slot), compared lexicographically, leave the smallest pair in every lane of the group.  A slot that is
//     unused, absent at the knot's time or whose distance is not < +inf enters as (+inf, no slot), which is the rule's
//     "best = +inf, slot = -1, replaced only by d < best";
//   * one lane per knot (n_knots <= 256 = the workgroup) subtracts the radius, writes its row and takes the smallest of
//     its four values; (value, knot) is reduced the same way inside each wavefront and across the four through LDS.
// Every index is bounded by the max_* of the call and by n_knots <= CILQR_DP_MAX_KNOTS; a scene whose counts leave them gets
// min_knot -2, a NaN min_clearance and NaN rows (DEVICE arrays; HOST arrays are refused before the launch).
// Built with -ffp-contract=off like every other file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cmath>

#include "clearance.hpp"
#include "dp_core.hpp"

namespace cilqr {

namespace {

constexpr int kClBlock = 256;
constexpr int kClWave = 64;
constexpr int kClMaxK = CILQR_DP_MAX_KNOTS;
constexpr int kClMaxS = CILQR_DP_MAX_STATIC;
constexpr int kClMaxD = CILQR_DP_MAX_DYNAMIC;
constexpr int kClStaticRec = 4 + 2 * kDpMaxV + 3 * kDpMaxV + 1;   // box, vertices, (ux, uy, length) per edge; odd stride
constexpr int kClLaneRec = 2 * kDpMaxV + 1;                       // a lane's placed polygon: its vertices (the box stays in registers); odd stride
constexpr int kClNoSlot = INT_MAX;
static_assert(kDpMaxV == CILQR_DP_MAX_VERTICES, "a polygon record holds the declared number of vertices");
static_assert(kClMaxK <= kClBlock, "one lane per knot writes the rows and enters the scene's minimum");
static_assert(kClMaxS <= 32 && kClMaxD <= 32, "the slots of a knot fit one wavefront's butterfly");

// hypot as the C library returns it: an infinite component wins over a NaN; everything else is hypot_ref's
CILQR_DEV double cl_hypot(double x, double y) {
  if (isinf(x) || isinf(y)) return HUGE_VAL;
  return hypot_ref(x, y);
}

// Polygon2d::BuildFromPoints (polygon2d.cpp:219-226, 246-256) on n >= 1 vertices in place: reversed if the area sum
// (scene_core.hpp) is negative, then boxed
CILQR_DEV void cl_normalise(double* pts, int n, double* box) {
  if (scene_area_negative(ScenePolygon{pts}, n))
    for (int i = 0, j = n - 1; i < j; ++i, --j) {
      const double x = pts[2 * i], y = pts[2 * i + 1];
      pts[2 * i] = pts[2 * j]; pts[2 * i + 1] = pts[2 * j + 1];
      pts[2 * j] = x; pts[2 * j + 1] = y;
    }
  dp_bounding_box(pts, n, box);
}

// LineSegment2d's constructor (line_segment2d.cpp:40-49) for edge i of n: unit vector and length
CILQR_DEV void cl_edge(const double* pts, int n, int i, double* ux, double* uy, double* length) {
  const int j = i >= n - 1 ? 0 : i + 1;
  const double dx = pts[2 * j] - pts[2 * i], dy = pts[2 * j + 1] - pts[2 * i + 1];
  const double len = cl_hypot(dx, dy);
  const bool point = len <= kMathEps;
  *ux = point ? 0.0 : dx / len;
  *uy = point ? 0.0 : dy / len;
  *length = len;
}

// LineSegment2d::DistanceTo (line_segment2d.cpp:61-75)
CILQR_DEV double cl_edge_distance(double sx, double sy, double ux, double uy, double len, double ex, double ey, double px, double py) {
  const double x0 = px - sx, y0 = py - sy;
  if (len <= kMathEps) return cl_hypot(x0, y0);
  const double proj = x0 * ux + y0 * uy;
  if (proj <= 0.0) return cl_hypot(x0, y0);
  if (proj >= len) return cl_hypot(px - ex, py - ey);
  return fabs(x0 * uy - y0 * ux);
}

// Polygon2d::DistanceTo (polygon2d.cpp:43-52) from the two disc centres c[0..1] (rear), c[2..3] (front) to a normalised
// polygon; edges: its (ux, uy, length) triples, or nullptr to take them from the vertices
CILQR_DEV void cl_polygon_distance(const double* box, const double* pts, const double* edges, int n, const double* c,
                                   double* d_rear, double* d_front) {
  double dr = HUGE_VAL, df = HUGE_VAL;
  for (int i = 0; i < n; ++i) {
    const int j = i >= n - 1 ? 0 : i + 1;
    double ux, uy, len;
    if (edges) {
      ux = edges[3 * i]; uy = edges[3 * i + 1]; len = edges[3 * i + 2];
    } else {
      cl_edge(pts, n, i, &ux, &uy, &len);
    }
    const double sx = pts[2 * i], sy = pts[2 * i + 1], ex = pts[2 * j], ey = pts[2 * j + 1];
    const double er = cl_edge_distance(sx, sy, ux, uy, len, ex, ey, c[0], c[1]);
    const double ef = cl_edge_distance(sx, sy, ux, uy, len, ex, ey, c[2], c[3]);
    dr = (er < dr) ? er : dr;   // std::min(d, e): a NaN is never taken
    df = (ef < df) ? ef : df;
  }
  *d_rear = dp_poly_has_point(box, pts, n, c[0], c[1]) ? 0.0 : dr;
  *d_front = dp_poly_has_point(box, pts, n, c[2], c[3]) ? 0.0 : df;
}

// the smallest (value, index) pair, compared lexicographically, among the `group` neighbouring lanes (a power of two <= 64,
// every lane of the wavefront active): left in every lane of the group
CILQR_DEV void cl_group_min(double* value, int* index, int group) {
  double v = *value;
  int at = *index;
  for (int w = 1; w < group; w <<= 1) {
    const double ov = __shfl_xor(v, w);
    const int oat = __shfl_xor(at, w);
    const bool take = ov < v || (ov == v && oat < at);
    v = take ? ov : v;
    at = take ? oat : at;
  }
  *value = v;
  *index = at;
}

CILQR_DEV int cl_group_of(int slots) {   // the power of two the slots of a knot are padded to
  int g = 1;
  while (g < slots) g <<= 1;
  return g;
}

}  // namespace

__global__ __launch_bounds__(kClBlock) void k_clearance(ClearanceParams P, const double* __restrict__ rows,
                                                        const double* __restrict__ static_points,
                                                        const int* __restrict__ static_counts,
                                                        const double* __restrict__ dyn_poly,
                                                        const int* __restrict__ dyn_poly_counts,
                                                        const double* __restrict__ dyn_traj,
                                                        const int* __restrict__ dyn_traj_counts,
                                                        double* __restrict__ clearance, int* __restrict__ nearest,
                                                        double* __restrict__ min_clearance, int* __restrict__ min_knot,
                                                        int* __restrict__ n_below) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int K = P.n_knots, S = P.max_static, D = P.max_dynamic, V = P.max_vertices;

  __shared__ double s_static[kClMaxS * kClStaticRec];   // box, vertices, edges of the normalised polygons
  __shared__ double s_body[kClMaxD * kDpMaxV * 2];      // body-frame polygons
  __shared__ double s_placed[kClBlock * kClLaneRec];    // per lane: the polygon it placed
  __shared__ double s_disc[kClMaxK * 4];                // rear x y, front x y
  __shared__ double s_time[kClMaxK];
  __shared__ double s_best[kClMaxK * 4];                // distances: rear static, rear dynamic, front static, front dynamic
  __shared__ int s_near[kClMaxK * 4];
  __shared__ double s_wave_min[kClBlock / kClWave];
  __shared__ int s_wave_knot[kClBlock / kClWave];
  __shared__ int s_static_n[kClMaxS], s_m[kClMaxD], s_T[kClMaxD];
  __shared__ int s_ok;

  if (tid == 0) s_ok = scene_counts_valid(b, S, D, V, P.max_samples, static_counts, dyn_poly_counts, dyn_traj_counts) ? 1 : 0;
  __syncthreads();
  if (s_ok == 0) {   // (uniform)
    for (int i = tid; i < K * 4; i += kClBlock) {
      if (clearance) clearance[(size_t)b * K * 4 + i] = NAN;
      if (nearest) nearest[(size_t)b * K * 4 + i] = -1;
    }
    if (tid == 0) {
      min_clearance[b] = NAN;
      min_knot[b] = -2;
    }
    return;
  }

  // ---- the scene and the knots
  if (tid < S) {
    const int n = static_counts[(size_t)b * S + tid];
    s_static_n[tid] = n;
    if (n > 0) {
      double* rec = s_static + tid * kClStaticRec;
      const double* src = static_points + ((size_t)b * S + tid) * V * 2;
      for (int v = 0; v < 2 * n; ++v) rec[4 + v] = src[v];
      cl_normalise(rec + 4, n, rec);
      double* edges = rec + 4 + 2 * kDpMaxV;
      for (int i = 0; i < n; ++i) cl_edge(rec + 4, n, i, edges + 3 * i, edges + 3 * i + 1, edges + 3 * i + 2);
    }
  }
  scene_stage_dynamic(b, D, V, kClBlock, dyn_poly, dyn_poly_counts, dyn_traj_counts, s_m, s_T, s_body);
  for (int k = tid; k < K; k += kClBlock) {
    const double* row = rows + ((size_t)b * K + k) * P.rows.fields;
    s_time[k] = row[P.rows.time];
    scene_discs_of_pose(row[P.rows.x], row[P.rows.y], row[P.rows.theta], P.r2x, P.f2x, s_disc + 4 * k);
    for (int c = 0; c < 4; ++c) {
      s_best[4 * k + c] = HUGE_VAL;
      s_near[4 * k + c] = -1;
    }
  }
  __syncthreads();

  // ---- (knot, dynamic slot): environment.cpp:113-130, then polygon2d.cpp:43-52
  if (D > 0) {
    const int G = cl_group_of(D);
    double* placed = s_placed + tid * kClLaneRec;
    for (int base = 0; base < K * G; base += kClBlock) {   // the same trips in every lane: the butterfly needs them all
      const int p = base + tid;
      const int k = p / G, d = p - k * G;
      double d_rear = HUGE_VAL, d_front = HUGE_VAL;
      if (k < K && d < D) {
        const int m = s_m[d];
        const double* traj = dyn_traj + ((size_t)b * D + d) * P.max_samples * 4;
        const int T = s_T[d];
        const double t = s_time[k];
        if (m >= 1 && scene_present<false>(traj, T, t)) {
          const double* tp = traj + (size_t)scene_sample_index<false>(traj, T, t) * 4;
          scene_place(s_body + d * V * 2, m, tp[1], tp[2], cos(tp[3]), sin(tp[3]), placed);
          double box[4];
          cl_normalise(placed, m, box);
          cl_polygon_distance(box, placed, nullptr, m, s_disc + 4 * k, &d_rear, &d_front);
        }
      }
      int at_rear = d_rear < HUGE_VAL ? d : kClNoSlot, at_front = d_front < HUGE_VAL ? d : kClNoSlot;
      d_rear = d_rear < HUGE_VAL ? d_rear : HUGE_VAL;   // (a NaN distance is not taken either)
      d_front = d_front < HUGE_VAL ? d_front : HUGE_VAL;
      cl_group_min(&d_rear, &at_rear, G);
      cl_group_min(&d_front, &at_front, G);
      if (k < K && d == 0) {
        s_best[4 * k + 1] = d_rear;
        s_near[4 * k + 1] = at_rear == kClNoSlot ? -1 : at_rear;
        s_best[4 * k + 3] = d_front;
        s_near[4 * k + 3] = at_front == kClNoSlot ? -1 : at_front;
      }
    }
  }

  // ---- (knot, static slot)
  if (S > 0) {
    const int G = cl_group_of(S);
    for (int base = 0; base < K * G; base += kClBlock) {
      const int p = base + tid;
      const int k = p / G, o = p - k * G;
      double d_rear = HUGE_VAL, d_front = HUGE_VAL;
      if (k < K && o < S) {
        const int n = s_static_n[o];
        if (n >= 1) {
          const double* rec = s_static + o * kClStaticRec;
          cl_polygon_distance(rec, rec + 4, rec + 4 + 2 * kDpMaxV, n, s_disc + 4 * k, &d_rear, &d_front);
        }
      }
      int at_rear = d_rear < HUGE_VAL ? o : kClNoSlot, at_front = d_front < HUGE_VAL ? o : kClNoSlot;
      d_rear = d_rear < HUGE_VAL ? d_rear : HUGE_VAL;
      d_front = d_front < HUGE_VAL ? d_front : HUGE_VAL;
      cl_group_min(&d_rear, &at_rear, G);
      cl_group_min(&d_front, &at_front, G);
      if (k < K && o == 0) {
        s_best[4 * k] = d_rear;
        s_near[4 * k] = at_rear == kClNoSlot ? -1 : at_rear;
        s_best[4 * k + 2] = d_front;
        s_near[4 * k + 2] = at_front == kClNoSlot ? -1 : at_front;
      }
    }
  }
  __syncthreads();

  // ---- the rows, the smallest value of the scene and the first knot that has it
  double lowest = HUGE_VAL;
  int at = kClNoSlot;
  if (tid < K) {
    for (int c = 0; c < 4; ++c) {
      const double v = s_best[4 * tid + c] - P.radius;   // +inf stays +inf
      if (clearance) clearance[((size_t)b * K + tid) * 4 + c] = v;
      if (nearest) nearest[((size_t)b * K + tid) * 4 + c] = s_near[4 * tid + c];
      if (v < lowest) {
        lowest = v;
        at = tid;
      }
    }
  }
  cl_group_min(&lowest, &at, kClWave);
  if ((tid & (kClWave - 1)) == 0) {
    s_wave_min[tid / kClWave] = lowest;
    s_wave_knot[tid / kClWave] = at;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kClBlock / kClWave; ++w)   // later wavefronts hold later knots: a strict `<` keeps the first
      if (s_wave_min[w] < lowest) {
        lowest = s_wave_min[w];
        at = s_wave_knot[w];
      }
    min_clearance[b] = lowest;
    min_knot[b] = at == kClNoSlot ? -1 : at;
    if (lowest < P.threshold) atomicAdd(n_below, 1);
  }
}

void launch_clearance(const ClearanceParams& P, const cilqr_scene_batch& dv, const double* rows, double* clearance,
                      int* nearest, double* min_clearance, int* min_knot, int* n_below, hipStream_t st) {
  if (dv.batch <= 0) return;
  hipLaunchKernelGGL(k_clearance, dim3(dv.batch), dim3(kClBlock), 0, st, P, rows, dv.static_points, dv.static_counts,
                     dv.dynamic_polygon_points, dv.dynamic_polygon_counts, dv.dynamic_trajectories,
                     dv.dynamic_trajectory_counts, clearance, nearest, min_clearance, min_knot, n_below);
}

}  // namespace cilqr
