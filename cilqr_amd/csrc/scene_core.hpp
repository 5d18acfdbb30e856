// Device functions every kernel that reads the arrays of a cilqr_scene_batch starts with (kernels_dp.hip,
// kernels_scene_points.hip, kernels_collision.hip, kernels_clearance.hip): the rules include/cilqr.h states once, each
// stated once here, in the reference's operand order.  Built with -ffp-contract=off like everything else; cos / sin of an
// obstacle's heading are the device library's, the heading of a pose goes through lean_sincos (dev_model.hpp).
#pragma once

#include "dev_model.hpp"

namespace cilqr {

CILQR_DEV double dp_min(double a, double b) { return (b < a) ? b : a; }   // std::min
CILQR_DEV double dp_max(double a, double b) { return (a < b) ? b : a; }   // std::max

// bounding box of n >= 1 vertices as Polygon2d::BuildFromPoints takes it (polygon2d.cpp:240-257): min_x max_x min_y max_y
CILQR_DEV void dp_bounding_box(const double* pts, int n, double* box) {
  double min_x = pts[0], max_x = pts[0], min_y = pts[1], max_y = pts[1];
  for (int i = 0; i < n; ++i) {
    min_x = dp_min(min_x, pts[2 * i]);
    max_x = dp_max(max_x, pts[2 * i]);
    min_y = dp_min(min_y, pts[2 * i + 1]);
    max_y = dp_max(max_y, pts[2 * i + 1]);
  }
  box[0] = min_x; box[1] = max_x; box[2] = min_y; box[3] = max_y;
}

// counts scene b may carry (S static and D dynamic slots of up to V vertices): anything else marks it invalid (DEVICE
// arrays; HOST arrays are checked before the launch)
CILQR_DEV bool scene_counts_valid(int b, int S, int D, int V, int max_samples, const int* static_counts,
                                  const int* dyn_poly_counts, const int* dyn_traj_counts) {
  bool ok = true;
  for (int o = 0; o < S; ++o) {
    const int n = static_counts[(size_t)b * S + o];
    ok = ok && n >= 0 && n <= V;
  }
  for (int d = 0; d < D; ++d) {
    const int m = dyn_poly_counts[(size_t)b * D + d], T = dyn_traj_counts[(size_t)b * D + d];
    ok = ok && m >= 0 && m <= V && T >= 0 && T <= max_samples;
  }
  return ok;
}

// a static polygon of n >= 1 vertices into its record: the box in rec[0..3], the vertices behind it
CILQR_DEV void scene_stage_static(const double* src, int n, double* rec) {
  for (int v = 0; v < 2 * n; ++v) rec[4 + v] = src[v];
  dp_bounding_box(rec + 4, n, rec);
}

// the dynamic slots of scene b into LDS by a workgroup of `block` lanes: vertex counts, sample counts, body-frame polygons
CILQR_DEV void scene_stage_dynamic(int b, int D, int V, int block, const double* dyn_poly, const int* dyn_poly_counts,
                                   const int* dyn_traj_counts, int* s_m, int* s_T, double* s_body) {
  const int tid = threadIdx.x;
  if (tid < D) {
    s_m[tid] = dyn_poly_counts[(size_t)b * D + tid];
    s_T[tid] = dyn_traj_counts[(size_t)b * D + tid];
  }
  for (int i = tid; i < D * V * 2; i += block) s_body[i] = dyn_poly[(size_t)b * D * V * 2 + i];
}

// Which sample of traj [T][4] (time x y theta, times non-decreasing) an obstacle shows at time t.  It is there from its
// first to its last sample (environment.cpp:117) and shows the first sample with t < sample time (std::upper_bound), past
// the end the last one.  kEps: the 1e-10 of Query...ObstaclesPoints on all three comparisons (environment.cpp:137-146);
// without it no `+ 0.0` is executed.
template <bool kEps>
CILQR_DEV bool scene_present(const double* traj, int T, double t) {
  if (T < 1) return false;
  return kEps ? !(traj[0] > t + kMathEps || traj[(size_t)(T - 1) * 4] < t - kMathEps)
              : !(traj[0] > t || traj[(size_t)(T - 1) * 4] < t);
}
template <bool kEps>
CILQR_DEV int scene_sample_index(const double* traj, int T, double t) {   // T >= 1
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kEps ? t < traj[(size_t)mid * 4] + kMathEps : t < traj[(size_t)mid * 4]) hi = mid;
    else lo = mid + 1;
  }
  return lo >= T ? T - 1 : lo;
}
// both: the index, or -1 where the obstacle is not there
template <bool kEps>
CILQR_DEV int scene_sample(const double* traj, int T, double t) {
  return scene_present<kEps>(traj, T, t) ? scene_sample_index<kEps>(traj, T, t) : -1;
}

// Pose::transform (pose.h:40-46) of body-frame vertex v by the pose (x, y, cos, sin)
CILQR_DEV void scene_place_vertex(const double* body, int v, double x, double y, double c, double s, double* ox, double* oy) {
  const double vx = body[2 * v], vy = body[2 * v + 1];
  *ox = x + vx * c - vy * s;
  *oy = y + vx * s + vy * c;
}
CILQR_DEV void scene_place(const double* body, int m, double x, double y, double c, double s, double* out) {
  for (int v = 0; v < m; ++v) scene_place_vertex(body, v, x, y, c, s, out + 2 * v, out + 2 * v + 1);
}

// the centres of the vehicle's two collision discs at a pose (vehicle_param.h:88-95): rear x y, front x y
CILQR_DEV void scene_discs_of_pose(double x, double y, double theta, double r2x, double f2x, double* out4) {
  double st, ct;
  lean_sincos(theta, &st, &ct);
  out4[0] = x + r2x * ct;
  out4[1] = y + r2x * st;
  out4[2] = x + f2x * ct;
  out4[3] = y + f2x * st;
}

// Polygon2d::BuildFromPoints (polygon2d.cpp:219-226) stores a polygon reversed when this sum of CrossProd(p0, p[i-1], p[i])
// is negative; vertex(i, &x, &y) yields vertex i of m >= 1 (ScenePolygon: the vertices of an array [m][2])
struct ScenePolygon {
  const double* pts;
  CILQR_DEV void operator()(int i, double* x, double* y) const { *x = pts[2 * i]; *y = pts[2 * i + 1]; }
};
template <class Vertex>
CILQR_DEV bool scene_area_negative(Vertex vertex, int m) {
  double x0, y0, px, py;
  vertex(0, &x0, &y0);
  px = x0;
  py = y0;
  double area = 0.0;
  for (int i = 1; i < m; ++i) {
    double cx, cy;
    vertex(i, &cx, &cy);
    area = area + ((px - x0) * (cy - y0) - (py - y0) * (cx - x0));
    px = cx;
    py = cy;
  }
  return area < 0.0;
}

// The points [first, last) of the x-sorted barrier table [nb][2] a square spanning [min_x, max_x] can touch
// (environment.cpp:54-80): two upper_bounds on x and the one predecessor; nothing where the square lies beside the table.
// nb >= 0, the size of a table.  dp_static_collision (dp_core.hpp) keeps its own statement of this search: with the
// shared one inlined k_dp_plan measured 3 % slower
CILQR_DEV void scene_barrier_window(const double* barrier, int nb, double min_x, double max_x, int* first, int* last) {
  *first = 0;
  *last = 0;
  if (nb == 0 || max_x < barrier[0] || min_x > barrier[(size_t)(nb - 1) * 2]) return;
  auto upper = [&](double val) {   // first barrier point with val < point.x
    int lo = 0, hi = nb;
    while (lo < hi) {
      const int mid = (lo + hi) / 2;
      if (val < barrier[(size_t)mid * 2]) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  };
  *first = upper(min_x);
  *last = upper(max_x);
  if (*first > 0) --*first;
}

}  // namespace cilqr
