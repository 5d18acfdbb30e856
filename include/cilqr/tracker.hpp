// include/cilqr/tracker.hpp -- the closed-loop Tracker (Tracker::Plan, algorithm/ilqr/tracker.cc:12-215) on rows in the
// layouts of include/cilqr.h: the host statement of cilqr_track_rows, which cilqr_track_rows_batch is held to, and below it
// an adapter with the reference's call surface (Tracker(config, vehicle), Init, Plan) for callers who hold the reference's
// types.
// Header-only, C++14, no HIP.  The rule is stated once, in include/cilqr.h ("track"); this file follows it step by step.
// Every operation is written so that it rounds once (build without contraction: -ffp-contract=off where the target has a
// fused multiply-add); sin / cos / tan are the C library's.
#ifndef CILQR_TRACKER_HPP_
#define CILQR_TRACKER_HPP_

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "trajectory_queries.hpp"

namespace cilqr {
namespace tracker {

constexpr int kMaxSimSteps = 32768;   // CILQR_TRACKER_MAX_SIM_STEPS
constexpr int kDrivenFields = 10;     // CILQR_TRAJ_FIELDS

// the 13 fields of cilqr_tracker_config / TrackerConfig (planner_config.h:18-43)
struct Config {
  double weight_l = 1e-1, weight_theta = 1e-12, weight_delta = 1e-12, weight_delta_rate = 0.1, preview_time = 0.2;
  double weight_s = 5.0 * 1e-1, weight_v = 1e-12, weight_a = 1e-12, weight_j = 0.1;
  double sumulation_dt = 0.01, dt = 0.1, tolerance = 0.01;
  int max_num_iteration = 150;
};
// what the tracker reads of VehicleParam (vehicle_param.h:31-64)
struct Vehicle {
  double wheel_base = 1.0;
  double delta_min = -40.0 / 180 * 3.14159265358979323846, delta_max = 40.0 / 180 * 3.14159265358979323846;
  double delta_rate_min = -40.0 / 180 * 3.14159265358979323846 / 3.0, delta_rate_max = 40.0 / 180 * 3.14159265358979323846 / 3.0;
  double jerk_min = -10.0, jerk_max = 10.0;
  double min_acceleration = -5.0, max_acceleration = 5.0;
};

// a configuration the rule can run at all (what cilqr_set_tracker_config asks of the values alone)
inline bool config_valid(const Config& c, int max_iterations = 1000) {
  const double f[12] = {c.weight_l, c.weight_theta, c.weight_delta, c.weight_delta_rate, c.preview_time, c.weight_s,
                        c.weight_v, c.weight_a, c.weight_j, c.sumulation_dt, c.dt, c.tolerance};
  for (double v : f)
    if (!std::isfinite(v)) return false;
  return c.sumulation_dt > 0.0 && c.dt > 0.0 && c.tolerance >= 0.0 && c.max_num_iteration >= 1 &&
         c.max_num_iteration <= max_iterations;
}

// fmax / fmin written out, so that they are one thing under every compiler: a NaN loses, of equal arguments the first wins
inline double max_of(double a, double b) { return (a >= b || b != b) ? a : b; }
inline double min_of(double a, double b) { return (a <= b || b != b) ? a : b; }

// row-major 3x3 products, every element accumulated k = 0, 1, 2
inline void mul33(const double* a, const double* b, double* r) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = a[i * 3 + 0] * b[0 * 3 + j];
      s += a[i * 3 + 1] * b[1 * 3 + j];
      s += a[i * 3 + 2] * b[2 * 3 + j];
      r[i * 3 + j] = s;
    }
}
inline void row33(const double* v, const double* m, double* out) {   // (1x3) (3x3)
  for (int j = 0; j < 3; ++j) {
    double s = v[0] * m[0 * 3 + j];
    s += v[1] * m[1 * 3 + j];
    s += v[2] * m[2 * 3 + j];
    out[j] = s;
  }
}
inline double dot3(const double* a, const double* b) {
  double s = a[0] * b[0];
  s += a[1] * b[1];
  s += a[2] * b[2];
  return s;
}

// the gains of the rule: A, Q 3x3 row-major, B [3], R scalar -> K [3]
inline void solve_lqr(const double* A, const double* B, const double* Q, double R, double tolerance, int max_iter, double* K) {
  double AT[9], P[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) AT[i * 3 + j] = A[j * 3 + i];
  std::memcpy(P, Q, sizeof(P));
  int num_iteration = 0;
  double diff = DBL_MAX;
  while (num_iteration++ < max_iter && diff > tolerance) {
    double ATP[9], ATPA[9], ATPB[3], BTP[3], BTPA[3], Pn[9];
    mul33(AT, P, ATP);
    mul33(ATP, A, ATPA);
    for (int i = 0; i < 3; ++i) ATPB[i] = dot3(ATP + i * 3, B) + 0.0;
    row33(B, P, BTP);
    const double inv = 1.0 / (R + dot3(BTP, B));
    row33(BTP, A, BTPA);
    double maxc = -DBL_MAX;
    for (int i = 0; i < 3; ++i) {
      const double left = ATPB[i] * inv;
      for (int j = 0; j < 3; ++j) {
        const double pn = (ATPA[i * 3 + j] - left * (BTPA[j] + 0.0)) + Q[i * 3 + j];
        maxc = max_of(maxc, pn - P[i * 3 + j]);
        Pn[i * 3 + j] = pn;
      }
    }
    diff = std::fabs(maxc);
    std::memcpy(P, Pn, sizeof(P));
  }
  double BTP[3], BTPA[3];
  row33(B, P, BTP);
  const double inv = 1.0 / (R + dot3(BTP, B));
  row33(BTP, A, BTPA);
  for (int j = 0; j < 3; ++j) K[j] = inv * (BTPA[j] + 0.0);
}

// the columns of a trajectory layout (row_layouts.hpp); fields = 0: no such layout.  station < 0: chord length
using FollowColumns = RowColumns;
constexpr FollowColumns follow_columns(int layout) { return trajectory_columns(layout); }

// One trajectory: rows [n_knots][fields] of `layout`, start6 (or nullptr: row 0) -> driven [n_drive][10].  The arguments are
// taken as checked (cilqr_track_rows).  true: n_drive rows were recorded; false: the failure of the rule, `driven` all zero.
inline bool track_rows(const Config& cfg, const Vehicle& veh, int layout, const double* rows, int n_knots, const double* start6,
                       int n_drive, double* driven, int max_steps = kMaxSimSteps) {
  namespace tq = trajectory_queries;
  const FollowColumns c = follow_columns(layout);
  const int K = n_knots, F = c.fields;
  // the follow table: time, station, x, y, theta, v per knot
  std::vector<double> tab((size_t)K * 6);
  double *ft = tab.data(), *fs = ft + K, *fx = fs + K, *fy = fx + K, *fth = fy + K, *fv = fth + K;
  for (int k = 0; k < K; ++k) {
    const double* r = rows + (size_t)k * F;
    ft[k] = r[c.time]; fx[k] = r[c.x]; fy[k] = r[c.y]; fth[k] = r[c.theta]; fv[k] = r[c.v];
    if (c.station >= 0) fs[k] = r[c.station];
  }
  if (c.station < 0) {
    double acc = 0.0;
    fs[0] = 0.0;
    for (int k = 1; k < K; ++k) {
      acc = acc + hypot_ref(fx[k] - fx[k - 1], fy[k] - fy[k - 1]);
      fs[k] = acc;
    }
  }
  // InitMatrix
  double latA[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, latQ[9] = {0}, lonA[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, lonQ[9] = {0};
  const double latB[3] = {0.0, 0.0, 1.0 * cfg.dt}, lonB[3] = {0.0, 0.0, 1.0 * cfg.dt};
  latQ[0] = cfg.weight_l; latQ[4] = cfg.weight_theta; latQ[8] = cfg.weight_delta;
  lonA[1] = cfg.dt;
  lonA[5] = -cfg.dt;
  lonQ[0] = cfg.weight_s; lonQ[4] = cfg.weight_v; lonQ[8] = cfg.weight_a;
  double Klon[3];
  solve_lqr(lonA, lonB, lonQ, cfg.weight_j, cfg.tolerance, cfg.max_num_iteration, Klon);

  double cx, cy, cth, cv, ca, cdl;
  if (start6 != nullptr) {
    cx = start6[0]; cy = start6[1]; cth = start6[2]; cv = start6[3]; ca = start6[4]; cdl = start6[5];
  } else {
    cx = rows[c.x]; cy = rows[c.y]; cth = rows[c.theta]; cv = rows[c.v]; ca = rows[c.a]; cdl = rows[c.delta];
  }
  const double L = veh.wheel_base;
  auto record = [&](int i, double time) {
    double* o = driven + (size_t)i * kDrivenFields;
    o[0] = time; o[1] = cx; o[2] = cy; o[3] = cth; o[4] = cv; o[5] = ca; o[6] = cdl;
    o[7] = std::tan(cdl) / L;
    o[8] = 0.0; o[9] = 0.0;
  };
  const double start_time = ft[0], end_time = ft[K - 1];
  record(0, start_time);
  double ctime = start_time;
  int i = 1, steps = 0;
  for (double t = start_time; t < end_time + kMathEps && i < n_drive && steps < max_steps; t += cfg.sumulation_dt, ++steps) {
    // ---- preview and projection
    double sn, cs;
    tq::sin_cos(cth, &sn, &cs);
    const double pvx = cx + cs * cv * cfg.preview_time;
    const double pvy = cy + sn * cv * cfg.preview_time;
    int at = 0;
    {
      double nearest = DBL_MAX;
      for (int k = 0; k < K; ++k) {
        const double dx = fx[k] - pvx, dy = fy[k] - pvy;
        const double d = dx * dx + dy * dy;
        if (d < nearest) {
          nearest = d;
          at = k;
        }
      }
    }
    double ps = fs[at], px = fx[at], py = fy[at], pth = fth[at];
    {
      const int i0 = at > 0 ? at - 1 : 0, i1 = at + 1 < K - 1 ? at + 1 : K - 1;
      if (i0 < i1) {
        const double v0x = pvx - fx[i0], v0y = pvy - fy[i0];
        const double v1x = fx[i1] - fx[i0], v1y = fy[i1] - fy[i0];
        const double v1_norm = std::sqrt(v1x * v1x + v1y * v1y);
        const double dot = v0x * v1x + v0y * v1y;
        const double st = fs[i0] + dot / v1_norm;
        if (std::fabs(fs[i1] - fs[i0]) < kMathEps) {
          ps = fs[i0]; px = fx[i0]; py = fy[i0]; pth = fth[i0];
        } else {
          const double w = (st - fs[i0]) / (fs[i1] - fs[i0]);
          ps = st;
          px = (1 - w) * fx[i0] + w * fx[i1];
          py = (1 - w) * fy[i0] + w * fy[i1];
          pth = tq::slerp(fth[i0], fs[i0], fth[i1], fs[i1], st);
        }
      }
    }
    double psn, pcs;
    tq::sin_cos(pth, &psn, &pcs);
    const double ddx = cx - px, ddy = cy - py;
    const double lat[3] = {psn * ddx - pcs * ddy, tq::NormalizeAngle(pth - cth), cdl};
    // ---- the followed trajectory at the clock's time
    double match_s, match_v;
    {
      const double time = ctime + 0.0;
      const int it = tq::bracket(ft, 1, 0, K, time);
      const double t0 = ft[it - 1], t1 = ft[it];
      if (std::fabs(t1 - t0) < kMathEps) {
        match_s = fs[it - 1];
        match_v = fv[it - 1];
      } else {
        const double w = (time - t0) / (t1 - t0);
        match_s = (1 - w) * fs[it - 1] + w * fs[it];
        match_v = (1 - w) * fv[it - 1] + w * fv[it];
      }
    }
    const double lon[3] = {match_s - ps, match_v - cv, ca};
    // ---- controls
    const double v_amend = max_of(2.0, cv);
    latA[1] = v_amend * 0.1;
    latA[5] = -v_amend / L * 0.1;
    double Klat[3];
    solve_lqr(latA, latB, latQ, cfg.weight_delta_rate, cfg.tolerance, cfg.max_num_iteration, Klat);
    double delta_rate = -dot3(Klat, lat), jerk = -dot3(Klon, lon);
    delta_rate = max_of(veh.delta_rate_min, min_of(veh.delta_rate_max, delta_rate));
    jerk = max_of(veh.jerk_min, min_of(veh.jerk_max, jerk));
    // ---- RK4
    {
      const double h = cfg.sumulation_dt, h2 = h / 2.0;
      double k1[3], k2[3], k3[3], k4[3];
      auto mode = [&](double th, double v, double dl, double* o) {
        double sn_, cs_;
        tq::sin_cos(th, &sn_, &cs_);
        o[0] = v * cs_;
        o[1] = v * sn_;
        o[2] = v * std::tan(dl) / L;
      };
      mode(cth, cv, cdl, k1);
      const double a1 = ca, a2 = ca + jerk * h2, a3 = ca + jerk * h2, a4 = ca + jerk * h;
      mode(cth + k1[2] * h2, cv + a1 * h2, cdl + delta_rate * h2, k2);
      mode(cth + k2[2] * h2, cv + a2 * h2, cdl + delta_rate * h2, k3);
      mode(cth + k3[2] * h, cv + a3 * h, cdl + delta_rate * h, k4);
      const double nx = cx + (k1[0] + k2[0] * 2.0 + k3[0] * 2.0 + k4[0]) / 6.0 * h;
      const double ny = cy + (k1[1] + k2[1] * 2.0 + k3[1] * 2.0 + k4[1]) / 6.0 * h;
      const double nth = tq::NormalizeAngle(cth + (k1[2] + k2[2] * 2.0 + k3[2] * 2.0 + k4[2]) / 6.0 * h);
      const double nv = max_of(0.0, cv + (a1 + a2 * 2.0 + a3 * 2.0 + a4) / 6.0 * h);
      const double ndl = tq::NormalizeAngle(min_of(
          veh.delta_max, max_of(veh.delta_min, cdl + (delta_rate + delta_rate * 2.0 + delta_rate * 2.0 + delta_rate) / 6.0 * h)));
      const double na = min_of(veh.max_acceleration, max_of(veh.min_acceleration, ca + (jerk + jerk * 2.0 + jerk * 2.0 + jerk) / 6.0 * h));
      cx = nx; cy = ny; cth = nth; cv = nv; cdl = ndl; ca = na;
    }
    ctime = t;
    if (i < K && ctime > ft[i] - kMathEps) {
      double* prev = driven + (size_t)(i - 1) * kDrivenFields;
      prev[8] = jerk;
      prev[9] = delta_rate;
      record(i, ctime);
      ++i;
    }
  }
  if (i == n_drive) return true;
  std::memset(driven, 0, sizeof(double) * (size_t)n_drive * kDrivenFields);
  return false;
}

}  // namespace tracker

// Tracker with the reference's call surface (algorithm/ilqr/tracker.h:13-52).  TrackerConfig, VehicleParam, TrajectoryPoint
// and DiscretizedTrajectory are the caller's types: the members planner_config.h:18-43, vehicle_param.h:31-64 and
// discretized_trajectory.h:22-43 name are all that is read.  Plan follows `coarse_traj` (time, s, x, y, theta, velocity of
// its points) from `start_state` (x, y, theta, velocity, a, delta) and hands back one point per followed point: time, x, y,
// theta, velocity, a, delta, kappa, jerk, delta_rate.  false: the reference's "tacker failed"; *opt_trajectory is untouched.
template <class TrackerConfig, class VehicleParam>
class TrackerT {
 public:
  TrackerT() = default;
  TrackerT(const TrackerConfig& config, const VehicleParam& param) { Init(config, param); }

  void Init(const TrackerConfig& config, const VehicleParam& param) {
    cfg_.weight_l = config.lateral_config.weight_l;
    cfg_.weight_theta = config.lateral_config.weight_theta;
    cfg_.weight_delta = config.lateral_config.weight_delta;
    cfg_.weight_delta_rate = config.lateral_config.weight_delta_rate;
    cfg_.preview_time = config.lateral_config.preview_time;
    cfg_.weight_s = config.longitudinal_config.weight_s;
    cfg_.weight_v = config.longitudinal_config.weight_v;
    cfg_.weight_a = config.longitudinal_config.weight_a;
    cfg_.weight_j = config.longitudinal_config.weight_j;
    cfg_.sumulation_dt = config.sumulation_dt;
    cfg_.dt = config.dt;
    cfg_.tolerance = config.tolerance;
    cfg_.max_num_iteration = (int)config.max_num_iteration;
    veh_.wheel_base = param.wheel_base;
    veh_.delta_min = param.delta_min; veh_.delta_max = param.delta_max;
    veh_.delta_rate_min = param.delta_rate_min; veh_.delta_rate_max = param.delta_rate_max;
    veh_.jerk_min = param.jerk_min; veh_.jerk_max = param.jerk_max;
    veh_.min_acceleration = param.min_acceleration; veh_.max_acceleration = param.max_acceleration;
  }

  template <class TrajectoryPoint, class DiscretizedTrajectory>
  bool Plan(const TrajectoryPoint& start_state, const DiscretizedTrajectory& coarse_traj,
            DiscretizedTrajectory* const opt_trajectory) const {
    const auto& pts = coarse_traj.trajectory();
    const int K = (int)pts.size();
    if (opt_trajectory == nullptr || K < 2 || !tracker::config_valid(cfg_)) return false;
    std::vector<double> rows((size_t)K * 9, 0.0), driven((size_t)K * tracker::kDrivenFields);   // CILQR_ROWS_COARSE
    for (int k = 0; k < K; ++k) {
      double* r = rows.data() + (size_t)k * 9;
      r[0] = pts[k].time; r[1] = pts[k].s; r[2] = pts[k].x; r[3] = pts[k].y; r[4] = pts[k].theta; r[5] = pts[k].kappa;
      r[6] = pts[k].velocity; r[7] = pts[k].a; r[8] = pts[k].delta;
    }
    const double start6[6] = {start_state.x, start_state.y, start_state.theta, start_state.velocity, start_state.a,
                              start_state.delta};
    if (!tracker::track_rows(cfg_, veh_, 2, rows.data(), K, start6, K, driven.data())) return false;
    std::vector<TrajectoryPoint> out((size_t)K);
    for (int k = 0; k < K; ++k) {
      const double* d = driven.data() + (size_t)k * tracker::kDrivenFields;
      TrajectoryPoint& p = out[k];
      p.time = d[0]; p.x = d[1]; p.y = d[2]; p.theta = d[3]; p.velocity = d[4]; p.a = d[5]; p.delta = d[6]; p.kappa = d[7];
      p.jerk = d[8]; p.delta_rate = d[9];
    }
    *opt_trajectory = DiscretizedTrajectory(out);
    return true;
  }

 private:
  tracker::Config cfg_;
  tracker::Vehicle veh_;
};

}  // namespace cilqr

#endif  // CILQR_TRACKER_HPP_
