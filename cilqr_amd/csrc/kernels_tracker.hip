// Alternative init guess: the closed-loop tracker the reference keeps next to iqr() and recommends for
// better results (README.md:61-67; IlqrOptimizer::InitGuess, ilqr_optimizer.cc:107-139, commented out at cc:168).
//
// Reference behaviour (algorithm/ilqr/tracker.cc): Tracker::lqr cc:169-215 simulates the vehicle at sumulation_dt
// = 10 ms with RK4 (VehicleDynamic cc:83-135); every step, CalcaulateInitState cc:19-55 projects a previewed point on
// the coarse trajectory (DiscretizedTrajectory::GetProjection / EvaluateTime) and two 3-state LQR controllers give
// delta_rate and jerk (LateralControl cc:57-72, LongitudinalControl cc:74-81) from gains of the iterative DARE solver
// math::SolveLQRProblem (algorithm/math/linear_quadratic_regulator.cc:30-78), re-solved every step for the lateral
// model (it depends on the speed).  The state is kept whenever the clock passes a knot of the coarse trajectory.
//
// One lane per problem; the coarse trajectory is read batch-fastest from `goals` (knot 0 from `coarse0`, because
// goals_[0] is the start state) and `cstation`, on the time axis i dt.  The steps themselves are tracker_core.hpp's, which
// cilqr_track_rows_batch (kernels_track.hip) shares.
#include <limits.h>

#include "tracker_core.hpp"

namespace cilqr {

__global__ __launch_bounds__(64) void k_init_guess_tracker(DeviceState s, TrackerParams tp, int B,
                                                             const int* __restrict__ warm_shift) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= B) return;
  if (warm_shift != nullptr && warm_shift[slot] >= 0) return;   // warm-started (kernels_warm.hip)
  const Params& p = s.p;
  const int K = p.K, Bc = s.Bcap;
  // the coarse trajectory: knot 0 from coarse0 (goals_[0] holds the start state), time_i = i dt (dp_planner.cpp:236)
  auto follow = [&](int i) {
    tracker_core::FollowPt f;
    if (i == 0) {
      const double2 a = s.coarse0[slot], b = s.coarse0[(size_t)Bc + slot];
      f.x = a.x; f.y = a.y; f.theta = b.x; f.v = b.y;
    } else {
      const double2* gp = s.goals + (size_t)i * 3 * Bc + slot;
      const double2 a = gp[0], b = gp[(size_t)Bc];
      f.x = a.x; f.y = a.y; f.theta = b.x; f.v = b.y;
    }
    f.s = s.cstation[(size_t)i * Bc + slot];
    return f;
  };
  auto follow_xy = [&](int i, double& x, double& y) {
    const double2 a = (i == 0) ? s.coarse0[slot] : s.goals[(size_t)i * 3 * Bc + slot];
    x = a.x;
    y = a.y;
  };
  if (!tp.have_station) {   // no stations from the caller: accumulated chord length of the coarse points
    double px, py, acc = 0.0;
    follow_xy(0, px, py);
    s.cstation[slot] = 0.0;
    for (int i = 1; i < K; ++i) {
      double x, y;
      follow_xy(i, x, y);
      acc = acc + hypot_ref(x - px, y - py);
      s.cstation[(size_t)i * Bc + slot] = acc;
      px = x;
      py = y;
    }
  }
  // start_state_: x, y, theta, velocity of goals_[0]; a = delta = 0 (ilqr_optimizer.cc:61, trajectory_planner.cpp:73-76)
  double x6[6];
  {
    const double2 a = s.goals[slot], b = s.goals[(size_t)Bc + slot];
    x6[0] = a.x; x6[1] = a.y; x6[2] = b.x; x6[3] = b.y; x6[4] = 0.0; x6[5] = 0.0;
  }
  store_x(s, 0, 0, slot, x6);
  // the time axis: time_i = i dt (dp_planner.cpp:236)
  struct Axis {
    decltype(follow)& pt;
    decltype(follow_xy)& xy;
    int K;
    double dt;
    CILQR_DEV double time(int i) const { return dt * i; }
    CILQR_DEV int locate(double time) const {
      int it;
      if (time >= dt * (K - 1)) {
        it = K - 1;
      } else if (time < dt * 0) {
        it = 0;
      } else {
        it = min(K - 1, max(0, (int)(time / dt)));
        while (it > 0 && !(dt * (it - 1) < time)) --it;
        while (dt * it < time) ++it;
      }
      return it;
    }
  } axis{follow, follow_xy, K, p.dt};
  struct Keep {
    const DeviceState& s;
    int slot;
    CILQR_DEV void keep(int i, const double* x, const double* u, double) const {
      store_u(s, 0, i - 1, slot, u);
      store_x(s, 0, i, slot, x);
    }
  } sink{s, slot};
  int i = tracker_core::tracker_drive(axis, p, tp, x6, K, INT_MAX, sink);
  // the reference gives up when the count differs ("tacker failed", cc:205-208); here the remaining knots repeat the
  // last state with zero controls.  A guard only: cilqr_set_tracker_config replays this clock on the host and refuses a
  // sumulation_dt that leaves knots unvisited; what is left is a handle whose own dt the default 10 ms does not divide
  for (; i < K; ++i) {
    const double u[2] = {0.0, 0.0};
    store_u(s, 0, i - 1, slot, u);
    store_x(s, 0, i, slot, x6);   // (x y theta v a delta as tracker_drive left them)
  }
}

void launch_init_guess_tracker(const DeviceState& s, const TrackerParams& tp, int B, hipStream_t st, const int* warm_shift) {
  hipLaunchKernelGGL(k_init_guess_tracker, dim3((B + 63) / 64), dim3(64), 0, st, s, tp, B, warm_shift);
}

}  // namespace cilqr
