// The scene prediction (include/cilqr.h, "scene prediction"), header-only: the trajectory a dynamic obstacle is taken to
// follow on the clock 0 ... span of a scene that starts at scene time t0, from nothing but the samples observed by t0.  The
// statement cilqr_predict_scene (host_planner.hip) calls and kernels_scene_predict.hip follows; cilqr_amd/scene_io.py:
// predict_trajectory is the same rule in NumPy.  Every operation is rounded once (build without contraction of a product and
// a sum into one operation); theta travels as bits.
#pragma once
#include <cstddef>
#include <cstring>

#include "scene_window.hpp"

namespace cilqr {
namespace scene_predict {

constexpr double kMargin = 1e-9;      // a sample counts as observed up to t0 + 1e-9: see cilqr.h
constexpr double kMinStep = 1e-10;    // two samples no further apart give no velocity
constexpr int kHold = 0;              // CILQR_PREDICT_HOLD
constexpr int kConstantVelocity = 1;  // CILQR_PREDICT_CONSTANT_VELOCITY

struct Motion {
  int j;                    // the latest observation; -1: unseen or left (count 0)
  double x0, y0, vx, vy;    // the position at t0 and the velocity
};

// out_samples samples of sample_dt reach past every query time of [0, span]
inline bool covers(int out_samples, double sample_dt, double span) {
  return (double)(out_samples - 1) * sample_dt >= span + kMargin;
}

// traj [T][4] time x y theta
inline Motion motion(const double* traj, int T, double t0, int mode, double max_age) {
  Motion m{-1, 0.0, 0.0, 0.0, 0.0};
  if (T < 1) return m;
  const int J = scene_window::first_true(T, [&](int k) { return kMargin < traj[(size_t)k * 4] - t0; });
  if (J == 0) return m;   // nothing observed yet
  const int j = J - 1;
  const double* s = traj + (size_t)j * 4;
  const double e = -(s[0] - t0);
  if (e > max_age) return m;   // left, or the recording ended before t0
  if (mode == kConstantVelocity && j >= 1) {
    const double h = s[0] - s[-4];
    if (h > kMinStep) {
      m.vx = (s[1] - s[-3]) / h;
      m.vy = (s[2] - s[-2]) / h;
    }
  }
  m.j = j;
  m.x0 = s[1] + m.vx * e;
  m.y0 = s[2] + m.vy * e;
  return m;
}

// The prediction into out [out_samples][4]; returns the count: out_samples, or 0 (nothing written).
inline int predict_trajectory(const double* traj, int T, double t0, int mode, double max_age, double sample_dt, int out_samples,
                              double* out) {
  const Motion m = motion(traj, T, t0, mode, max_age);
  if (m.j < 0) return 0;
  for (int i = 0; i < out_samples; ++i) {
    const double tm = (double)i * sample_dt;
    double* o = out + (size_t)i * 4;
    o[0] = tm;
    o[1] = m.x0 + m.vx * tm;
    o[2] = m.y0 + m.vy * tm;
    std::memcpy(o + 3, traj + (size_t)m.j * 4 + 3, sizeof(double));
  }
  return out_samples;
}

}  // namespace scene_predict
}  // namespace cilqr
