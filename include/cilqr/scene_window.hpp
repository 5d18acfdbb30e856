// The scene window (include/cilqr.h, "scene window"), header-only: which samples of a dynamic obstacle's trajectory a scene
// that starts at scene time t0 and is read on the clock 0 ... span needs, and those samples on that clock.  The statement
// cilqr_window_scene (host_planner.hip) calls and kernels_scene_window.hip follows; cilqr_amd/scene_io.py: window_trajectory
// is the same rule in NumPy.  Every operation is rounded once; x, y and theta travel as bits.
#pragma once
#include <cstddef>
#include <cstring>

namespace cilqr {
namespace scene_window {

constexpr double kMargin = 1e-9;   // against the 1e-10 of the Query...Points rule (scene_core.hpp): see cilqr.h

// std::lower_bound's halving written out over a predicate: the first k of [0, T) with pred(k), T if the halving meets
// none -- defined whether or not pred is monotone
template <class Pred>
inline int first_true(int T, Pred pred) {
  int first = 0, len = T;
  while (len > 0) {
    const int half = len >> 1;
    if (!pred(first + half)) {
      first += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return first;
}

struct Bounds {
  int lo, hi, count;   // samples lo ... hi; count = hi - lo + 1 (0 and lo = 0, hi = -1 for T < 1)
};

// traj [T][4] time x y theta.  For T >= 1 the count is >= 1 on any input: the second predicate implies the first, so the
// two halvings probe the same samples until one goes left where the other goes right, and L <= H.
inline Bounds window_bounds(const double* traj, int T, double t0, double span) {
  if (T < 1) return Bounds{0, -1, 0};
  const double upper = span + kMargin;
  const int L = first_true(T, [&](int k) { return !(traj[(size_t)k * 4] - t0 < -kMargin); });
  const int H = first_true(T, [&](int k) { return upper < traj[(size_t)k * 4] - t0; });
  const int lo = L - 1 > 0 ? L - 1 : 0;
  const int hi = H < T - 1 ? H : T - 1;
  return Bounds{lo, hi, hi - lo + 1};
}

// The window into out [out_samples][4]; returns the count, or -1 (nothing written) where it exceeds out_samples.
inline int window_trajectory(const double* traj, int T, double t0, double span, int out_samples, double* out) {
  const Bounds w = window_bounds(traj, T, t0, span);
  if (w.count > out_samples) return -1;
  for (int j = 0; j < w.count; ++j) {
    const double* s = traj + (size_t)(w.lo + j) * 4;
    double* o = out + (size_t)j * 4;
    o[0] = s[0] - t0;
    std::memcpy(o + 1, s + 1, 3 * sizeof(double));
  }
  return w.count;
}

}  // namespace scene_window
}  // namespace cilqr
