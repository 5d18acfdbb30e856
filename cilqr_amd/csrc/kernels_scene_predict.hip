// cilqr_predict_scenes_batch (include/cilqr.h, "scene prediction"): for every dynamic obstacle of a batch the trajectory it
// is taken to follow on the clock 0 ... span of a scene that starts at its own t0, from the samples observed by t0 alone,
// written where the scene kernels read next.  The host statement is include/cilqr/scene_predict.hpp; this file follows it
// operation by operation (-ffp-contract=off: time - t0, the two differences and quotients of the velocity, and product then
// sum, two roundings, for every position), so the predictions are its bits.
//
// One wavefront per (scene, dynamic slot); the four wavefronts of a workgroup take neighbouring slots of one scene, as in
// kernels_scene_window.hip.
//   search  ONE border, the latest sample observed by t0, found by the wave together (wave_search.hpp: sw_wave_first): two
//           rounds for the 1501 samples of a 15 s recording.  On non-decreasing times the predicate is monotone and the
//           index is the halving's; on times that decrease it may differ, and still lies in [0, T].
//   read    all lanes read samples j and j - 1 (the same two lines) and derive the motion, each for itself.
//   write   lane m writes samples m, m + 64, ...: 32 bytes per lane, 2 KiB of contiguous output per wave and step.  16-byte
//           stores where the output base is 16-byte aligned (a slot's offset is a multiple of 32 bytes), 8-byte stores
//           otherwise.
// Every index that is probed or read lies in [0, T) with T <= max_samples checked first, on any input.  No atomics here and
// no kernel of its own for the flags: k_scene_window_ok (kernels_scene_window.hip) folds the counts into ok and the total.
#include "dev_model.hpp"
#include "scene_predict.hpp"
#include "scene_window.hpp"
#include "wave_search.hpp"

namespace cilqr {

constexpr int kSpWaves = 4;   // slots of one scene per workgroup
constexpr int kSpLanes = kSwWave * kSpWaves;

__global__ __launch_bounds__(kSpLanes) void k_scene_predict(ScenePredictParams P, int groups, const double* __restrict__ src,
                                                            const int* __restrict__ src_counts, const double* __restrict__ t0,
                                                            double* __restrict__ out, int* __restrict__ out_counts) {
  const int lane = threadIdx.x & (kSwWave - 1), wave = threadIdx.x >> 6;
  const int D = P.max_dynamic;
  const int b = (int)(blockIdx.x / (unsigned)groups);
  const int d = (int)(blockIdx.x - (unsigned)b * (unsigned)groups) * kSpWaves + wave;
  if (d >= D) return;   // the whole wave
  const size_t slot = (size_t)b * D + d;
  // ---- what refuses the scene as a whole: a source count it cannot carry, a t0 that is no time
  bool bad = false;
  for (int o = lane; o < D; o += kSwWave) {
    const int n = src_counts[(size_t)b * D + o];
    bad = bad || n < 0 || n > P.max_samples;
  }
  const double t0b = t0[b];
  bad = bad || !(fabs(t0b) <= DBL_MAX);
  if (__ballot(bad) != 0ull) {
    if (lane == 0) out_counts[slot] = -1;
    return;
  }
  const int T = src_counts[slot];
  if (T < 1) {
    if (lane == 0) out_counts[slot] = 0;
    return;
  }
  // ---- the latest observation
  const double* __restrict__ tr = src + slot * (size_t)P.max_samples * 4;
  const int J = sw_wave_first(T, lane, [&](int k) { return scene_predict::kMargin < tr[(size_t)k * 4] - t0b; });   // in [0, T]
  if (J == 0) {   // unseen
    if (lane == 0) out_counts[slot] = 0;
    return;
  }
  const int j = J - 1;
  const double* __restrict__ s = tr + (size_t)j * 4;
  const double tj = s[0], xj = s[1], yj = s[2], thj = s[3];
  const double e = -(tj - t0b);
  if (e > P.max_age) {   // left
    if (lane == 0) out_counts[slot] = 0;
    return;
  }
  // ---- the motion
  double vx = 0.0, vy = 0.0;
  if (P.mode == scene_predict::kConstantVelocity && j >= 1) {
    const double h = tj - s[-4];
    if (h > scene_predict::kMinStep) {
      vx = (xj - s[-3]) / h;
      vy = (yj - s[-2]) / h;
    }
  }
  const double x0 = xj + vx * e, y0 = yj + vy * e;
  if (lane == 0) out_counts[slot] = P.out_samples;
  // ---- the samples
  double* __restrict__ o = out + slot * (size_t)P.out_samples * 4;
  const bool wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (wide) {
    for (int m = lane; m < P.out_samples; m += kSwWave) {
      const double tm = (double)m * P.sample_dt;
      double2 v0, v1;
      v0.x = tm;
      v0.y = x0 + vx * tm;
      v1.x = y0 + vy * tm;
      v1.y = thj;
      *reinterpret_cast<double2*>(o + (size_t)m * 4) = v0;
      *reinterpret_cast<double2*>(o + (size_t)m * 4 + 2) = v1;
    }
  } else {
    for (int m = lane; m < P.out_samples; m += kSwWave) {
      const double tm = (double)m * P.sample_dt;
      double* om = o + (size_t)m * 4;
      om[0] = tm;
      om[1] = x0 + vx * tm;
      om[2] = y0 + vy * tm;
      om[3] = thj;
    }
  }
}

void launch_scene_predict(const ScenePredictParams& P, const double* src, const int* src_counts, const double* t0, double* out,
                          int* out_counts, int* ok, int* n_failed, hipStream_t st) {
  if (P.max_dynamic > 0) {
    const int groups = (P.max_dynamic + kSpWaves - 1) / kSpWaves;
    const dim3 grid((unsigned)((long long)P.batch * groups));   // the host has checked that this fits
    hipLaunchKernelGGL(k_scene_predict, grid, dim3(kSpLanes), 0, st, P, groups, src, src_counts, t0, out, out_counts);
  }
  launch_scene_window_ok(P.batch, P.max_dynamic, out_counts, ok, n_failed, st);
}

}  // namespace cilqr
