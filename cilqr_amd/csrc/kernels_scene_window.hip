// cilqr_window_scenes_batch (include/cilqr.h, "scene window"): the samples a scene that starts at its own t0 needs of every
// dynamic obstacle's trajectory, cut out of long recordings where they lie in HBM and put on the clock 0 ... span.  The host
// statement is include/cilqr/scene_window.hpp; this file follows it operation by operation (-ffp-contract=off; the only
// arithmetic is time - t0 and span + 1e-9), so the windows are its bits.
//
// One wavefront per (scene, dynamic slot); the four wavefronts of a workgroup take neighbouring slots of one scene, whose
// source counts and t0 they read from the same lines.  A window is a few dozen samples out of thousands: what decides the
// kernel is how the two borders are found, not the copy.
//   search  the rule's halving is a chain of log2 T dependent loads (17 for 10^5 samples), each a trip to HBM.  Here the
//           wave searches together (wave_search.hpp: sw_wave_first): three rounds for 10^5 samples, two for the 1501 of a
//           15 s recording.  On non-decreasing times both predicates are monotone, and the first index that holds is what
//           the halving returns as well.
//   copy    one sample (32 bytes) per lane and step: a wave moves 2 KiB of contiguous source.  16-byte accesses where both
//           base pointers are 16-byte aligned (a slot's offset is a multiple of 32 bytes), 8-byte accesses otherwise.
// Every index that is probed or copied lies in [0, T) with T <= max_samples checked first, on any input.  No atomics here;
// k_scene_window_ok folds a scene's counts into its flag, one lane per scene, and adds the failed scenes up (one atomic
// per wave that saw one).
#include "dev_model.hpp"
#include "scene_window.hpp"
#include "wave_search.hpp"

namespace cilqr {

constexpr int kSwWaves = 4;   // slots of one scene per workgroup
constexpr int kSwLanes = kSwWave * kSwWaves;
constexpr double kSwMargin = 1e-9;   // scene_window.hpp: kMargin

__global__ __launch_bounds__(kSwLanes) void k_scene_window(SceneWindowParams P, int groups, const double* __restrict__ src,
                                                           const int* __restrict__ src_counts, const double* __restrict__ t0,
                                                           double* __restrict__ out, int* __restrict__ out_counts) {
  const int lane = threadIdx.x & (kSwWave - 1), wave = threadIdx.x >> 6;
  const int D = P.max_dynamic;
  const int b = (int)(blockIdx.x / (unsigned)groups);
  const int d = (int)(blockIdx.x - (unsigned)b * (unsigned)groups) * kSwWaves + wave;
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
  // ---- the two borders
  const double* __restrict__ tr = src + slot * (size_t)P.max_samples * 4;
  const double upper = P.span + kSwMargin;
  const int L = sw_wave_first(T, lane, [&](int k) { return !(tr[(size_t)k * 4] - t0b < -kSwMargin); });
  const int H = sw_wave_first(T, lane, [&](int k) { return upper < tr[(size_t)k * 4] - t0b; });
  const int lo = L - 1 > 0 ? L - 1 : 0;
  const int hi = H < T - 1 ? H : T - 1;
  const int count = hi - lo + 1;
  if (count > P.out_samples || count < 1) {   // count < 1: times that decrease can do that to the wave search; refused too
    if (lane == 0) out_counts[slot] = -1;
    return;
  }
  if (lane == 0) out_counts[slot] = count;
  // ---- the copy: samples lo ... hi, the time column on the scene's clock
  const double* __restrict__ s = tr + (size_t)lo * 4;
  double* __restrict__ o = out + slot * (size_t)P.out_samples * 4;
  const bool wide = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (wide) {
    for (int j = lane; j < count; j += kSwWave) {
      double2 v0 = *reinterpret_cast<const double2*>(s + (size_t)j * 4);
      const double2 v1 = *reinterpret_cast<const double2*>(s + (size_t)j * 4 + 2);
      v0.x = v0.x - t0b;
      *reinterpret_cast<double2*>(o + (size_t)j * 4) = v0;
      *reinterpret_cast<double2*>(o + (size_t)j * 4 + 2) = v1;
    }
  } else {
    for (int j = lane; j < count; j += kSwWave) {
      const double* sj = s + (size_t)j * 4;
      double* oj = o + (size_t)j * 4;
      const double t = sj[0], x = sj[1], y = sj[2], th = sj[3];
      oj[0] = t - t0b;
      oj[1] = x;
      oj[2] = y;
      oj[3] = th;
    }
  }
}

// ok[b] = no window count of scene b is negative; *n_failed += the scenes where one is
__global__ __launch_bounds__(kSwLanes) void k_scene_window_ok(int B, int D, const int* __restrict__ out_counts,
                                                              int* __restrict__ ok, int* __restrict__ n_failed) {
  const long long b = (long long)blockIdx.x * kSwLanes + threadIdx.x;
  bool fail = false;
  if (b < B) {
    for (int d = 0; d < D; ++d) fail = fail || out_counts[(size_t)b * D + d] < 0;
    if (ok != nullptr) ok[b] = fail ? 0 : 1;
  }
  const unsigned long long failed = __ballot(fail);
  if ((threadIdx.x & (kSwWave - 1)) == 0 && failed != 0ull) atomicAdd(n_failed, __popcll(failed));
}

void launch_scene_window(const SceneWindowParams& P, const double* src, const int* src_counts, const double* t0, double* out,
                         int* out_counts, int* ok, int* n_failed, hipStream_t st) {
  if (P.max_dynamic > 0) {
    const int groups = (P.max_dynamic + kSwWaves - 1) / kSwWaves;
    const dim3 grid((unsigned)((long long)P.batch * groups));   // the host has checked that this fits
    hipLaunchKernelGGL(k_scene_window, grid, dim3(kSwLanes), 0, st, P, groups, src, src_counts, t0, out, out_counts);
  }
  launch_scene_window_ok(P.batch, P.max_dynamic, out_counts, ok, n_failed, st);
}

void launch_scene_window_ok(int batch, int max_dynamic, const int* out_counts, int* ok, int* n_failed, hipStream_t st) {
  const dim3 grid_ok((unsigned)(((long long)batch + kSwLanes - 1) / kSwLanes));
  hipLaunchKernelGGL(k_scene_window_ok, grid_ok, dim3(kSwLanes), 0, st, batch, max_dynamic, out_counts, ok, n_failed);
}

}  // namespace cilqr
