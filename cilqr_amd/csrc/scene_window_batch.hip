// cilqr_window_scenes_batch (include/cilqr.h, "scene window"): the host side -- argument checks, staging of HOST arrays,
// the launch of kernels_scene_window.hip, the count's way back.
#include <climits>
#include <cmath>

#include "scene_batch.hpp"
#include "scene_window.hpp"

using namespace cilqr;

extern "C" int cilqr_window_scenes_batch(cilqr_handle h, const cilqr_scene_batch* scenes, const double* t0, double span,
                                         int32_t out_samples, double* trajectories, int32_t* counts, int32_t* ok,
                                         int32_t* n_overflow) {
  if (h == nullptr || scenes == nullptr || t0 == nullptr) return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (int rc = check_scene_batch(sb)) return rc;
  if (sb.max_dynamic > 0 && (trajectories == nullptr || counts == nullptr)) return CILQR_ERR_NULL;
  if (!std::isfinite(span) || span < 0.0 || out_samples < 1) return CILQR_ERR_ARG;
  // the source may be as long as it likes (max_samples is not held to CILQR_DP_MAX_SAMPLES here); the window is what the
  // scene kernels read next
  const int groups = (sb.max_dynamic + 3) / 4;
  if (out_samples > CILQR_DP_MAX_SAMPLES || (long long)sb.batch * (groups > 0 ? groups : 1) > INT_MAX) return CILQR_ERR_CAPACITY;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;
  const bool on_host = sb.memory == CILQR_MEM_HOST;
  const size_t B = (size_t)sb.batch, D = (size_t)sb.max_dynamic;
  if (on_host) {
    for (size_t i = 0; i < B * D; ++i)
      if (sb.dynamic_trajectory_counts[i] < 0 || sb.dynamic_trajectory_counts[i] > sb.max_samples) return CILQR_ERR_ARG;
    for (size_t b = 0; b < B; ++b)
      if (!std::isfinite(t0[b])) return CILQR_ERR_ARG;
  }

  SceneWindowParams P;
  P.batch = sb.batch; P.max_dynamic = sb.max_dynamic; P.max_samples = sb.max_samples; P.out_samples = out_samples;
  P.span = span;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  // ---- the count and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  staged_call c(h, h->sw, on_host, st);
  const double *d_src, *d_t0;
  const int* d_scnt;
  double* d_win;
  int *d_wcnt, *d_ok, *d_count;
  c.counter(&d_count);
  c.in(sb.dynamic_trajectories, B * D * sb.max_samples * 4, &d_src);
  c.in(sb.dynamic_trajectory_counts, B * D, &d_scnt);
  c.in(t0, B, &d_t0);
  c.inout(trajectories, B * D * out_samples * 4, &d_win);   // what lies behind a count stays as it is
  c.out(counts, B * D, &d_wcnt);
  c.out(ok, B, &d_ok);
  if (int rc = c.stage()) return rc;
  launch_scene_window(P, d_src, d_scnt, d_t0, d_win, d_wcnt, d_ok, d_count, st);
  HIP_TRY(hipGetLastError());
  return c.finish(n_overflow);
}
