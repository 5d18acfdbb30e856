// cilqr_predict_scenes_batch (include/cilqr.h, "scene prediction"): the host side -- argument checks, staging of HOST
// arrays, the launch of kernels_scene_predict.hip, the count's way back.
#include <climits>
#include <cmath>

#include "scene_batch.hpp"
#include "scene_predict.hpp"

using namespace cilqr;

extern "C" int cilqr_predict_scenes_batch(cilqr_handle h, const cilqr_scene_batch* scenes, const double* t0, double span,
                                          int32_t mode, double max_age, double sample_dt, int32_t out_samples,
                                          double* trajectories, int32_t* counts, int32_t* ok, int32_t* n_refused) {
  if (h == nullptr || scenes == nullptr || t0 == nullptr) return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (int rc = check_scene_batch(sb)) return rc;
  if (sb.max_dynamic > 0 && (trajectories == nullptr || counts == nullptr)) return CILQR_ERR_NULL;
  if (int rc = check_prediction(span, mode, max_age, sample_dt, out_samples)) return rc;
  // the source may be as long as it likes, as in cilqr_window_scenes_batch; the prediction is what the scene kernels read next
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

  ScenePredictParams P;
  P.batch = sb.batch; P.max_dynamic = sb.max_dynamic; P.max_samples = sb.max_samples; P.out_samples = out_samples;
  P.mode = mode; P.max_age = max_age; P.sample_dt = sample_dt;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  // ---- the count and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  staged_call c(h, h->pr, on_host, st);
  const double *d_src, *d_t0;
  const int* d_scnt;
  double* d_out;
  int *d_ocnt, *d_ok, *d_count;
  c.counter(&d_count);
  c.in(sb.dynamic_trajectories, B * D * sb.max_samples * 4, &d_src);
  c.in(sb.dynamic_trajectory_counts, B * D, &d_scnt);
  c.in(t0, B, &d_t0);
  c.inout(trajectories, B * D * out_samples * 4, &d_out);   // the rows of a slot with count 0 or -1 stay as they are
  c.out(counts, B * D, &d_ocnt);
  c.out(ok, B, &d_ok);
  if (int rc = c.stage()) return rc;
  launch_scene_predict(P, d_src, d_scnt, d_t0, d_out, d_ocnt, d_ok, d_count, st);
  HIP_TRY(hipGetLastError());
  return c.finish(n_refused);
}
