// cilqr_window_scenes_batch (include/cilqr.h, "scene window"): the host side -- argument checks, staging of HOST arrays,
// the launch of kernels_scene_window.hip, the count's way back.
#include <climits>
#include <cmath>

#include "audit_batch.hpp"
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
  // ---- work space of the handle (grown, never shrunk): the count; HOST arrays: a block in, a block out
  block_layout l_tab, l_in, l_out;
  const slot s_count = l_tab.add(4);
  const slot s_src = l_in.add(B * D * (size_t)sb.max_samples * 4 * 8), s_scnt = l_in.add(B * D * 4), s_t0 = l_in.add(B * 8);
  const slot s_win = l_out.add(B * D * (size_t)out_samples * 4 * 8), s_wcnt = l_out.add(B * D * 4), s_ok = l_out.add(B * 4);
  HIP_TRY(h->sw_tab_host.grow(l_tab.bytes() + 256));
  HIP_TRY(h->sw_tab.grow(l_tab.bytes() + 256, &h->grown_bytes));
  if (on_host) {
    HIP_TRY(h->sw_in.grow(l_in.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->sw_out.grow(l_out.bytes() + 256, &h->grown_bytes));
  }
  int* d_count = s_count.in<int>(h->sw_tab.as<char>());
  HIP_TRY(hipMemsetAsync(d_count, 0, 4, st));

  const double *d_src = sb.dynamic_trajectories, *d_t0 = t0;
  const int* d_scnt = sb.dynamic_trajectory_counts;
  double* d_win = trajectories;
  int *d_wcnt = counts, *d_ok = ok;
  char* bo = h->sw_out.as<char>();
  if (on_host) {   // the caller's windows go in as well: what lies behind a count stays as it is
    char* bi = h->sw_in.as<char>();
    if (int rc = copy_in(bi, s_src, sb.dynamic_trajectories, st)) return rc;
    if (int rc = copy_in(bi, s_scnt, sb.dynamic_trajectory_counts, st)) return rc;
    if (int rc = copy_in(bi, s_t0, t0, st)) return rc;
    if (int rc = copy_in(bo, s_win, trajectories, st)) return rc;
    d_src = s_src.in<const double>(bi);
    d_scnt = s_scnt.in<const int>(bi);
    d_t0 = s_t0.in<const double>(bi);
    d_win = s_win.in<double>(bo);
    d_wcnt = s_wcnt.in<int>(bo);
    d_ok = s_ok.in<int>(bo);
  }
  launch_scene_window(P, d_src, d_scnt, d_t0, d_win, d_wcnt, d_ok, d_count, st);
  HIP_TRY(hipGetLastError());
  if (on_host) {
    if (int rc = copy_out(trajectories, bo, s_win, st)) return rc;
    if (int rc = copy_out(counts, bo, s_wcnt, st)) return rc;
    if (int rc = copy_out(ok, bo, s_ok, st)) return rc;
  }
  return wait_and_fetch_count(d_count, s_count.in<int>(h->sw_tab_host.as<char>()), st, n_overflow);
}
