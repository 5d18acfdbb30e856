// cilqr_track_rows / cilqr_track_rows_batch (include/cilqr.h, "track"): the host call around include/cilqr/tracker.hpp, and
// the host side of the batched one -- argument checks, the follow table in the handle's work space, staging of HOST arrays,
// the two launches of kernels_track.hip, the count's way back.
#include "../../include/cilqr/tracker.hpp"
#include "scene_batch.hpp"
#include "track.hpp"

using namespace cilqr;
namespace tk = cilqr::tracker;

namespace {

// what both calls check about one trajectory's shape
int check_track_arguments(int32_t layout, int32_t n_knots, int32_t n_drive) {
  if (tk::follow_columns(layout).fields == 0) return CILQR_ERR_ARG;   // CILQR_ROWS_POINTS and CILQR_ROWS_CONTROLS included
  if (n_knots < 2 || n_drive < 1 || n_drive > n_knots) return CILQR_ERR_ARG;
  return CILQR_OK;
}

}  // namespace

extern "C" int cilqr_track_rows(const cilqr_config* cfg, const cilqr_tracker_config* tcfg, int32_t layout, const double* rows,
                                int32_t n_knots, const double* start6, int32_t n_drive, double* driven) {
  if (cfg == nullptr || tcfg == nullptr || rows == nullptr || driven == nullptr) return CILQR_ERR_NULL;
  if (int rc = check_track_arguments(layout, n_knots, n_drive)) return rc;
  tk::Config c;
  c.weight_l = tcfg->weight_l; c.weight_theta = tcfg->weight_theta; c.weight_delta = tcfg->weight_delta;
  c.weight_delta_rate = tcfg->weight_delta_rate; c.preview_time = tcfg->preview_time;
  c.weight_s = tcfg->weight_s; c.weight_v = tcfg->weight_v; c.weight_a = tcfg->weight_a; c.weight_j = tcfg->weight_j;
  c.sumulation_dt = tcfg->sumulation_dt; c.dt = tcfg->dt; c.tolerance = tcfg->tolerance;
  c.max_num_iteration = tcfg->max_num_iteration;
  if (!tk::config_valid(c, CILQR_TRACKER_MAX_ITERATIONS)) return CILQR_ERR_ARG;
  tk::Vehicle v;
  v.wheel_base = cfg->wheel_base;
  v.delta_min = cfg->delta_min; v.delta_max = cfg->delta_max;
  v.delta_rate_min = cfg->delta_rate_min; v.delta_rate_max = cfg->delta_rate_max;
  v.jerk_min = cfg->jerk_min; v.jerk_max = cfg->jerk_max;
  v.min_acceleration = cfg->min_acceleration; v.max_acceleration = cfg->max_acceleration;
  return tk::track_rows(c, v, layout, rows, n_knots, start6, n_drive, driven, CILQR_TRACKER_MAX_SIM_STEPS) ? CILQR_OK
                                                                                                           : CILQR_ERR_STATE;
}

extern "C" int cilqr_track_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                                      const double* start6, int32_t n_drive, double* driven, int32_t* ok, int32_t* n_failed,
                                      int32_t memory) {
  if (h == nullptr || rows == nullptr || driven == nullptr || ok == nullptr) return CILQR_ERR_NULL;
  if (batch < 1) return CILQR_ERR_ARG;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if (int rc = check_track_arguments(layout, n_knots, n_drive)) return rc;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  TrackParams P;
  P.batch = batch; P.n_knots = n_knots; P.n_drive = n_drive;
  P.fields = tk::follow_columns(layout).fields;
  P.max_steps = CILQR_TRACKER_MAX_SIM_STEPS;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)batch, K = (size_t)n_knots, D = (size_t)n_drive, F = (size_t)P.fields;
  // ---- the count, the follow table and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  HIP_TRY(h->tk_work.grow(follow_table_bytes(batch, n_knots) + 256, &h->grown_bytes));
  staged_call c(h, h->tk, memory == CILQR_MEM_HOST, st);
  const double *d_rows, *d_start;
  double* d_driven;
  int *d_ok, *d_count;
  c.counter(&d_count);
  c.in(rows, B * K * F, &d_rows);
  c.in(start6, B * 6, &d_start);
  c.out(driven, B * D * CILQR_TRAJ_FIELDS, &d_driven);
  c.out(ok, B, &d_ok);
  if (int rc = c.stage()) return rc;
  const FollowTable tab = follow_table_in(h->tk_work.as<char>(), batch, n_knots);
  launch_track_gather(P, d_rows, d_start, tab, st);
  HIP_TRY(hipGetLastError());
  launch_track_rows(P, h->ds.p, h->tracker, tab, d_driven, d_ok, d_count, st);
  HIP_TRY(hipGetLastError());
  return c.finish(n_failed);
}
