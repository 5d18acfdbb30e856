// cilqr_track_rows / cilqr_track_rows_batch (include/cilqr.h, "track"): the host call around include/cilqr/tracker.hpp, and
// the host side of the batched one -- argument checks, the follow table in the handle's work space, staging of HOST arrays,
// the two launches of kernels_track.hip, the count's way back.
#include "../../include/cilqr/tracker.hpp"
#include "audit_batch.hpp"
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
  const bool on_host = memory == CILQR_MEM_HOST;
  // ---- work space of the handle (grown, never shrunk): the count and the follow table; HOST arrays: a block in, a block out
  block_layout l_tab, l_work, l_in, l_out;
  const slot s_count = l_tab.add(4);
  const slot s_table = l_work.add(follow_table_bytes(batch, n_knots));
  const slot s_rows = l_in.add(B * K * F * 8), s_start = l_in.add(start6 ? B * 6 * 8 : 0);
  const slot s_driven = l_out.add(B * D * CILQR_TRAJ_FIELDS * 8), s_ok = l_out.add(B * 4);
  HIP_TRY(h->tk_tab_host.grow(l_tab.bytes() + 256));
  HIP_TRY(h->tk_tab.grow(l_tab.bytes() + 256, &h->grown_bytes));
  HIP_TRY(h->tk_work.grow(l_work.bytes() + 256, &h->grown_bytes));
  if (on_host) {
    HIP_TRY(h->tk_in.grow(l_in.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->tk_out.grow(l_out.bytes() + 256, &h->grown_bytes));
  }
  int* d_count = s_count.in<int>(h->tk_tab.as<char>());
  HIP_TRY(hipMemsetAsync(d_count, 0, 4, st));

  const double *d_rows = rows, *d_start = start6;
  double* d_driven = driven;
  int* d_ok = ok;
  char* bo = h->tk_out.as<char>();
  if (on_host) {
    char* bi = h->tk_in.as<char>();
    if (int rc = copy_in(bi, s_rows, rows, st)) return rc;
    if (int rc = copy_in(bi, s_start, start6, st)) return rc;
    d_rows = s_rows.in<const double>(bi);
    if (start6) d_start = s_start.in<const double>(bi);
    d_driven = s_driven.in<double>(bo);
    d_ok = s_ok.in<int>(bo);
  }
  const FollowTable tab = follow_table_in(s_table.in<char>(h->tk_work.as<char>()), batch, n_knots);
  launch_track_gather(P, d_rows, d_start, tab, st);
  HIP_TRY(hipGetLastError());
  launch_track_rows(P, h->ds.p, h->tracker, tab, d_driven, d_ok, d_count, st);
  HIP_TRY(hipGetLastError());
  if (on_host) {
    if (int rc = copy_out(driven, bo, s_driven, st)) return rc;
    if (int rc = copy_out(ok, bo, s_ok, st)) return rc;
  }
  return wait_and_fetch_count(d_count, s_count.in<int>(h->tk_tab_host.as<char>()), st, n_failed);
}
