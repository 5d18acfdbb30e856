// cilqr_stop_rows / cilqr_stop_rows_batch (include/cilqr.h, "stop"): the host call around
// include/cilqr/trajectory_queries.hpp, and the host side of the batched one -- argument checks, staging of HOST arrays,
// the launch of kernels_stop.hip.
#include <cmath>

#include "../../include/cilqr/trajectory_queries.hpp"
#include "scene_batch.hpp"
#include "stop.hpp"

using namespace cilqr;
namespace tq = cilqr::trajectory_queries;

static_assert(tq::kStopStopped == CILQR_STOP_STOPPED && tq::kStopMoving == CILQR_STOP_MOVING &&
                  tq::kStopOverrun == CILQR_STOP_OVERRUN && tq::kStopRefused == CILQR_STOP_REFUSED,
              "the statuses of the statement are those of the header");

// what is wrong with a value before what is too large
int cilqr::check_stop_arguments(int32_t layout, int32_t n_knots, int32_t n_profiles, const double* profiles, double delta_t,
                                int32_t n_out) {
  if (tq::columns_of(layout).fields == 0 || n_knots < 2 || n_out < 1) return CILQR_ERR_ARG;
  if (n_profiles < 1 || n_profiles > CILQR_STOP_MAX_PROFILES || !(delta_t > 0.0)) return CILQR_ERR_ARG;
  for (int m = 0; m < n_profiles; ++m) {
    const double a_target = profiles[2 * m], jerk = profiles[2 * m + 1];
    if (!std::isfinite(a_target) || !std::isfinite(jerk) || !(a_target <= 0.0) || !(jerk < 0.0)) return CILQR_ERR_ARG;
  }
  if (n_knots > CILQR_DP_MAX_KNOTS || n_out > CILQR_DP_MAX_KNOTS) return CILQR_ERR_CAPACITY;
  return CILQR_OK;
}

extern "C" int cilqr_stop_rows(int32_t layout, const double* rows, int32_t n_knots, int32_t n_profiles, const double* profiles,
                               const double* start_va, double delta_t, int32_t n_out, double* out_rows, int32_t* status,
                               int32_t* stop_knot, double* travel) {
  if (rows == nullptr || profiles == nullptr) return CILQR_ERR_NULL;
  if (out_rows == nullptr && status == nullptr && stop_knot == nullptr && travel == nullptr) return CILQR_ERR_ARG;
  if (int rc = check_stop_arguments(layout, n_knots, n_profiles, profiles, delta_t, n_out)) return rc;
  for (int m = 0; m < n_profiles; ++m) {
    const int st = tq::stop_rows(layout, rows, n_knots, profiles[2 * m], profiles[2 * m + 1], start_va, delta_t, n_out,
                                 out_rows ? out_rows + (size_t)m * n_out * CILQR_PLAN_FIELDS : nullptr,
                                 stop_knot ? stop_knot + m : nullptr, travel ? travel + m : nullptr);
    if (status) status[m] = st;
  }
  return CILQR_OK;
}

int cilqr::stop_rows_batch_impl(cilqr_solver* h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                                int32_t n_profiles, const double* profiles, const double* start_va, double delta_t,
                                int32_t n_out, double* out_rows, int32_t* status, int32_t* stop_knot, double* travel,
                                int32_t memory) {
  if (h == nullptr || rows == nullptr || profiles == nullptr) return CILQR_ERR_NULL;
  if (batch < 1) return CILQR_ERR_ARG;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if (out_rows == nullptr && status == nullptr && stop_knot == nullptr && travel == nullptr) return CILQR_ERR_ARG;
  if (int rc = check_stop_arguments(layout, n_knots, n_profiles, profiles, delta_t, n_out)) return rc;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  StopParams P;
  P.batch = batch; P.n_knots = n_knots; P.fields = tq::columns_of(layout).fields;
  P.n_profiles = n_profiles; P.n_out = n_out; P.delta_t = delta_t;
  for (int m = 0; m < CILQR_STOP_MAX_PROFILES; ++m) {   // the profiles travel with the launch
    P.profile[m][0] = m < n_profiles ? profiles[2 * m] : 0.0;
    P.profile[m][1] = m < n_profiles ? profiles[2 * m + 1] : 0.0;
  }

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)batch, K = (size_t)n_knots, F = (size_t)P.fields, M = (size_t)n_profiles, N = (size_t)n_out;
  // ---- HOST arrays: a block in and a block out, the handle's work space (grown, never shrunk)
  staged_call c(h, h->sr, memory == CILQR_MEM_HOST, st);
  const double *d_rows, *d_va;
  double *d_out, *d_travel;
  int *d_status, *d_knot;
  c.in(rows, B * K * F, &d_rows);
  c.in(start_va, B * 2, &d_va);
  c.out(out_rows, M * B * N * CILQR_PLAN_FIELDS, &d_out);
  c.out(status, M * B, &d_status);
  c.out(stop_knot, M * B, &d_knot);
  c.out(travel, M * B, &d_travel);
  if (int rc = c.stage()) return rc;
  launch_stop(P, d_rows, d_va, d_out, d_status, d_knot, d_travel, st);
  HIP_TRY(hipGetLastError());
  return c.finish();
}

extern "C" int cilqr_stop_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                                     int32_t n_profiles, const double* profiles, const double* start_va, double delta_t,
                                     int32_t n_out, double* out_rows, int32_t* status, int32_t* stop_knot, double* travel,
                                     int32_t memory) {
  return stop_rows_batch_impl(h, batch, layout, rows, n_knots, n_profiles, profiles, start_va, delta_t, n_out, out_rows,
                              status, stop_knot, travel, memory);
}
