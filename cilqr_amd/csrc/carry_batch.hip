// cilqr_carry_rows / cilqr_carry_rows_batch (include/cilqr.h, "carry"): the host call around
// include/cilqr/trajectory_queries.hpp, and the host side of the batched one -- argument checks, staging of HOST arrays,
// the launch of kernels_carry.hip, the count's way back.
#include <cmath>

#include "../../include/cilqr/trajectory_queries.hpp"
#include "scene_batch.hpp"
#include "carry.hpp"

using namespace cilqr;
namespace tq = cilqr::trajectory_queries;

int cilqr::check_carry_arguments(int32_t layout, int32_t n_rows, double max_advance) {
  if (tq::columns_of(layout).fields == 0 || n_rows < 2) return CILQR_ERR_ARG;
  if (!std::isfinite(max_advance) || max_advance < 0.0) return CILQR_ERR_ARG;
  if (n_rows > CILQR_DP_MAX_KNOTS) return CILQR_ERR_CAPACITY;
  return CILQR_OK;
}

namespace {

// ... and about the knots asked for: what is wrong with a value before what is too large
int check_carry_call(int32_t layout, int32_t n_rows, double max_advance, int32_t n_knots, double delta_t) {
  if (n_knots < 1 || !(delta_t > 0.0)) return CILQR_ERR_ARG;
  if (int rc = check_carry_arguments(layout, n_rows, max_advance)) return rc;
  if (n_knots > CILQR_DP_MAX_KNOTS) return CILQR_ERR_CAPACITY;
  return CILQR_OK;
}

}  // namespace

extern "C" int cilqr_carry_rows(int32_t layout, const double* rows, int32_t n_rows, double advance, double max_advance,
                                int32_t n_knots, double delta_t, double* coarse9, double* coarse6, double* knots3,
                                double* station, int32_t* state) {
  if (rows == nullptr || state == nullptr) return CILQR_ERR_NULL;
  if (int rc = check_carry_call(layout, n_rows, max_advance, n_knots, delta_t)) return rc;
  *state = tq::carry_rows(layout, rows, n_rows, advance, max_advance, n_knots, delta_t, coarse9, coarse6, knots3, station);
  return CILQR_OK;
}

int cilqr::carry_rows_batch_impl(cilqr_solver* h, int32_t batch, int32_t layout, const double* rows, int32_t n_rows,
                                 const double* advance, double max_advance, int32_t n_knots, int32_t n_live, double delta_t,
                                 double* coarse9, double* coarse6, double* knots3, double* station, int32_t* state,
                                 int32_t* n_kept, int32_t memory) {
  if (h == nullptr || rows == nullptr || advance == nullptr || state == nullptr) return CILQR_ERR_NULL;
  if (batch < 1) return CILQR_ERR_ARG;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if (int rc = check_carry_call(layout, n_rows, max_advance, n_knots, delta_t)) return rc;
  if (n_live < 1 || n_live > n_knots) return CILQR_ERR_ARG;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  CarryParams P;
  P.batch = batch; P.n_rows = n_rows; P.fields = tq::columns_of(layout).fields;
  P.n_knots = n_knots; P.n_live = n_live; P.max_advance = max_advance; P.delta_t = delta_t;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)batch, R = (size_t)n_rows, K = (size_t)n_knots, F = (size_t)P.fields;
  // ---- the count and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  staged_call c(h, h->cy, memory == CILQR_MEM_HOST, st);
  const double *d_rows, *d_adv;
  double *d_c9, *d_c6, *d_k3, *d_stn;
  int *d_state, *d_count;
  c.counter(&d_count);
  c.in(rows, B * R * F, &d_rows);
  c.in(advance, B, &d_adv);
  c.out(coarse9, B * K * CILQR_COARSE_FIELDS, &d_c9);
  c.out(coarse6, B * K * 6, &d_c6);
  c.out(knots3, B * K * 3, &d_k3);
  c.out(station, B * K, &d_stn);
  c.out(state, B, &d_state);
  if (int rc = c.stage()) return rc;
  launch_carry(P, d_rows, d_adv, d_c9, d_c6, d_k3, d_stn, d_state, d_count, st);
  HIP_TRY(hipGetLastError());
  return c.finish(n_kept);
}

extern "C" int cilqr_carry_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_rows,
                                      const double* advance, double max_advance, int32_t n_knots, double delta_t,
                                      double* coarse9, double* coarse6, double* knots3, double* station, int32_t* state,
                                      int32_t* n_kept, int32_t memory) {
  return carry_rows_batch_impl(h, batch, layout, rows, n_rows, advance, max_advance, n_knots, n_knots, delta_t, coarse9,
                               coarse6, knots3, station, state, n_kept, memory);
}
