// cilqr_carry_rows / cilqr_carry_rows_batch (include/cilqr.h, "carry"): the host call around
// include/cilqr/trajectory_queries.hpp, and the host side of the batched one -- argument checks, staging of HOST arrays,
// the launch of kernels_carry.hip, the count's way back.
#include <cmath>

#include "../../include/cilqr/trajectory_queries.hpp"
#include "audit_batch.hpp"
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
  // ---- work space of the handle (grown, never shrunk): the count; HOST arrays: one block in, one block out
  block_layout l_tab, l_in, l_out;
  const slot s_count = l_tab.add(4);
  const slot s_rows = l_in.add(B * R * F * 8), s_adv = l_in.add(B * 8);
  const slot s_c9 = l_out.add(coarse9 ? B * K * CILQR_COARSE_FIELDS * 8 : 0), s_c6 = l_out.add(coarse6 ? B * K * 6 * 8 : 0);
  const slot s_k3 = l_out.add(knots3 ? B * K * 3 * 8 : 0), s_stn = l_out.add(station ? B * K * 8 : 0);
  const slot s_state = l_out.add(B * 4);
  HIP_TRY(h->cy_tab_host.grow(l_tab.bytes() + 256));
  HIP_TRY(h->cy_tab.grow(l_tab.bytes() + 256, &h->grown_bytes));
  const bool on_host = memory == CILQR_MEM_HOST;
  if (on_host) {
    HIP_TRY(h->cy_in.grow(l_in.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->cy_out.grow(l_out.bytes() + 256, &h->grown_bytes));
  }
  int* d_count = s_count.in<int>(h->cy_tab.as<char>());
  HIP_TRY(hipMemsetAsync(d_count, 0, 4, st));

  const double *d_rows = rows, *d_adv = advance;
  double *d_c9 = coarse9, *d_c6 = coarse6, *d_k3 = knots3, *d_stn = station;
  int* d_state = state;
  char* bo = h->cy_out.as<char>();
  if (on_host) {
    char* bi = h->cy_in.as<char>();
    if (int rc = copy_in(bi, s_rows, rows, st)) return rc;
    if (int rc = copy_in(bi, s_adv, advance, st)) return rc;
    d_rows = s_rows.in<const double>(bi);
    d_adv = s_adv.in<const double>(bi);
    if (coarse9) d_c9 = s_c9.in<double>(bo);
    if (coarse6) d_c6 = s_c6.in<double>(bo);
    if (knots3) d_k3 = s_k3.in<double>(bo);
    if (station) d_stn = s_stn.in<double>(bo);
    d_state = s_state.in<int>(bo);
  }
  launch_carry(P, d_rows, d_adv, d_c9, d_c6, d_k3, d_stn, d_state, d_count, st);
  HIP_TRY(hipGetLastError());
  if (on_host) {
    if (int rc = copy_out(coarse9, bo, s_c9, st)) return rc;
    if (int rc = copy_out(coarse6, bo, s_c6, st)) return rc;
    if (int rc = copy_out(knots3, bo, s_k3, st)) return rc;
    if (int rc = copy_out(station, bo, s_stn, st)) return rc;
    if (int rc = copy_out(state, bo, s_state, st)) return rc;
  }
  return wait_and_fetch_count(d_count, s_count.in<int>(h->cy_tab_host.as<char>()), st, n_kept);
}

extern "C" int cilqr_carry_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_rows,
                                      const double* advance, double max_advance, int32_t n_knots, double delta_t,
                                      double* coarse9, double* coarse6, double* knots3, double* station, int32_t* state,
                                      int32_t* n_kept, int32_t memory) {
  return carry_rows_batch_impl(h, batch, layout, rows, n_rows, advance, max_advance, n_knots, n_knots, delta_t, coarse9,
                               coarse6, knots3, station, state, n_kept, memory);
}
