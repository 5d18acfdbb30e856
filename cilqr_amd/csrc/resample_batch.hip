// cilqr_resample_rows / cilqr_resample_rows_batch (include/cilqr.h, "resample"): the host call around
// include/cilqr/trajectory_queries.hpp, and the host side of the batched one -- argument checks, staging of HOST arrays,
// the launch of kernels_resample.hip.
#include "../../include/cilqr/trajectory_queries.hpp"
#include "resample.hpp"
#include "scene_batch.hpp"

using namespace cilqr;
namespace tq = cilqr::trajectory_queries;

namespace {

// what both calls check about one trajectory's shape
int check_resample_arguments(int32_t layout, int32_t n_knots, int32_t key, int32_t n_queries) {
  if (n_knots < 2 || n_queries < 1) return CILQR_ERR_ARG;
  if (tq::columns_of(layout).fields == 0) return CILQR_ERR_ARG;
  if (key != CILQR_KEY_TIME && key != CILQR_KEY_STATION) return CILQR_ERR_ARG;
  if (tq::key_column(layout, key) < 0) return CILQR_ERR_ARG;   // CILQR_ROWS_TRAJ has no station column
  if (n_knots > CILQR_DP_MAX_KNOTS) return CILQR_ERR_CAPACITY;
  return CILQR_OK;
}

}  // namespace

extern "C" int cilqr_resample_rows(int32_t layout, const double* rows, int32_t n_knots, int32_t key, const double* queries,
                                   int32_t n_queries, double* out) {
  if (rows == nullptr || queries == nullptr || out == nullptr) return CILQR_ERR_NULL;
  if (int rc = check_resample_arguments(layout, n_knots, key, n_queries)) return rc;
  if (out == rows) return CILQR_ERR_ARG;
  tq::resample_rows(layout, rows, n_knots, key, queries, n_queries, out);
  return CILQR_OK;
}

extern "C" int cilqr_resample_rows_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                                         int32_t key, const double* queries, int32_t n_queries, int32_t per_problem,
                                         double* out, int32_t memory) {
  if (h == nullptr || rows == nullptr || queries == nullptr || out == nullptr) return CILQR_ERR_NULL;
  if (batch < 1) return CILQR_ERR_ARG;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if (per_problem != 0 && per_problem != 1) return CILQR_ERR_ARG;
  if (out == rows) return CILQR_ERR_ARG;
  if (int rc = check_resample_arguments(layout, n_knots, key, n_queries)) return rc;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  ResampleParams P;
  P.batch = batch; P.n_knots = n_knots; P.n_queries = n_queries;
  P.fields = tq::columns_of(layout).fields;
  P.key_col = tq::key_column(layout, key);
  P.per_problem = per_problem;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)batch, K = (size_t)n_knots, M = (size_t)n_queries, F = (size_t)P.fields;
  // HOST arrays: a block in and a block out of the handle's work space (grown, never shrunk)
  staged_call c(h, h->rs, memory == CILQR_MEM_HOST, st);
  const double *d_rows, *d_queries;
  double* d_out;
  c.in(rows, B * K * F, &d_rows);
  c.in(queries, (per_problem ? B : 1) * M, &d_queries);
  c.out(out, B * M * F, &d_out);
  if (int rc = c.stage()) return rc;
  launch_resample(P, d_rows, d_queries, d_out, st);
  HIP_TRY(hipGetLastError());
  return c.finish();
}
