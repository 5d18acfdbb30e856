// cilqr_policy_gains_batch / cilqr_policy_rollout_batch (include/cilqr.h, "policy"): the host side -- argument checks, staging
// of HOST arrays, the stage chain of the gains call, the launches of kernels_policy.hip.
#include <cmath>
#include <cstring>

#include "policy.hpp"
#include "scene_batch.hpp"

using namespace cilqr;

namespace {

// the layouts that carry the states AND the controls: CILQR_ROWS_TRAJ, CILQR_ROWS_PLAN; fields = 0 for every other
RowColumns policy_columns(int32_t layout) {
  const RowColumns c = trajectory_columns(layout);
  return c.jerk >= 0 && c.rate >= 0 ? c : row_columns(-1);
}

}  // namespace

// The stage chain on rows where they lie: load, the rows as the current iterate, quadratize, backward, the three tensors as
// cilqr_stage_read writes them.  Every link is the stage call itself or the kernel behind it, so the bits are the chain's.
extern "C" int cilqr_policy_gains_batch(cilqr_handle h, const cilqr_problem_batch* in, int32_t layout, const double* rows,
                                        const double* lambda, double* Kfb, double* kff, double* dV, int32_t* ok) {
  if (h == nullptr || in == nullptr || rows == nullptr || Kfb == nullptr || kff == nullptr) return CILQR_ERR_NULL;
  const RowColumns cols = policy_columns(layout);
  if (cols.fields == 0) return CILQR_ERR_ARG;
  // the checks of a load: CILQR_ERR_STATE while solves are submitted, more than one lane group CILQR_ERR_ARG, n_knots,
  // capacities, the memory flag
  if (int rc = cilqr_stage_load(h, in)) return rc;

  hipStream_t st = h->stream;
  const DeviceState& d = h->ds;
  const int B = in->batch, N = h->cfg.n_steps, K = N + 1;
  staged_call c(h, h->po, in->memory == CILQR_MEM_HOST, st);
  const double *d_rows, *d_lambda;
  double *d_K, *d_k, *d_dV;
  int32_t* d_ok;
  c.in(rows, (size_t)B * K * cols.fields, &d_rows);
  c.in(lambda, (size_t)B, &d_lambda);
  c.out(Kfb, (size_t)B * N * 12, &d_K);
  c.out(kff, (size_t)B * N * 2, &d_k);
  c.out(dV, (size_t)B * 2, &d_dV);
  c.out(ok, (size_t)B, &d_ok);
  if (int rc = c.stage()) return rc;
  launch_policy_set_rows(d, B, cols, d_rows, st);
  HIP_TRY(hipGetLastError());
  h->stage = 1 | 2;   // as cilqr_stage_set_trajectory leaves it (the stream is waited for by the stage calls below)
  if (int rc = cilqr_stage_quadratize(h)) return rc;
  if (int rc = cilqr_stage_backward(h, d_lambda, CILQR_MEM_DEVICE)) return rc;
  launch_expand(d, B, CILQR_T_KFB, d_K, st);
  launch_expand(d, B, CILQR_T_KFF, d_k, st);
  if (d_dV != nullptr) launch_gather_scalar(d.dV, 2, d.Bcap, B, d_dV, 2, 0, st);
  launch_policy_mask(d, B, d_K, d_k, d_dV, d_ok, st);
  HIP_TRY(hipGetLastError());
  return c.finish();
}

extern "C" int cilqr_policy_rollout_batch(cilqr_handle h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                                          const double* Kfb, const double* kff, double alpha, int32_t n_samples,
                                          const double* start6, int32_t clamp, int32_t n_out, double* out_rows,
                                          double* max_dev, double* end_dev, int32_t* n_clamped, int32_t memory) {
  if (h == nullptr || rows == nullptr || Kfb == nullptr || start6 == nullptr) return CILQR_ERR_NULL;
  if (out_rows == nullptr && max_dev == nullptr && end_dev == nullptr && n_clamped == nullptr) return CILQR_ERR_NULL;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  const RowColumns cols = policy_columns(layout);
  if (cols.fields == 0) return CILQR_ERR_ARG;
  if (batch < 1 || n_knots < 2 || n_out < 1 || n_out > n_knots) return CILQR_ERR_ARG;
  if (n_samples < 1 || n_samples > CILQR_POLICY_MAX_SAMPLES) return CILQR_ERR_ARG;
  if (kff != nullptr && !std::isfinite(alpha)) return CILQR_ERR_ARG;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  PolicyParams P;
  std::memset(&P, 0, sizeof(P));
  P.dyn = DynP{h->ds.p.dt, h->ds.p.wheel_base, h->ds.p.inv_wheel_base};
  P.jerk_min = h->ds.p.jerk_min; P.jerk_max = h->ds.p.jerk_max;
  P.rate_min = h->ds.p.delta_rate_min; P.rate_max = h->ds.p.delta_rate_max;
  P.alpha = kff != nullptr ? alpha : 0.0;
  P.batch = batch; P.n_knots = n_knots; P.n_samples = n_samples; P.n_out = n_out;
  P.clamp = clamp != 0; P.has_kff = kff != nullptr;
  P.cols = cols;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)batch, K = (size_t)n_knots, N = K - 1, S = (size_t)n_samples;
  staged_call c(h, h->po, memory == CILQR_MEM_HOST, st);
  const double *d_rows, *d_K, *d_k, *d_start;
  double *d_out, *d_max, *d_end;
  int32_t* d_clamped;
  c.in(rows, B * K * cols.fields, &d_rows);
  c.in(Kfb, B * N * 12, &d_K);
  c.in(kff, B * N * 2, &d_k);
  c.in(start6, S * B * 6, &d_start);
  c.out(out_rows, S * B * (size_t)n_out * CILQR_TRAJ_FIELDS, &d_out);
  c.out(max_dev, S * B, &d_max);
  c.out(end_dev, S * B, &d_end);
  c.out(n_clamped, S * B, &d_clamped);
  if (int rc = c.stage()) return rc;
  launch_policy_rollout(P, d_rows, d_K, d_k, d_start, d_out, d_max, d_end, d_clamped, st);
  HIP_TRY(hipGetLastError());
  return c.finish();
}
