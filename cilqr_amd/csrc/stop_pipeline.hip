// cilqr_stop_scenes_batch (include/cilqr.h, "stop"): stop rows for every profile, the audit of every slice, the choice and
// the gather.  The first two steps are the body behind the public call (stop_rows_batch_impl) and the public entry point
// (cilqr_check_collisions_batch) on device views, so that what the pipeline computes is what a caller of those calls gets.
#include "../../include/cilqr/trajectory_queries.hpp"
#include "audit_batch.hpp"
#include "stop.hpp"

using namespace cilqr;

extern "C" int cilqr_stop_scenes_batch(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_scene_batch* scenes,
                                       int32_t layout, const double* rows, int32_t n_knots, int32_t n_profiles,
                                       const double* profiles, const double* start_va, double delta_t, int32_t n_out,
                                       double collision_buffer, double* out_rows, int32_t* choice, int32_t* status,
                                       int32_t* first_hit, int32_t* n_none) {
  if (h == nullptr || dp_cfg == nullptr || scenes == nullptr || rows == nullptr || profiles == nullptr ||
      out_rows == nullptr || choice == nullptr || scenes->center == nullptr)
    return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  // ---- the checks of both calls, before anything is launched
  if (int rc = check_scene_batch(sb)) return rc;
  if (int rc = check_stop_arguments(layout, n_knots, n_profiles, profiles, delta_t, n_out)) return rc;
  if (int rc = check_audit_arguments(CILQR_ROWS_PLAN, n_out, collision_buffer)) return rc;
  if (int rc = check_audit_admissible(h, sb, n_out)) return rc;
  const bool on_host = sb.memory == CILQR_MEM_HOST;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots, M = (size_t)n_profiles;
  const size_t F = (size_t)trajectory_queries::columns_of(layout).fields, per = (size_t)n_out * CILQR_PLAN_FIELDS;
  // ---- work space: the slices of all profiles, and their statuses and hits where the caller does not take them
  block_layout l;
  const slot s_slices = l.add(M * B * per * 8), s_status = l.add(M * B * 4), s_first = l.add(M * B * 4);
  HIP_TRY(h->ss_work.grow(l.bytes() + 256, &h->grown_bytes));
  char* w = h->ss_work.as<char>();
  double* d_slices = s_slices.in<double>(w);

  staged_call c(h, h->ss, on_host, st);
  cilqr_scene_batch dv;
  const double *d_rows, *d_va;
  double* d_out;
  int *d_choice, *d_status, *d_first, *d_count;
  c.counter(&d_count);
  c.in(rows, B * K * F, &d_rows);
  c.in(start_va, B * 2, &d_va);
  c.scenes(sb, &dv);
  c.out(out_rows, B * per, &d_out);
  c.out(choice, B, &d_choice);
  c.out(status, M * B, &d_status);
  c.out(first_hit, M * B, &d_first);
  if (int rc = c.stage()) return rc;
  if (d_status == nullptr) d_status = s_status.in<int>(w);
  if (d_first == nullptr) d_first = s_first.in<int>(w);

  // ---- 1. stop, 2. audit, 3. choose and 4. gather
  if (int rc = stop_rows_batch_impl(h, sb.batch, layout, d_rows, n_knots, n_profiles, profiles, d_va, delta_t, n_out, d_slices,
                                    d_status, nullptr, nullptr, CILQR_MEM_DEVICE))
    return rc;
  for (size_t m = 0; m < M; ++m)
    if (int rc = cilqr_check_collisions_batch(h, dp_cfg, &dv, CILQR_ROWS_PLAN, d_slices + m * B * per, n_out, collision_buffer,
                                              nullptr, d_first + m * B, nullptr, nullptr))
      return rc;
  launch_stop_choose((int)B, n_profiles, per, d_status, d_first, d_slices, d_choice, d_out, n_none ? d_count : nullptr, st);
  HIP_TRY(hipGetLastError());
  return c.finish(n_none);
}
