// cilqr_clearance_rows_batch (include/cilqr.h, "clearance"): the host side -- argument checks, the vehicle's discs by
// DpEnvironment's own arithmetic (so that they are the host call's bits), staging of HOST arrays, the launch of
// kernels_clearance.hip, the count's way back.
#include <cmath>
#include <cstring>

#include "audit_batch.hpp"
#include "clearance.hpp"

using namespace cilqr;

extern "C" int cilqr_clearance_rows_batch(cilqr_handle h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes,
                                          int32_t layout, const double* rows, int32_t n_knots, double* clearance,
                                          int32_t* nearest, double* min_clearance, int32_t* min_knot, double threshold,
                                          int32_t* n_below) {
  if (h == nullptr || cfg == nullptr || scenes == nullptr || rows == nullptr || min_clearance == nullptr ||
      min_knot == nullptr || scenes->center == nullptr)
    return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (int rc = check_audit_batch(sb, layout, n_knots, 0.0)) return rc;
  if (n_below != nullptr && !std::isfinite(threshold)) return CILQR_ERR_ARG;
  if (int rc = check_audit_admissible(h, sb, n_knots)) return rc;
  const bool on_host = sb.memory == CILQR_MEM_HOST;

  const DpEnvironment::Discs discs = DpEnvironment::DiscsOf(dp_config_of(*cfg));
  ClearanceParams P;
  std::memset(&P, 0, sizeof(P));
  P.radius = discs.radius; P.r2x = discs.rear_x; P.f2x = discs.front_x;
  P.threshold = threshold;
  P.n_knots = n_knots;
  scene_limits_into(&P, sb);
  P.rows = pose_columns(layout);

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots;
  // ---- the count and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  staged_call c(h, h->cl, on_host, st);
  cilqr_scene_batch dv;
  const double* d_rows;
  double *d_clear, *d_min;
  int *d_near, *d_knot, *d_count;
  c.counter(&d_count);
  c.in(rows, B * K * P.rows.fields, &d_rows);
  c.scenes(sb, &dv);
  c.out(clearance, B * K * CILQR_CLEARANCE_FIELDS, &d_clear);
  c.out(nearest, B * K * CILQR_CLEARANCE_FIELDS, &d_near);
  c.out(min_clearance, B, &d_min);
  c.out(min_knot, B, &d_knot);
  if (int rc = c.stage()) return rc;
  launch_clearance(P, dv, d_rows, d_clear, d_near, d_min, d_knot, d_count, st);
  HIP_TRY(hipGetLastError());
  return c.finish(n_below);
}
