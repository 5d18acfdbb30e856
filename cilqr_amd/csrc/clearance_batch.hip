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
  P.rows = row_layout(layout);

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots;
  // ---- work space of the handle (grown, never shrunk): the count; HOST arrays: one block in, one block out
  block_layout l_tab, l_out;
  const slot s_count = l_tab.add(4);
  const AuditInput in(sb, n_knots, P.rows);
  const slot s_clear = l_out.add(clearance ? B * K * CILQR_CLEARANCE_FIELDS * 8 : 0);
  const slot s_near = l_out.add(nearest ? B * K * CILQR_CLEARANCE_FIELDS * 4 : 0);
  const slot s_min = l_out.add(B * 8), s_knot = l_out.add(B * 4);
  HIP_TRY(h->cl_tab_host.grow(l_tab.bytes() + 256));
  HIP_TRY(h->cl_tab.grow(l_tab.bytes() + 256, &h->grown_bytes));
  if (on_host) {
    HIP_TRY(h->cl_in.grow(in.l.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->cl_out.grow(l_out.bytes() + 256, &h->grown_bytes));
  }
  int* d_count = s_count.in<int>(h->cl_tab.as<char>());
  HIP_TRY(hipMemsetAsync(d_count, 0, 4, st));

  cilqr_scene_batch dv = sb;
  const double* d_rows = rows;
  double *d_clear = clearance, *d_min = min_clearance;
  int *d_near = nearest, *d_knot = min_knot;
  char* bo = h->cl_out.as<char>();
  if (on_host) {
    if (int rc = in.upload(sb, rows, h->cl_in.as<char>(), st, &d_rows, &dv)) return rc;
    if (clearance) d_clear = s_clear.in<double>(bo);
    if (nearest) d_near = s_near.in<int>(bo);
    d_min = s_min.in<double>(bo);
    d_knot = s_knot.in<int>(bo);
  }
  launch_clearance(P, dv, d_rows, d_clear, d_near, d_min, d_knot, d_count, st);
  HIP_TRY(hipGetLastError());
  if (on_host) {
    if (int rc = copy_out(clearance, bo, s_clear, st)) return rc;
    if (int rc = copy_out(nearest, bo, s_near, st)) return rc;
    if (int rc = copy_out(min_clearance, bo, s_min, st)) return rc;
    if (int rc = copy_out(min_knot, bo, s_knot, st)) return rc;
  }
  return wait_and_fetch_count(d_count, s_count.in<int>(h->cl_tab_host.as<char>()), st, n_below);
}
