// cilqr_frenet_rows / cilqr_cartesian_points and their batched forms (include/cilqr.h, "frenet"): the host calls around
// include/cilqr/trajectory_queries.hpp, and the host side of the batched ones -- argument checks, the centre line's tables
// on their way to the device, staging of HOST arrays, the launches of kernels_frenet.hip.
#include <vector>

#include "../../include/cilqr/trajectory_queries.hpp"
#include "frenet.hpp"
#include "scene_batch.hpp"

using namespace cilqr;
namespace tq = cilqr::trajectory_queries;

namespace {

// do [a, a + na) and [b, b + nb) share a byte?
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// the packed [n][2] x, y of the scan of a centre line [n][7]
std::vector<double> center_xy(const double* center, int32_t n_center) {
  std::vector<double> xy((size_t)n_center * 2);
  for (size_t i = 0; i < (size_t)n_center; ++i) {
    xy[2 * i] = center[i * tq::kCenterFields + 1];
    xy[2 * i + 1] = center[i * tq::kCenterFields + 2];
  }
  return xy;
}

}  // namespace

extern "C" int cilqr_frenet_rows(const double* center, int32_t n_center, int32_t layout, const double* rows, int32_t n_rows,
                                 double* frenet) {
  if (center == nullptr || rows == nullptr || frenet == nullptr) return CILQR_ERR_NULL;
  int fields = 0, xc = 0;
  if (n_center < 2 || n_rows < 1 || !tq::point_columns(layout, &fields, &xc)) return CILQR_ERR_ARG;
  const size_t out_bytes = (size_t)n_rows * tq::kFrenetFields * 8;
  if (overlap(frenet, out_bytes, rows, (size_t)n_rows * fields * 8) ||
      overlap(frenet, out_bytes, center, (size_t)n_center * tq::kCenterFields * 8))
    return CILQR_ERR_ARG;
  tq::project_rows(center, n_center, layout, rows, n_rows, frenet);
  return CILQR_OK;
}

extern "C" int cilqr_cartesian_points(const double* center, int32_t n_center, const double* sl, int32_t n, double* xyt) {
  if (center == nullptr || sl == nullptr || xyt == nullptr) return CILQR_ERR_NULL;
  if (n_center < 2 || n < 1) return CILQR_ERR_ARG;
  const size_t out_bytes = (size_t)n * 3 * 8;
  if (overlap(xyt, out_bytes, sl, (size_t)n * 2 * 8) || overlap(xyt, out_bytes, center, (size_t)n_center * tq::kCenterFields * 8))
    return CILQR_ERR_ARG;
  for (int32_t i = 0; i < n; ++i)
    tq::cartesian_point(center, n_center, sl[(size_t)i * 2], sl[(size_t)i * 2 + 1], xyt + (size_t)i * 3);
  return CILQR_OK;
}

extern "C" int cilqr_frenet_rows_batch(cilqr_handle h, const double* center, int32_t n_center, int32_t batch, int32_t layout,
                                       const double* rows, int32_t n_knots, double* frenet, int32_t memory) {
  if (h == nullptr || center == nullptr || rows == nullptr || frenet == nullptr) return CILQR_ERR_NULL;
  int fields = 0, xc = 0;
  if (n_center < 2 || batch < 1 || n_knots < 1 || !tq::point_columns(layout, &fields, &xc)) return CILQR_ERR_ARG;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  const size_t Q = (size_t)batch * (size_t)n_knots, F = (size_t)fields;
  const size_t in_bytes = Q * F * 8, out_bytes = Q * tq::kFrenetFields * 8;
  if (overlap(frenet, out_bytes, rows, in_bytes) || overlap(frenet, out_bytes, center, (size_t)n_center * tq::kCenterFields * 8))
    return CILQR_ERR_ARG;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  FrenetParams P;
  P.n_queries = Q; P.n_center = n_center; P.fields = fields;
  // the centre line's tables and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  const std::vector<double> xy = center_xy(center, n_center);
  staged_call c(h, h->fr, memory == CILQR_MEM_HOST, st);
  const double* d_rows;
  double* d_out;
  c.table(center, (size_t)n_center * tq::kCenterFields, &P.center);
  c.table(xy.data(), xy.size(), &P.xy);
  c.in(rows, Q * F, &d_rows);
  c.out(frenet, Q * tq::kFrenetFields, &d_out);
  if (int rc = c.stage()) return rc;
  launch_frenet(P, d_rows, d_out, st);
  HIP_TRY(hipGetLastError());
  return c.finish();
}

extern "C" int cilqr_cartesian_points_batch(cilqr_handle h, const double* center, int32_t n_center, int32_t n, const double* sl,
                                            double* xyt, int32_t memory) {
  if (h == nullptr || center == nullptr || sl == nullptr || xyt == nullptr) return CILQR_ERR_NULL;
  if (n_center < 2 || n < 1) return CILQR_ERR_ARG;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  const size_t in_bytes = (size_t)n * 2 * 8, out_bytes = (size_t)n * 3 * 8;
  if (overlap(xyt, out_bytes, sl, in_bytes) || overlap(xyt, out_bytes, center, (size_t)n_center * tq::kCenterFields * 8))
    return CILQR_ERR_ARG;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  staged_call c(h, h->fr, memory == CILQR_MEM_HOST, st);
  const double *d_center, *d_sl;
  double* d_out;
  c.table(center, (size_t)n_center * tq::kCenterFields, &d_center);
  c.in(sl, (size_t)n * 2, &d_sl);
  c.out(xyt, (size_t)n * 3, &d_out);
  if (int rc = c.stage()) return rc;
  launch_cartesian(d_center, n_center, n, d_sl, d_out, st);
  HIP_TRY(hipGetLastError());
  return c.finish();
}
