// cilqr_frenet_rows / cilqr_cartesian_points and their batched forms (include/cilqr.h, "frenet"): the host calls around
// include/cilqr/trajectory_queries.hpp, and the host side of the batched ones -- argument checks, the centre line's tables
// on their way to the device, staging of HOST arrays, the launches of kernels_frenet.hip.
#include <cstring>

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

// the centre line in the handle's table block: [n][7] as given and the packed [n][2] x, y of the scan
struct CenterTables {
  const double* center = nullptr;
  const double* xy = nullptr;
};
int upload_center(cilqr_handle h, const double* center, int32_t n_center, bool with_xy, hipStream_t st, CenterTables* out) {
  const size_t n = (size_t)n_center;
  block_layout l_tab;
  const slot s_center = l_tab.add(n * tq::kCenterFields * 8), s_xy = l_tab.add(with_xy ? n * 2 * 8 : 0);
  HIP_TRY(h->fr_tab_host.grow(l_tab.bytes() + 256));
  HIP_TRY(h->fr_tab.grow(l_tab.bytes() + 256, &h->grown_bytes));
  // pinned block -> device (the stream is waited for at the end of every call, so the block is free again)
  char* th = h->fr_tab_host.as<char>();
  char* td = h->fr_tab.as<char>();
  std::memcpy(th + s_center.off, center, s_center.bytes);
  if (with_xy) {
    double* xy = s_xy.in<double>(th);
    for (size_t i = 0; i < n; ++i) {
      xy[2 * i] = center[i * tq::kCenterFields + 1];
      xy[2 * i + 1] = center[i * tq::kCenterFields + 2];
    }
  }
  HIP_TRY(hipMemcpyAsync(td, th, l_tab.bytes(), hipMemcpyHostToDevice, st));
  out->center = s_center.in<const double>(td);
  out->xy = s_xy.in<const double>(td);
  return CILQR_OK;
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
  CenterTables tab;
  if (int rc = upload_center(h, center, n_center, true, st, &tab)) return rc;
  FrenetParams P;
  P.n_queries = Q; P.n_center = n_center; P.fields = fields;
  P.center = tab.center; P.xy = tab.xy;

  const double* d_rows = rows;
  double* d_out = frenet;
  const bool on_host = memory == CILQR_MEM_HOST;
  block_layout l_in, l_out;
  const slot s_rows = l_in.add(in_bytes), s_out = l_out.add(out_bytes);
  if (on_host) {   // work space of the handle (grown, never shrunk): one block in, one block out
    HIP_TRY(h->fr_in.grow(l_in.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->fr_out.grow(l_out.bytes() + 256, &h->grown_bytes));
    if (int rc = copy_in(h->fr_in.as<char>(), s_rows, rows, st)) return rc;
    d_rows = s_rows.in<const double>(h->fr_in.as<char>());
    d_out = s_out.in<double>(h->fr_out.as<char>());
  }
  launch_frenet(P, d_rows, d_out, st);
  HIP_TRY(hipGetLastError());
  if (on_host)
    if (int rc = copy_out(frenet, h->fr_out.as<char>(), s_out, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));   // this stream alone: solves on other handles go on
  return CILQR_OK;
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
  CenterTables tab;
  if (int rc = upload_center(h, center, n_center, false, st, &tab)) return rc;

  const double* d_sl = sl;
  double* d_out = xyt;
  const bool on_host = memory == CILQR_MEM_HOST;
  block_layout l_in, l_out;
  const slot s_sl = l_in.add(in_bytes), s_out = l_out.add(out_bytes);
  if (on_host) {
    HIP_TRY(h->fr_in.grow(l_in.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->fr_out.grow(l_out.bytes() + 256, &h->grown_bytes));
    if (int rc = copy_in(h->fr_in.as<char>(), s_sl, sl, st)) return rc;
    d_sl = s_sl.in<const double>(h->fr_in.as<char>());
    d_out = s_out.in<double>(h->fr_out.as<char>());
  }
  launch_cartesian(tab.center, n_center, n, d_sl, d_out, st);
  HIP_TRY(hipGetLastError());
  if (on_host)
    if (int rc = copy_out(xyt, h->fr_out.as<char>(), s_out, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return CILQR_OK;
}
