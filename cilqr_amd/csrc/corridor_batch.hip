// cilqr_default_corridor_config, cilqr_build_corridors and cilqr_lane_constraints (include/cilqr.h): the host side of the
// corridor producer -- argument checks, staging of HOST arrays in blocks of the call's own, the launch of
// kernels_corridor.hip, the wait for it -- and the lane tables, which are host work altogether.
#include <cmath>

#include "staging.hpp"

using namespace cilqr;

extern "C" {

void cilqr_default_corridor_config(cilqr_corridor_config* c) {
  if (c == nullptr) return;
  c->max_diff_x = 25.0; c->max_diff_y = 25.0; c->radius = 150.0;   // planner_config.h:77-79
  c->max_axis_x = 10.0; c->max_axis_y = 10.0;                      // planner_config.h:81-82
  c->lane_segment_length = 5.0;                                    // planner_config.h:85
  c->is_multiple_sample = 0;                                       // planner_config.h:76
  c->reserved0 = 0;
}

int cilqr_build_corridors(cilqr_handle h, const cilqr_corridor_config* cfg, int32_t batch, int32_t n_knots,
                          const double* knots, const double* points, const int32_t* point_count,
                          int32_t max_points, double* corridor, int32_t* corridor_count, int32_t cmax,
                          int32_t memory, int32_t* n_failed, double* polygons) {
  if (h == nullptr || cfg == nullptr || knots == nullptr || point_count == nullptr || corridor == nullptr ||
      corridor_count == nullptr)
    return CILQR_ERR_NULL;                                          // corridor.cc:29-35
  if (points == nullptr && max_points > 0) return CILQR_ERR_NULL;
  if (batch <= 0 || n_knots <= 0 || cmax < 3 || max_points < 0) return CILQR_ERR_ARG;   // empty trajectory cc:24-27
  if (max_points + (cfg->is_multiple_sample ? 24 : 8) > kCorMaxPts) return CILQR_ERR_CAPACITY;
  if (memory != CILQR_MEM_HOST && memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t)batch * n_knots;
  CorridorParams cp{cfg->max_diff_x, cfg->max_diff_y, cfg->radius, cfg->max_axis_x, cfg->max_axis_y,
                    cfg->is_multiple_sample ? 6 : 2};
  if (h->cor_done.get() == nullptr) HIP_TRY(h->cor_done.create());
  if (n_failed) *n_failed = 0;   // what a call that fails from here on reports
  // (a producer beside solves in flight -- bench.py: end_to_end -- runs on the handle's own stream at normal priority: on a
  // low-priority stream the call took 25 ms instead of 16.5 and the pipeline lost 1.5 %, r06 log 7)
  hipStream_t cst = h->stream;
  // The failure count and its landing place on the host belong to the handle: a hipMalloc / hipFree per call is a
  // device-wide synchronisation, i.e. a producer that runs beside solves in flight (other handles, a pool) would wait for
  // all of them.  HOST arrays: one block in, one block out, both of this call alone.
  call_blocks own;
  staged_call c(h, h->cor, memory == CILQR_MEM_HOST, cst);
  c.io_blocks(own);
  const double *d_knots, *d_pts;
  const int* d_cnt;
  double *d_cor, *d_poly;
  int *d_ccnt, *t_fail;
  c.counter(&t_fail);
  c.in(knots, n * 3, &d_knots);
  c.in(points, n * max_points * 2, &d_pts);
  c.in(point_count, n, &d_cnt);
  c.out(corridor, n * cmax * 3, &d_cor);
  c.out(corridor_count, n, &d_ccnt);
  c.out(polygons, n * cmax * 2, &d_poly);
  if (int rc = c.stage()) return rc;
  launch_build_corridors((int)n, cp, d_knots, d_pts, d_cnt, max_points, d_cor, d_ccnt, cmax, t_fail, d_poly, cst);
  HIP_TRY(hipGetLastError());
  if (int rc = c.fetch()) return rc;
  // a large batch is milliseconds of kernel time: the caller's thread naps through it instead of spinning (it usually has
  // solves in flight whose worker threads want the cores); a small one is waited for the short way
  if (n >= (size_t)1 << 18) {
    HIP_TRY(hipEventRecord(h->cor_done.get(), cst));
    if (wait_event(h->cor_done.get(), true) != CILQR_OK) return CILQR_ERR_DEVICE;
  } else {
    HIP_TRY(hipStreamSynchronize(cst));
  }
  if (n_failed) *n_failed = c.count();
  return CILQR_OK;
}

int cilqr_lane_constraints(const double* boundary, int32_t n, double segment_length, int32_t is_left,
                           double* rows, int32_t max_rows) {
  if (boundary == nullptr || rows == nullptr) return CILQR_ERR_NULL;
  if (n < 1 || max_rows < 1) return CILQR_ERR_ARG;
  // LaneBoundarySample corridor.cc:298-311: keep a point once it is a segment length from the last kept one
  int m = 0;              // rows written
  double lx = boundary[0], ly = boundary[1];
  for (int i = 0; i < n; ++i) {
    const double x = boundary[2 * i], y = boundary[2 * i + 1];
    if (std::hypot(x - lx, y - ly) >= segment_length - 1e-10) {
      if (m >= max_rows) return CILQR_ERR_CAPACITY;
      // Cal{Left,Right}LaneConstraints cc:265-296: the left barrier runs from the new point back to
      // the previous one, the right barrier forward; HalfPlaneConstraint cc:313-321
      const double ax = is_left ? x : lx, ay = is_left ? y : ly;
      const double bx = is_left ? lx : x, by = is_left ? ly : y;
      const double a = by - ay, b = -(bx - ax);
      double* r = rows + 7 * (size_t)m;
      r[0] = a; r[1] = b; r[2] = a * ax + b * ay;
      r[3] = ax; r[4] = ay; r[5] = bx; r[6] = by;
      ++m;
      lx = x; ly = y;
    }
  }
  if (m < 1) return CILQR_ERR_CONSTRAINTS;   // fewer than two sampled points  cc:273-275
  return m;
}

}  // extern "C"
