// cilqr_dp_plan_batch (include/cilqr.h): the host side of the batched DP coarse planner -- argument checks, the tables a
// call shares between its scenes (built by the host planner's own classes, include/cilqr/dp_planner.hpp, so that they
// are its bits), the handle's work space, the launches of kernels_dp.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "dp_core.hpp"
#include "scene_batch.hpp"

using cilqr::DpParams;

// the placed dynamic polygons of the scenes in flight: the batch is planned in chunks of as many scenes as fit
constexpr size_t kPlacedBytesCap = (size_t)1 << 30;

extern "C" int cilqr_dp_plan_batch(cilqr_handle h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes,
                                   const double* start3, int32_t n_knots, double* coarse9, double* coarse6,
                                   double* knots3, double* station, int32_t* found, int32_t* n_not_found) {
  return cilqr_dp_plan_batch_impl(h, cfg, scenes, start3, n_knots, coarse9, coarse6, knots3, station, found, n_not_found,
                                  nullptr);
}

int cilqr_dp_path_samples(const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes, int32_t n_knots, int32_t* n_samples) {
  if (!(cfg->delta_t > 0.0) || !(cfg->tf > 0.0)) return CILQR_ERR_ARG;
  if ((int32_t)(cfg->tf / cfg->delta_t + 1) != n_knots) return CILQR_ERR_KNOTS;
  const cilqr::DpConfig d = cilqr::dp_config_of(*cfg);
  const cilqr::DpEnvironment env(d, cilqr::reference_line_of(scenes->center, scenes->n_center));
  const cilqr::DpPlanner dp(d, &env);
  int nq = 0;
  for (int t = 0; t < cilqr::kDpNT; ++t) {
    if (dp.segment_points(t) < 1) return CILQR_ERR_KNOTS;
    nq += dp.segment_points(t);
  }
  if (nq > CILQR_DP_MAX_KNOTS) return CILQR_ERR_CAPACITY;
  *n_samples = nq;
  return CILQR_OK;
}

int cilqr_dp_plan_batch_impl(cilqr_solver* h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes, const double* start3,
                             int32_t n_knots, double* coarse9, double* coarse6, double* knots3, double* station,
                             int32_t* found, int32_t* n_not_found, double* times_out) {
  if (h == nullptr || cfg == nullptr || scenes == nullptr || start3 == nullptr || found == nullptr ||
      scenes->center == nullptr)
    return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (int rc = cilqr::check_scene_batch(sb)) return rc;
  if (!(cfg->delta_t > 0.0) || !(cfg->tf > 0.0)) return CILQR_ERR_ARG;
  if ((int32_t)(cfg->tf / cfg->delta_t + 1) != n_knots) return CILQR_ERR_KNOTS;
  if (cilqr::beyond_limits(sb, n_knots)) return CILQR_ERR_CAPACITY;
  if (cilqr::solves_in_flight(h)) return CILQR_ERR_STATE;
  const bool on_host = sb.memory == CILQR_MEM_HOST;
  if (on_host && !cilqr::host_counts_valid(sb)) return CILQR_ERR_ARG;

  // ---- the lattice and the road, by the host planner's own constructors
  const cilqr::DpConfig d = cilqr::dp_config_of(*cfg);
  const cilqr::DpEnvironment env(d, cilqr::reference_line_of(sb.center, sb.n_center));
  const cilqr::DpPlanner dp(d, &env);
  DpParams P;
  std::memset(&P, 0, sizeof(P));
  P.delta_t = d.delta_t; P.unit_time = dp.unit_time(); P.safe_margin = dp.safe_margin();
  P.radius = env.disc_radius(); P.r2x = env.rear_disc_x(); P.f2x = env.front_disc_x(); P.wheel_base = d.wheel_base;
  P.w_obstacle = d.dp_w_obstacle; P.w_lateral = d.dp_w_lateral; P.w_lateral_change = d.dp_w_lateral_change;
  P.w_lateral_velocity_change = d.dp_w_lateral_velocity_change; P.w_velocity_bias = d.dp_w_longitudinal_velocity_bias;
  P.w_velocity_change = d.dp_w_longitudinal_velocity_change; P.nominal_velocity = d.dp_nominal_velocity;
  for (int t = 0; t < cilqr::kDpNT; ++t) P.time[t] = dp.layer_time(t);
  for (int s = 0; s < cilqr::kDpNS; ++s) P.station[s] = dp.station_step(s);
  for (int l = 0; l + 1 < cilqr::kDpNL; ++l) P.lateral[l] = dp.lateral_fraction(l);
  for (int t = 0; t < cilqr::kDpNT; ++t) {
    P.nseg[t] = dp.segment_points(t);
    P.qoff[t + 1] = P.qoff[t] + P.nseg[t];
    if (P.nseg[t] < 1) return CILQR_ERR_KNOTS;   // a layer without a path sample: tf shorter than five steps of delta_t
  }
  P.nq = P.qoff[cilqr::kDpNT];
  if (P.nq > CILQR_DP_MAX_KNOTS) return CILQR_ERR_CAPACITY;
  const std::vector<cilqr::DpPoint2>& barrier = env.barrier();
  P.n_center = sb.n_center; P.n_barrier = (int)barrier.size(); P.n_knots = n_knots;
  P.max_static = sb.max_static; P.max_dynamic = sb.max_dynamic; P.max_vertices = sb.max_vertices; P.max_samples = sb.max_samples;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots;
  // ---- work space of the handle (grown, never shrunk: nothing is allocated once the largest call has been seen): the
  // placed polygons of a chunk; the count, the road's tables and, HOST arrays, a block in and a block out
  cilqr::block_layout l_placed;
  const size_t rec = 4 + 2 * (size_t)sb.max_vertices;
  const size_t per_scene = (size_t)P.nq * sb.max_dynamic * (rec * 8 + 4);
  size_t chunk = B;
  if (per_scene > 0) chunk = std::min(B, std::max<size_t>(1, kPlacedBytesCap / per_scene));
  const cilqr::slot s_placed = l_placed.add(chunk * (size_t)P.nq * sb.max_dynamic * rec * 8);
  const cilqr::slot s_placed_n = l_placed.add(chunk * (size_t)P.nq * sb.max_dynamic * 4);
  HIP_TRY(h->dp_placed.grow(l_placed.bytes() + 256, &h->grown_bytes));
  cilqr::staged_call c(h, h->dp, on_host, st);
  cilqr_scene_batch dv;
  const double* d_start;
  double *d_c9, *d_c6, *d_k3, *d_stn;
  int *d_found, *d_fail;
  static_assert(sizeof(cilqr::DpPoint2) == 16, "the barrier table travels as [n][2] doubles");
  c.table(sb.center, (size_t)sb.n_center * 7, &P.center);
  c.table(reinterpret_cast<const double*>(barrier.data()), barrier.size() * 2, &P.barrier);
  c.counter(&d_fail);
  c.in(start3, B * 3, &d_start);
  c.scenes(sb, &dv);
  c.out(coarse9, B * K * CILQR_COARSE_FIELDS, &d_c9);
  c.out(coarse6, B * K * 6, &d_c6);
  c.out(knots3, B * K * 3, &d_k3);
  c.out(station, B * K, &d_stn);
  c.out(found, B, &d_found);
  if (int rc = c.stage()) return rc;

  double* placed = s_placed.in<double>(h->dp_placed.get());
  int* placed_n = s_placed_n.in<int>(h->dp_placed.get());
  for (size_t first = 0; first < B; first += chunk) {
    const int n = (int)std::min(chunk, B - first);
    cilqr::launch_dp_place(P, dv, (int)first, n, placed, placed_n, st);
    cilqr::launch_dp_plan(P, dv, (int)first, n, d_start, placed, placed_n, d_c9, d_c6, d_k3, d_stn, d_found, d_fail, st);
  }
  HIP_TRY(hipGetLastError());
  if (int rc = c.finish(n_not_found)) return rc;
  if (times_out)   // k_dp_plan's time column: knots past the path's samples stay zero
    for (int k = 0; k < n_knots; ++k) times_out[k] = k < P.nq ? P.delta_t * k : 0.0;
  return CILQR_OK;
}
