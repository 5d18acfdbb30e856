// cilqr_dp_plan_batch (include/cilqr.h): the host side of the batched DP coarse planner -- argument checks, the tables a
// call shares between its scenes (built by the host planner's own classes, include/cilqr/dp_planner.hpp, so that they
// are its bits), the handle's work space, the launches of kernels_dp.hip.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/cilqr/dp_planner.hpp"
#include "dp_core.hpp"
#include "solver_priv.hpp"

namespace {

using cilqr::DpParams;

// the placed dynamic polygons of the scenes in flight: the batch is planned in chunks of as many scenes as fit
constexpr size_t kPlacedBytesCap = (size_t)1 << 30;

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

// counts of HOST arrays: negative, or above what the arrays store
bool host_counts_valid(const cilqr_scene_batch& sb) {
  const size_t B = (size_t)sb.batch;
  for (size_t i = 0; i < B * sb.max_static; ++i)
    if (sb.static_counts[i] < 0 || sb.static_counts[i] > sb.max_vertices) return false;
  for (size_t i = 0; i < B * sb.max_dynamic; ++i)
    if (sb.dynamic_polygon_counts[i] < 0 || sb.dynamic_polygon_counts[i] > sb.max_vertices ||
        sb.dynamic_trajectory_counts[i] < 0 || sb.dynamic_trajectory_counts[i] > sb.max_samples)
      return false;
  return true;
}

}  // namespace

extern "C" int cilqr_dp_plan_batch(cilqr_handle h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes,
                                   const double* start3, int32_t n_knots, double* coarse9, double* coarse6,
                                   double* knots3, double* station, int32_t* found, int32_t* n_not_found) {
  return cilqr_dp_plan_batch_impl(h, cfg, scenes, start3, n_knots, coarse9, coarse6, knots3, station, found, n_not_found,
                                  nullptr);
}

int cilqr_dp_plan_batch_impl(cilqr_solver* h, const cilqr_dp_config* cfg, const cilqr_scene_batch* scenes, const double* start3,
                             int32_t n_knots, double* coarse9, double* coarse6, double* knots3, double* station,
                             int32_t* found, int32_t* n_not_found, double* times_out) {
  if (h == nullptr || cfg == nullptr || scenes == nullptr || start3 == nullptr || found == nullptr ||
      scenes->center == nullptr)
    return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (sb.batch < 1 || sb.n_center < 2 || sb.max_static < 0 || sb.max_dynamic < 0 || sb.max_vertices < 0 ||
      sb.max_samples < 0 || !(cfg->delta_t > 0.0) || !(cfg->tf > 0.0))
    return CILQR_ERR_ARG;
  if (sb.memory != CILQR_MEM_HOST && sb.memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if ((sb.max_static > 0 && (sb.static_points == nullptr || sb.static_counts == nullptr)) ||
      (sb.max_dynamic > 0 && (sb.dynamic_polygon_points == nullptr || sb.dynamic_polygon_counts == nullptr ||
                              sb.dynamic_trajectories == nullptr || sb.dynamic_trajectory_counts == nullptr)))
    return CILQR_ERR_NULL;
  if ((sb.max_static > 0 || sb.max_dynamic > 0) && sb.max_vertices < 1) return CILQR_ERR_ARG;
  if (sb.max_dynamic > 0 && sb.max_samples < 1) return CILQR_ERR_ARG;
  if ((int32_t)(cfg->tf / cfg->delta_t + 1) != n_knots) return CILQR_ERR_KNOTS;
  if (sb.max_vertices > CILQR_DP_MAX_VERTICES || sb.max_static > CILQR_DP_MAX_STATIC ||
      sb.max_dynamic > CILQR_DP_MAX_DYNAMIC || sb.max_samples > CILQR_DP_MAX_SAMPLES || n_knots > CILQR_DP_MAX_KNOTS)
    return CILQR_ERR_CAPACITY;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->job_count != 0) return CILQR_ERR_STATE;   // submitted solves not collected yet (cilqr_wait)
  }
  const bool on_host = sb.memory == CILQR_MEM_HOST;
  if (on_host && !host_counts_valid(sb)) return CILQR_ERR_ARG;

  // ---- the lattice and the road, by the host planner's own constructors
  cilqr::DpConfig d;
  d.tf = cfg->tf; d.delta_t = cfg->delta_t; d.dp_nominal_velocity = cfg->dp_nominal_velocity; d.dp_w_obstacle = cfg->dp_w_obstacle;
  d.dp_w_lateral = cfg->dp_w_lateral; d.dp_w_lateral_change = cfg->dp_w_lateral_change;
  d.dp_w_lateral_velocity_change = cfg->dp_w_lateral_velocity_change;
  d.dp_w_longitudinal_velocity_bias = cfg->dp_w_longitudinal_velocity_bias;
  d.dp_w_longitudinal_velocity_change = cfg->dp_w_longitudinal_velocity_change;
  d.front_hang_length = cfg->front_hang_length; d.wheel_base = cfg->wheel_base; d.rear_hang_length = cfg->rear_hang_length;
  d.width = cfg->width; d.max_velocity = cfg->max_velocity;
  std::vector<std::array<double, 7>> center(sb.n_center);
  for (int i = 0; i < sb.n_center; ++i)
    for (int e = 0; e < 7; ++e) center[i][e] = sb.center[(size_t)i * 7 + e];
  const cilqr::ReferenceLine ref(center);
  const cilqr::DpEnvironment env(d, ref);
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
  // ---- work space of the handle (grown, never shrunk: nothing is allocated once the largest call has been seen)
  const size_t b_center = (size_t)sb.n_center * 7 * 8, b_barrier = barrier.size() * 2 * 8;
  const size_t o_barrier = round256(b_center), b_tab = o_barrier + round256(b_barrier) + 256;
  HIP_TRY(h->dp_tab_host.grow(b_tab));
  HIP_TRY(h->dp_tab.grow(b_tab, &h->grown_bytes));
  if (h->dp_fail.get() == nullptr) HIP_TRY(h->dp_fail.alloc(256));
  if (h->dp_fail_host.get() == nullptr) HIP_TRY(h->dp_fail_host.alloc(64));
  const size_t rec = 4 + 2 * (size_t)sb.max_vertices;
  const size_t per_scene = (size_t)P.nq * sb.max_dynamic * (rec * 8 + 4);
  size_t chunk = B;
  if (per_scene > 0) chunk = std::min(B, std::max<size_t>(1, kPlacedBytesCap / per_scene));
  const size_t o_placed_n = round256(chunk * (size_t)P.nq * sb.max_dynamic * rec * 8);
  HIP_TRY(h->dp_placed.grow(o_placed_n + round256(chunk * (size_t)P.nq * sb.max_dynamic * 4) + 256, &h->grown_bytes));
  // HOST arrays: one block in, one block out
  const size_t b_start = B * 3 * 8, b_sp = B * sb.max_static * sb.max_vertices * 2 * 8, b_sc = B * sb.max_static * 4;
  const size_t b_dp = B * sb.max_dynamic * sb.max_vertices * 2 * 8, b_dc = B * sb.max_dynamic * 4;
  const size_t b_dt = B * sb.max_dynamic * sb.max_samples * 4 * 8;
  const size_t i_sp = round256(b_start), i_sc = i_sp + round256(b_sp), i_dp = i_sc + round256(b_sc), i_dpc = i_dp + round256(b_dp);
  const size_t i_dt = i_dpc + round256(b_dc), i_dtc = i_dt + round256(b_dt), b_in = i_dtc + round256(b_dc) + 256;
  const size_t b_c9 = coarse9 ? B * K * CILQR_COARSE_FIELDS * 8 : 0, b_c6 = coarse6 ? B * K * 6 * 8 : 0;
  const size_t b_k3 = knots3 ? B * K * 3 * 8 : 0, b_stn = station ? B * K * 8 : 0, b_found = B * 4;
  const size_t o_c6 = round256(b_c9), o_k3 = o_c6 + round256(b_c6), o_stn = o_k3 + round256(b_k3);
  const size_t o_found = o_stn + round256(b_stn), b_out = o_found + round256(b_found) + 256;
  if (on_host) {
    HIP_TRY(h->dp_in.grow(b_in, &h->grown_bytes));
    HIP_TRY(h->dp_out.grow(b_out, &h->grown_bytes));
  }

  // ---- tables: pinned block -> device (the stream is waited for at the end of every call, so the block is free again)
  char* th = h->dp_tab_host.as<char>();
  char* td = h->dp_tab.as<char>();
  std::memcpy(th, sb.center, b_center);
  if (b_barrier) std::memcpy(th + o_barrier, barrier.data(), b_barrier);
  static_assert(sizeof(cilqr::DpPoint2) == 16, "the barrier table travels as [n][2] doubles");
  HIP_TRY(hipMemcpyAsync(td, th, o_barrier + b_barrier, hipMemcpyHostToDevice, st));
  P.center = reinterpret_cast<const double*>(td);
  P.barrier = reinterpret_cast<const double*>(td + o_barrier);
  int* d_fail = h->dp_fail.as<int>();
  HIP_TRY(hipMemsetAsync(d_fail, 0, 4, st));

  const double *d_start = start3, *d_sp = sb.static_points, *d_dp = sb.dynamic_polygon_points, *d_dt = sb.dynamic_trajectories;
  const int *d_sc = sb.static_counts, *d_dpc = sb.dynamic_polygon_counts, *d_dtc = sb.dynamic_trajectory_counts;
  double *d_c9 = coarse9, *d_c6 = coarse6, *d_k3 = knots3, *d_stn = station;
  int* d_found = found;
  if (on_host) {
    char* bi = h->dp_in.as<char>();
    char* bo = h->dp_out.as<char>();
    HIP_TRY(hipMemcpyAsync(bi, start3, b_start, hipMemcpyHostToDevice, st));
    if (b_sp) {
      HIP_TRY(hipMemcpyAsync(bi + i_sp, sb.static_points, b_sp, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(bi + i_sc, sb.static_counts, b_sc, hipMemcpyHostToDevice, st));
    }
    if (b_dp) {
      HIP_TRY(hipMemcpyAsync(bi + i_dp, sb.dynamic_polygon_points, b_dp, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(bi + i_dpc, sb.dynamic_polygon_counts, b_dc, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(bi + i_dt, sb.dynamic_trajectories, b_dt, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(bi + i_dtc, sb.dynamic_trajectory_counts, b_dc, hipMemcpyHostToDevice, st));
    }
    d_start = reinterpret_cast<const double*>(bi);
    d_sp = reinterpret_cast<const double*>(bi + i_sp); d_sc = reinterpret_cast<const int*>(bi + i_sc);
    d_dp = reinterpret_cast<const double*>(bi + i_dp); d_dpc = reinterpret_cast<const int*>(bi + i_dpc);
    d_dt = reinterpret_cast<const double*>(bi + i_dt); d_dtc = reinterpret_cast<const int*>(bi + i_dtc);
    if (coarse9) d_c9 = reinterpret_cast<double*>(bo);
    if (coarse6) d_c6 = reinterpret_cast<double*>(bo + o_c6);
    if (knots3) d_k3 = reinterpret_cast<double*>(bo + o_k3);
    if (station) d_stn = reinterpret_cast<double*>(bo + o_stn);
    d_found = reinterpret_cast<int*>(bo + o_found);
  }

  double* placed = h->dp_placed.as<double>();
  int* placed_n = reinterpret_cast<int*>(h->dp_placed.as<char>() + o_placed_n);
  for (size_t first = 0; first < B; first += chunk) {
    const int n = (int)std::min(chunk, B - first);
    cilqr::launch_dp_place(P, (int)first, n, d_dp, d_dpc, d_dt, d_dtc, placed, placed_n, st);
    cilqr::launch_dp_plan(P, (int)first, n, d_start, d_sp, d_sc, d_dpc, d_dtc, placed, placed_n, d_c9, d_c6, d_k3, d_stn,
                          d_found, d_fail, st);
  }
  HIP_TRY(hipGetLastError());
  if (on_host) {
    char* bo = h->dp_out.as<char>();
    if (coarse9) HIP_TRY(hipMemcpyAsync(coarse9, bo, b_c9, hipMemcpyDeviceToHost, st));
    if (coarse6) HIP_TRY(hipMemcpyAsync(coarse6, bo + o_c6, b_c6, hipMemcpyDeviceToHost, st));
    if (knots3) HIP_TRY(hipMemcpyAsync(knots3, bo + o_k3, b_k3, hipMemcpyDeviceToHost, st));
    if (station) HIP_TRY(hipMemcpyAsync(station, bo + o_stn, b_stn, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(found, bo + o_found, b_found, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipMemcpyAsync(h->dp_fail_host.get(), d_fail, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // this stream alone: solves on other handles go on
  if (n_not_found) *n_not_found = *h->dp_fail_host.as<int>();
  if (times_out)   // k_dp_plan's time column: knots past the path's samples stay zero
    for (int k = 0; k < n_knots; ++k) times_out[k] = k < P.nq ? P.delta_t * k : 0.0;
  return CILQR_OK;
}
