// cilqr_scene_points_batch and cilqr_plan_scenes_batch (include/cilqr.h): the host side -- argument checks, the handle's
// work space, staging of HOST arrays, the launches of kernels_scene_points.hip and, for the pipeline, the calls of the
// stages it chains (cilqr_dp_plan_batch, cilqr_build_corridors, cilqr_solve_batch: the public entry points on device
// views, so that what they compute is what a caller of the four calls gets).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "scene_points.hpp"
#include "solver_priv.hpp"

namespace {

using cilqr::ScenePointsParams;

// the obstacle points of the scenes in flight (cilqr_plan_scenes_batch): as many scenes as fit (planner_batch.hip: kPlacedBytesCap)
constexpr size_t kPointsBytesCap = (size_t)1 << 30;

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

// the checks cilqr_dp_plan_batch makes on a scene batch, in its order
int check_scene_batch(const cilqr_scene_batch& sb) {
  if (sb.batch < 1 || sb.n_center < 2 || sb.max_static < 0 || sb.max_dynamic < 0 || sb.max_vertices < 0 || sb.max_samples < 0)
    return CILQR_ERR_ARG;
  if (sb.memory != CILQR_MEM_HOST && sb.memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if ((sb.max_static > 0 && (sb.static_points == nullptr || sb.static_counts == nullptr)) ||
      (sb.max_dynamic > 0 && (sb.dynamic_polygon_points == nullptr || sb.dynamic_polygon_counts == nullptr ||
                              sb.dynamic_trajectories == nullptr || sb.dynamic_trajectory_counts == nullptr)))
    return CILQR_ERR_NULL;
  if ((sb.max_static > 0 || sb.max_dynamic > 0) && sb.max_vertices < 1) return CILQR_ERR_ARG;
  if (sb.max_dynamic > 0 && sb.max_samples < 1) return CILQR_ERR_ARG;
  return CILQR_OK;
}

bool beyond_limits(const cilqr_scene_batch& sb, int n_knots) {
  return sb.max_vertices > CILQR_DP_MAX_VERTICES || sb.max_static > CILQR_DP_MAX_STATIC ||
         sb.max_dynamic > CILQR_DP_MAX_DYNAMIC || sb.max_samples > CILQR_DP_MAX_SAMPLES || n_knots > CILQR_DP_MAX_KNOTS;
}

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

bool solves_in_flight(cilqr_solver* h) {
  std::lock_guard<std::mutex> lk(h->mu);
  return h->job_count != 0;   // submitted solves not collected yet (cilqr_wait)
}

int worst_case_points(const cilqr_scene_batch& sb, int per_vertex) {
  return (sb.max_static + sb.max_dynamic) * sb.max_vertices * per_vertex;
}

// Bytes of the device image of a HOST scene batch, and the image itself: the six per-problem arrays back to back in
// `block` (which holds at least scene_image_bytes), `view` = the batch with its arrays there.
struct SceneImage {
  size_t b_sp, b_sc, b_dp, b_dc, b_dt, o_sc, o_dp, o_dpc, o_dt, o_dtc, bytes;
  explicit SceneImage(const cilqr_scene_batch& sb) {
    const size_t B = (size_t)sb.batch;
    b_sp = B * sb.max_static * sb.max_vertices * 2 * 8; b_sc = B * sb.max_static * 4;
    b_dp = B * sb.max_dynamic * sb.max_vertices * 2 * 8; b_dc = B * sb.max_dynamic * 4;
    b_dt = B * sb.max_dynamic * sb.max_samples * 4 * 8;
    o_sc = round256(b_sp); o_dp = o_sc + round256(b_sc); o_dpc = o_dp + round256(b_dp); o_dt = o_dpc + round256(b_dc);
    o_dtc = o_dt + round256(b_dt); bytes = o_dtc + round256(b_dc);
  }
};

int upload_scene_image(const cilqr_scene_batch& sb, const SceneImage& im, char* block, hipStream_t st, cilqr_scene_batch* view) {
  if (im.b_sp) {
    HIP_TRY(hipMemcpyAsync(block, sb.static_points, im.b_sp, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(block + im.o_sc, sb.static_counts, im.b_sc, hipMemcpyHostToDevice, st));
  }
  if (im.b_dp) {
    HIP_TRY(hipMemcpyAsync(block + im.o_dp, sb.dynamic_polygon_points, im.b_dp, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(block + im.o_dpc, sb.dynamic_polygon_counts, im.b_dc, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(block + im.o_dt, sb.dynamic_trajectories, im.b_dt, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(block + im.o_dtc, sb.dynamic_trajectory_counts, im.b_dc, hipMemcpyHostToDevice, st));
  }
  *view = sb;
  view->memory = CILQR_MEM_DEVICE;
  view->static_points = reinterpret_cast<const double*>(block);
  view->static_counts = reinterpret_cast<const int32_t*>(block + im.o_sc);
  view->dynamic_polygon_points = reinterpret_cast<const double*>(block + im.o_dp);
  view->dynamic_polygon_counts = reinterpret_cast<const int32_t*>(block + im.o_dpc);
  view->dynamic_trajectories = reinterpret_cast<const double*>(block + im.o_dt);
  view->dynamic_trajectory_counts = reinterpret_cast<const int32_t*>(block + im.o_dtc);
  return CILQR_OK;
}

ScenePointsParams points_params(const cilqr_scene_batch& sb, int n_knots, int max_points, int per_vertex) {
  return ScenePointsParams{n_knots, sb.max_static, sb.max_dynamic, sb.max_vertices, sb.max_samples, max_points, per_vertex};
}

void launch_points(const ScenePointsParams& P, const cilqr_scene_batch& dv, int first, int n, const double* d_times,
                   double* points, int* point_count, int* scene_ok, hipStream_t st) {
  cilqr::launch_scene_points(P, first, n, d_times, dv.static_points, dv.static_counts, dv.dynamic_polygon_points,
                             dv.dynamic_polygon_counts, dv.dynamic_trajectories, dv.dynamic_trajectory_counts, points,
                             point_count, scene_ok, st);
}

// the knot times: pinned block -> device table (the stream is waited for at the end of every call, so the block is free again)
int upload_times(cilqr_solver* h, const double* times, int n_knots, hipStream_t st) {
  HIP_TRY(h->sp_host.grow(round256((size_t)CILQR_DP_MAX_KNOTS * 8) + 256));
  HIP_TRY(h->sp_tab.grow(round256((size_t)CILQR_DP_MAX_KNOTS * 8), &h->grown_bytes));
  std::memcpy(h->sp_host.get(), times, (size_t)n_knots * 8);
  HIP_TRY(hipMemcpyAsync(h->sp_tab.get(), h->sp_host.get(), (size_t)n_knots * 8, hipMemcpyHostToDevice, st));
  return CILQR_OK;
}

}  // namespace

extern "C" int cilqr_scene_points_batch(cilqr_handle h, const cilqr_scene_batch* scenes, int32_t n_knots,
                                        const double* knot_times, int32_t is_multiple_sample, int32_t max_points,
                                        double* points, int32_t* point_count, int32_t* scene_ok) {
  if (h == nullptr || scenes == nullptr || knot_times == nullptr || point_count == nullptr) return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (int rc = check_scene_batch(sb)) return rc;
  if (n_knots < 1 || max_points < 0) return CILQR_ERR_ARG;
  if (beyond_limits(sb, n_knots)) return CILQR_ERR_CAPACITY;
  const int per_vertex = is_multiple_sample ? 6 : 1;
  if (max_points < worst_case_points(sb, per_vertex)) return CILQR_ERR_ARG;
  if (points == nullptr && max_points > 0) return CILQR_ERR_NULL;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;
  const bool on_host = sb.memory == CILQR_MEM_HOST;
  if (on_host && !host_counts_valid(sb)) return CILQR_ERR_ARG;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots;
  if (int rc = upload_times(h, knot_times, n_knots, st)) return rc;
  const ScenePointsParams P = points_params(sb, n_knots, max_points, per_vertex);
  const double* d_times = h->sp_tab.as<double>();
  if (!on_host) {
    launch_points(P, sb, 0, sb.batch, d_times, points, point_count, scene_ok, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // this stream alone: solves on other handles go on
    return CILQR_OK;
  }
  // HOST arrays: the scenes in, the caller's points in as well (what lies behind point_count stays as it is), all out
  const SceneImage im(sb);
  const size_t b_pts = B * K * (size_t)max_points * 2 * 8, b_cnt = B * K * 4, b_ok = B * 4;
  const size_t o_cnt = round256(b_pts), o_ok = o_cnt + round256(b_cnt);
  HIP_TRY(h->sp_in.grow(im.bytes + 256, &h->grown_bytes));
  HIP_TRY(h->sp_out.grow(o_ok + round256(b_ok) + 256, &h->grown_bytes));
  cilqr_scene_batch dv;
  if (int rc = upload_scene_image(sb, im, h->sp_in.as<char>(), st, &dv)) return rc;
  char* bo = h->sp_out.as<char>();
  if (b_pts) HIP_TRY(hipMemcpyAsync(bo, points, b_pts, hipMemcpyHostToDevice, st));
  launch_points(P, dv, 0, sb.batch, d_times, reinterpret_cast<double*>(bo), reinterpret_cast<int*>(bo + o_cnt),
                reinterpret_cast<int*>(bo + o_ok), st);
  HIP_TRY(hipGetLastError());
  if (b_pts) HIP_TRY(hipMemcpyAsync(points, bo, b_pts, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(point_count, bo + o_cnt, b_cnt, hipMemcpyDeviceToHost, st));
  if (scene_ok) HIP_TRY(hipMemcpyAsync(scene_ok, bo + o_ok, b_ok, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CILQR_OK;
}

extern "C" int cilqr_plan_scenes_batch(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_corridor_config* corridor_cfg,
                                       const cilqr_scene_batch* scenes, const double* start4, int32_t n_knots,
                                       cilqr_solution_batch* out, double* plan, double* coarse9, int32_t* outcome,
                                       int32_t* n_dp_failed, int32_t* n_corridor_failed) {
  if (h == nullptr || dp_cfg == nullptr || corridor_cfg == nullptr || scenes == nullptr || start4 == nullptr ||
      out == nullptr || scenes->center == nullptr)
    return CILQR_ERR_NULL;
  if (out->traj == nullptr || out->cost_hist == nullptr || out->n_cost == nullptr || out->status == nullptr)
    return CILQR_ERR_NULL;
  const cilqr_scene_batch& sb = *scenes;
  if (int rc = check_scene_batch(sb)) return rc;
  if (!(dp_cfg->delta_t > 0.0) || !(dp_cfg->tf > 0.0)) return CILQR_ERR_ARG;
  if (out->memory != CILQR_MEM_HOST && out->memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if ((int32_t)(dp_cfg->tf / dp_cfg->delta_t + 1) != n_knots || n_knots != h->cfg.n_steps + 1) return CILQR_ERR_KNOTS;
  if (beyond_limits(sb, n_knots) || sb.batch > h->capacity) return CILQR_ERR_CAPACITY;
  const int per_vertex = corridor_cfg->is_multiple_sample ? 6 : 1;
  const int max_points = worst_case_points(sb, per_vertex);
  if (max_points + (corridor_cfg->is_multiple_sample ? 24 : 8) > cilqr::kCorMaxPts) return CILQR_ERR_CAPACITY;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;
  const bool on_host = sb.memory == CILQR_MEM_HOST;
  if (on_host && !host_counts_valid(sb)) return CILQR_ERR_ARG;

  // ---- lane tables (Corridor::Plan, corridor.cc:43-51): once per call, on the host
  const int cap = (int)((sb.center[(size_t)(sb.n_center - 1) * 7] - sb.center[0]) / 0.1) + 8;
  if (cap < 1) return CILQR_ERR_ARG;
  std::vector<double> left((size_t)cap * 2), right((size_t)cap * 2);
  const int n_barrier = cilqr_road_barriers(sb.center, sb.n_center, left.data(), right.data(), cap);
  if (n_barrier < 0) return n_barrier;
  std::vector<double> left_rows((size_t)n_barrier * CILQR_LANE_FIELDS), right_rows((size_t)n_barrier * CILQR_LANE_FIELDS);
  const int n_left = cilqr_lane_constraints(left.data(), n_barrier, corridor_cfg->lane_segment_length, 1, left_rows.data(), n_barrier);
  if (n_left < 0) return n_left;
  const int n_right = cilqr_lane_constraints(right.data(), n_barrier, corridor_cfg->lane_segment_length, 0, right_rows.data(), n_barrier);
  if (n_right < 0) return n_right;
  if (n_left > h->smax || n_right > h->smax) return CILQR_ERR_CAPACITY;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)sb.batch, K = (size_t)n_knots, cmax = (size_t)h->cmax;
  // ---- work space: the intermediates of the whole batch, then (HOST arrays) the scenes and the outputs on their way
  const size_t b_s3 = B * 3 * 8, b_c6 = B * K * 6 * 8, b_k3 = B * K * 3 * 8, b_stn = B * K * 8, b_found = B * 4;
  const size_t b_cor = B * K * cmax * 3 * 8, b_ccnt = B * K * 4, b_counts = 2 * 4;
  const size_t b_traj = out->memory == CILQR_MEM_HOST && plan ? B * K * CILQR_TRAJ_FIELDS * 8 : 0;
  const size_t o_c6 = round256(b_s3), o_k3 = o_c6 + round256(b_c6), o_stn = o_k3 + round256(b_k3), o_found = o_stn + round256(b_stn);
  const size_t o_cor = o_found + round256(b_found), o_ccnt = o_cor + round256(b_cor), o_counts = o_ccnt + round256(b_ccnt);
  const size_t o_traj = o_counts + round256(b_counts), o_host = o_traj + round256(b_traj);
  const SceneImage im(sb);
  const size_t b_s4 = B * 4 * 8, b_plan = plan ? B * K * CILQR_PLAN_FIELDS * 8 : 0, b_c9 = coarse9 ? B * K * CILQR_COARSE_FIELDS * 8 : 0;
  const size_t b_outcome = outcome ? B * 4 : 0;
  const size_t o_s4 = o_host + round256(im.bytes), o_plan = o_s4 + round256(b_s4), o_c9 = o_plan + round256(b_plan);
  const size_t o_outcome = o_c9 + round256(b_c9);
  HIP_TRY(h->ps_work.grow((on_host ? o_outcome + round256(b_outcome) : o_host) + 256, &h->grown_bytes));
  const size_t per_scene = K * ((size_t)max_points * 2 * 8 + 4);
  size_t chunk = std::min(B, std::max<size_t>(1, kPointsBytesCap / per_scene));
  if (h->scene_chunk > 0) chunk = std::min(B, (size_t)h->scene_chunk);
  const size_t o_pcnt = round256(chunk * K * (size_t)max_points * 2 * 8);
  HIP_TRY(h->ps_points.grow(o_pcnt + round256(chunk * K * 4) + 256, &h->grown_bytes));
  HIP_TRY(h->sp_host.grow(round256((size_t)CILQR_DP_MAX_KNOTS * 8) + 256));

  char* w = h->ps_work.as<char>();
  double *d_s3 = reinterpret_cast<double*>(w), *d_c6 = reinterpret_cast<double*>(w + o_c6), *d_k3 = reinterpret_cast<double*>(w + o_k3);
  double *d_stn = reinterpret_cast<double*>(w + o_stn), *d_cor = reinterpret_cast<double*>(w + o_cor);
  int *d_found = reinterpret_cast<int*>(w + o_found), *d_ccnt = reinterpret_cast<int*>(w + o_ccnt), *d_counts = reinterpret_cast<int*>(w + o_counts);
  cilqr_scene_batch dv = sb;
  const double* d_s4 = start4;
  double *d_plan = plan, *d_c9 = coarse9;
  int* d_outcome = outcome;
  if (on_host) {
    if (int rc = upload_scene_image(sb, im, w + o_host, st, &dv)) return rc;
    HIP_TRY(hipMemcpyAsync(w + o_s4, start4, b_s4, hipMemcpyHostToDevice, st));
    d_s4 = reinterpret_cast<const double*>(w + o_s4);
    if (plan) d_plan = reinterpret_cast<double*>(w + o_plan);
    if (coarse9) d_c9 = reinterpret_cast<double*>(w + o_c9);
    if (outcome) d_outcome = reinterpret_cast<int*>(w + o_outcome);
  }
  HIP_TRY(hipMemsetAsync(d_counts, 0, b_counts, st));

  // ---- DpPlanner::Plan (trajectory_planner.cpp:32)
  cilqr::launch_plan_start3((int)B, d_s4, d_s3, st);
  HIP_TRY(hipGetLastError());
  std::vector<double> times(K);
  if (int rc = cilqr_dp_plan_batch_impl(h, dp_cfg, &dv, d_s3, n_knots, d_c9, d_c6, d_k3, d_stn, d_found, nullptr, times.data()))
    return rc;

  // ---- Corridor::BuildCorridorConstraints (corridor.cc:58-87) with the Environment's points, a chunk of scenes at a time
  if (int rc = upload_times(h, times.data(), n_knots, st)) return rc;
  const ScenePointsParams P = points_params(sb, n_knots, max_points, per_vertex);
  double* d_pts = h->ps_points.as<double>();
  int* d_pcnt = reinterpret_cast<int*>(h->ps_points.as<char>() + o_pcnt);
  for (size_t first = 0; first < B; first += chunk) {
    const int n = (int)std::min(chunk, B - first);
    launch_points(P, dv, (int)first, n, h->sp_tab.as<double>(), d_pts, d_pcnt, nullptr, st);
    HIP_TRY(hipGetLastError());
    if (int rc = cilqr_build_corridors(h, corridor_cfg, n, n_knots, d_k3 + first * K * 3, d_pts, d_pcnt, max_points,
                                       d_cor + first * K * cmax * 3, d_ccnt + first * K, (int32_t)cmax, CILQR_MEM_DEVICE,
                                       nullptr, nullptr))
      return rc;
  }
  cilqr::launch_plan_outcome((int)B, n_knots, d_found, d_ccnt, d_outcome, d_counts, st);
  HIP_TRY(hipGetLastError());

  // ---- IlqrOptimizer::Plan (trajectory_planner.cpp:80-86)
  cilqr_problem_batch prob;
  std::memset(&prob, 0, sizeof(prob));
  prob.batch = sb.batch; prob.n_knots = n_knots; prob.cmax = (int32_t)cmax; prob.memory = CILQR_MEM_DEVICE;
  prob.start = d_s4; prob.coarse = d_c6; prob.corridor = d_cor; prob.corridor_count = d_ccnt;
  prob.n_left = n_left; prob.n_right = n_right; prob.left_lane = left_rows.data(); prob.right_lane = right_rows.data();
  prob.coarse_station = d_stn;
  if (int rc = cilqr_solve_batch(h, &prob, out)) return rc;

  // ---- the result rows (trajectory_planner.cpp:101-125) and the way back
  if (plan) {
    const double* d_traj = out->traj;
    if (out->memory == CILQR_MEM_HOST) {
      HIP_TRY(hipMemcpyAsync(w + o_traj, out->traj, b_traj, hipMemcpyHostToDevice, st));
      d_traj = reinterpret_cast<const double*>(w + o_traj);
    }
    cilqr::launch_plan_rows((int)B, n_knots, d_traj, d_plan, st);
    HIP_TRY(hipGetLastError());
  }
  if (on_host) {
    if (plan) HIP_TRY(hipMemcpyAsync(plan, d_plan, b_plan, hipMemcpyDeviceToHost, st));
    if (coarse9) HIP_TRY(hipMemcpyAsync(coarse9, d_c9, b_c9, hipMemcpyDeviceToHost, st));
    if (outcome) HIP_TRY(hipMemcpyAsync(outcome, d_outcome, b_outcome, hipMemcpyDeviceToHost, st));
  }
  int* counts_host = reinterpret_cast<int*>(h->sp_host.as<char>() + round256((size_t)CILQR_DP_MAX_KNOTS * 8));
  HIP_TRY(hipMemcpyAsync(counts_host, d_counts, b_counts, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // this stream alone: solves on other handles go on
  if (n_dp_failed) *n_dp_failed = counts_host[0];
  if (n_corridor_failed) *n_corridor_failed = counts_host[1];
  return CILQR_OK;
}
