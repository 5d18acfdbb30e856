// cilqr_scene_points_batch and cilqr_plan_scenes_batch / _warm (include/cilqr.h): the host side -- argument checks, the handle's
// work space, staging of HOST arrays, the launches of kernels_scene_points.hip and, for the pipeline, the calls of the
// stages it chains (cilqr_dp_plan_batch, cilqr_build_corridors, cilqr_solve_batch_warm: the public entry points on device
// views, so that what they compute is what a caller of the four calls gets).  The pipeline's body is shared with
// carry_pipeline.hip (scene_pipeline.hpp), which puts another coarse stage in the DP planner's place.
#include <algorithm>
#include <cstring>
#include <vector>

#include "scene_pipeline.hpp"
#include "scene_points.hpp"

using namespace cilqr;

namespace {

// the obstacle points of the scenes in flight (cilqr_plan_scenes_batch): as many scenes as fit (planner_batch.hip: kPlacedBytesCap)
constexpr size_t kPointsBytesCap = (size_t)1 << 30;

int worst_case_points(const cilqr_scene_batch& sb, int per_vertex) {
  return (sb.max_static + sb.max_dynamic) * sb.max_vertices * per_vertex;
}

ScenePointsParams points_params(const cilqr_scene_batch& sb, int n_knots, int max_points, int per_vertex) {
  return ScenePointsParams{n_knots, sb.max_static, sb.max_dynamic, sb.max_vertices, sb.max_samples, max_points, per_vertex};
}

// the pinned block sp_host: the knot times of the longest trajectory, then the pipeline's two outcome counts
struct HostBlock {
  block_layout l;
  slot times = l.add((size_t)CILQR_DP_MAX_KNOTS * 8), counts = l.add(2 * 4);
};
const HostBlock kHost;

// the knot times: pinned block -> device table (the stream is waited for at the end of every call, so the block is free again)
int upload_times(cilqr_solver* h, const double* times, int n_knots, hipStream_t st) {
  HIP_TRY(h->sp_host.grow(kHost.l.bytes()));
  HIP_TRY(h->sp.tab.grow(kHost.times.bytes, &h->grown_bytes));
  std::memcpy(h->sp_host.get(), times, (size_t)n_knots * 8);
  HIP_TRY(hipMemcpyAsync(h->sp.tab.get(), h->sp_host.get(), (size_t)n_knots * 8, hipMemcpyHostToDevice, st));
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
  const ScenePointsParams P = points_params(sb, n_knots, max_points, per_vertex);
  // the knot times and, HOST arrays, a block in and a block out: the handle's work space (grown, never shrunk)
  staged_call c(h, h->sp, on_host, st);
  cilqr_scene_batch dv;
  const double* d_times;
  double* d_pts;
  int *d_cnt, *d_ok;
  c.table(knot_times, K, &d_times);
  c.scenes(sb, &dv);
  c.inout(points, B * K * max_points * 2, &d_pts);   // what lies behind point_count stays as it is
  c.out(point_count, B * K, &d_cnt);
  c.out(scene_ok, B, &d_ok);
  if (int rc = c.stage()) return rc;
  launch_scene_points(P, dv, 0, sb.batch, d_times, d_pts, d_cnt, d_ok, st);
  HIP_TRY(hipGetLastError());
  return c.finish();
}

// the body of the pipeline entry points; `warm` NULL: the plain call (cilqr_solve_batch_warm with NULL is cilqr_solve_batch);
// `coarse` NULL: the DP planner on the whole batch
int cilqr::plan_scenes(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_corridor_config* corridor_cfg,
                       const cilqr_scene_batch* scenes, const double* start4, int32_t n_knots, const cilqr_warm_start* warm,
                       CoarseStage* coarse, cilqr_solution_batch* out, double* plan, double* coarse9, int32_t* outcome,
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
  // the warm start against the problem batch the solve will get: n_knots knots, its arrays where the scenes are
  if (warm != nullptr) {
    cilqr_problem_batch like;
    std::memset(&like, 0, sizeof(like));
    like.batch = sb.batch; like.n_knots = n_knots; like.memory = sb.memory;
    if (int rc = cilqr_check_warm(&like, warm)) return rc;
  }
  const int per_vertex = corridor_cfg->is_multiple_sample ? 6 : 1;
  const int max_points = worst_case_points(sb, per_vertex);
  if (max_points + (corridor_cfg->is_multiple_sample ? 24 : 8) > kCorMaxPts) return CILQR_ERR_CAPACITY;
  if (coarse != nullptr)
    if (int rc = coarse->check(*dp_cfg, sb, n_knots)) return rc;
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
  block_layout l_work, l_points;
  const slot s_s3 = l_work.add(B * 3 * 8), s_c6 = l_work.add(B * K * 6 * 8), s_k3 = l_work.add(B * K * 3 * 8);
  const slot s_stn = l_work.add(B * K * 8), s_found = l_work.add(B * 4), s_cor = l_work.add(B * K * cmax * 3 * 8);
  const slot s_ccnt = l_work.add(B * K * 4), s_counts = l_work.add(2 * 4);
  const slot s_traj = l_work.add(out->memory == CILQR_MEM_HOST && plan ? B * K * CILQR_TRAJ_FIELDS * 8 : 0);
  const size_t b_device = l_work.bytes();   // what a call on DEVICE arrays needs
  const SceneImage im(l_work, sb);
  const slot s_s4 = l_work.add(B * 4 * 8), s_plan = l_work.add(plan ? B * K * CILQR_PLAN_FIELDS * 8 : 0);
  const slot s_c9 = l_work.add(coarse9 ? B * K * CILQR_COARSE_FIELDS * 8 : 0), s_outcome = l_work.add(outcome ? B * 4 : 0);
  const slot s_wrows = l_work.add(warm ? B * widths(*warm, n_knots).rows * 8 : 0), s_wshift = l_work.add(warm && warm->shift ? B * 4 : 0);
  HIP_TRY(h->ps_work.grow((on_host ? l_work.bytes() : b_device) + 256, &h->grown_bytes));
  const size_t per_scene = K * ((size_t)max_points * 2 * 8 + 4);
  size_t chunk = std::min(B, std::max<size_t>(1, kPointsBytesCap / per_scene));
  if (h->scene_chunk > 0) chunk = std::min(B, (size_t)h->scene_chunk);
  const slot s_pts = l_points.add(chunk * K * (size_t)max_points * 2 * 8), s_pcnt = l_points.add(chunk * K * 4);
  HIP_TRY(h->ps_points.grow(l_points.bytes() + 256, &h->grown_bytes));
  HIP_TRY(h->sp_host.grow(kHost.l.bytes()));

  char* w = h->ps_work.as<char>();
  double *d_s3 = s_s3.in<double>(w), *d_c6 = s_c6.in<double>(w), *d_k3 = s_k3.in<double>(w);
  double *d_stn = s_stn.in<double>(w), *d_cor = s_cor.in<double>(w);
  int *d_found = s_found.in<int>(w), *d_ccnt = s_ccnt.in<int>(w), *d_counts = s_counts.in<int>(w);
  cilqr_scene_batch dv = sb;
  const double* d_s4 = start4;
  double *d_plan = plan, *d_c9 = coarse9;
  int* d_outcome = outcome;
  if (on_host) {
    if (int rc = im.upload(sb, w, st, &dv)) return rc;
    if (int rc = copy_in(w, s_s4, start4, st)) return rc;
    d_s4 = s_s4.in<const double>(w);
    if (plan) d_plan = s_plan.in<double>(w);
    if (coarse9) d_c9 = s_c9.in<double>(w);
    if (outcome) d_outcome = s_outcome.in<int>(w);
  }
  cilqr_warm_start dw;   // the warm start as the solve on device views takes it
  if (warm != nullptr) {
    dw = *warm;
    dw.memory = CILQR_MEM_DEVICE;
    if (on_host) {
      if (int rc = copy_in(w, s_wrows, warm->rows, st)) return rc;
      if (int rc = copy_in(w, s_wshift, warm->shift, st)) return rc;
      dw.rows = s_wrows.in<const double>(w);
      dw.shift = warm->shift ? s_wshift.in<const int32_t>(w) : nullptr;
    }
  }
  HIP_TRY(hipMemsetAsync(d_counts, 0, s_counts.bytes, st));

  // ---- DpPlanner::Plan (trajectory_planner.cpp:32), or the caller's coarse stage in its place
  std::vector<double> times(K);
  if (coarse == nullptr) {
    launch_plan_start3((int)B, d_s4, d_s3, st);
    HIP_TRY(hipGetLastError());
    if (int rc = cilqr_dp_plan_batch_impl(h, dp_cfg, &dv, d_s3, n_knots, d_c9, d_c6, d_k3, d_stn, d_found, nullptr, times.data()))
      return rc;
  } else {
    const CoarseArgs a{h, dp_cfg, &sb, &dv, n_knots, d_s4, d_s3, d_c9, d_c6, d_k3, d_stn, d_found, times.data()};
    if (int rc = coarse->run(a)) return rc;
  }

  // ---- Corridor::BuildCorridorConstraints (corridor.cc:58-87) with the Environment's points, a chunk of scenes at a time
  if (int rc = upload_times(h, times.data(), n_knots, st)) return rc;
  const ScenePointsParams P = points_params(sb, n_knots, max_points, per_vertex);
  double* d_pts = s_pts.in<double>(h->ps_points.get());
  int* d_pcnt = s_pcnt.in<int>(h->ps_points.get());
  for (size_t first = 0; first < B; first += chunk) {
    const int n = (int)std::min(chunk, B - first);
    launch_scene_points(P, dv, (int)first, n, h->sp.tab.as<double>(), d_pts, d_pcnt, nullptr, st);
    HIP_TRY(hipGetLastError());
    if (int rc = cilqr_build_corridors(h, corridor_cfg, n, n_knots, d_k3 + first * K * 3, d_pts, d_pcnt, max_points,
                                       d_cor + first * K * cmax * 3, d_ccnt + first * K, (int32_t)cmax, CILQR_MEM_DEVICE,
                                       nullptr, nullptr))
      return rc;
  }
  launch_plan_outcome((int)B, n_knots, d_found, d_ccnt, d_outcome, d_counts, st);
  HIP_TRY(hipGetLastError());

  // ---- IlqrOptimizer::Plan (trajectory_planner.cpp:80-86)
  cilqr_problem_batch prob;
  std::memset(&prob, 0, sizeof(prob));
  prob.batch = sb.batch; prob.n_knots = n_knots; prob.cmax = (int32_t)cmax; prob.memory = CILQR_MEM_DEVICE;
  prob.start = d_s4; prob.coarse = d_c6; prob.corridor = d_cor; prob.corridor_count = d_ccnt;
  prob.n_left = n_left; prob.n_right = n_right; prob.left_lane = left_rows.data(); prob.right_lane = right_rows.data();
  prob.coarse_station = d_stn;
  if (int rc = cilqr_solve_batch_warm(h, &prob, warm ? &dw : nullptr, out)) return rc;

  // ---- the result rows (trajectory_planner.cpp:101-125) and the way back
  if (plan) {
    const double* d_traj = out->traj;
    if (out->memory == CILQR_MEM_HOST) {
      if (int rc = copy_in(w, s_traj, out->traj, st)) return rc;
      d_traj = s_traj.in<const double>(w);
    }
    launch_plan_rows((int)B, n_knots, d_traj, d_plan, st);
    HIP_TRY(hipGetLastError());
  }
  if (on_host) {
    if (int rc = copy_out(plan, w, s_plan, st)) return rc;
    if (int rc = copy_out(coarse9, w, s_c9, st)) return rc;
    if (int rc = copy_out(outcome, w, s_outcome, st)) return rc;
  }
  int* counts_host = kHost.counts.in<int>(h->sp_host.get());
  HIP_TRY(hipMemcpyAsync(counts_host, d_counts, s_counts.bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // this stream alone: solves on other handles go on
  if (n_dp_failed) *n_dp_failed = counts_host[0];
  if (n_corridor_failed) *n_corridor_failed = counts_host[1];
  return CILQR_OK;
}

extern "C" int cilqr_plan_scenes_batch(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_corridor_config* corridor_cfg,
                                       const cilqr_scene_batch* scenes, const double* start4, int32_t n_knots,
                                       cilqr_solution_batch* out, double* plan, double* coarse9, int32_t* outcome,
                                       int32_t* n_dp_failed, int32_t* n_corridor_failed) {
  return plan_scenes(h, dp_cfg, corridor_cfg, scenes, start4, n_knots, nullptr, nullptr, out, plan, coarse9, outcome,
                     n_dp_failed, n_corridor_failed);
}

extern "C" int cilqr_plan_scenes_batch_warm(cilqr_handle h, const cilqr_dp_config* dp_cfg,
                                            const cilqr_corridor_config* corridor_cfg, const cilqr_scene_batch* scenes,
                                            const double* start4, int32_t n_knots, const cilqr_warm_start* warm,
                                            cilqr_solution_batch* out, double* plan, double* coarse9, int32_t* outcome,
                                            int32_t* n_dp_failed, int32_t* n_corridor_failed) {
  return plan_scenes(h, dp_cfg, corridor_cfg, scenes, start4, n_knots, warm, nullptr, out, plan, coarse9, outcome,
                     n_dp_failed, n_corridor_failed);
}
