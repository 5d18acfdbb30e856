// cilqr_plan_scenes_batch_carry (include/cilqr.h, "the pipeline of a later cycle"): the pipeline of scene_pipeline.hip with
// another coarse stage -- carry, audit, select, and the DP planner for the listed scenes alone.  Every step is the public
// entry point on device views (cilqr_check_collisions_batch) or the body behind one (carry_rows_batch_impl,
// cilqr_dp_plan_batch_impl), so that what the stage computes is what a caller of those calls gets; k_dp_plan sees a listed
// scene as a scene of a batch of its own.
#include <algorithm>
#include <cmath>

#include "../../include/cilqr/trajectory_queries.hpp"
#include "carry.hpp"
#include "scene_pipeline.hpp"
#include "scene_points.hpp"

using namespace cilqr;

namespace {

// the gathered scenes in flight: as many as fit (planner_batch.hip: kPlacedBytesCap), unless CILQR_OPT_SCENE_CHUNK says
constexpr size_t kGatherBytesCap = (size_t)1 << 30;

struct CarryStage : CoarseStage {
  const cilqr_carry& c;
  int32_t* source;   // the caller's, in the memory of the scenes; may be null
  int n_live = 0;    // the path samples the planner fills
  int n_sel = 0;
  CarryStage(const cilqr_carry& carry, int32_t* src) : c(carry), source(src) {}

  int check(const cilqr_dp_config& dp_cfg, const cilqr_scene_batch& sb, int n_knots) override {
    if (c.rows == nullptr || c.advance == nullptr) return CILQR_ERR_NULL;
    if (c.memory != sb.memory) return CILQR_ERR_ARG;
    if (!std::isfinite(c.max_start_offset) || c.max_start_offset < 0.0) return CILQR_ERR_ARG;
    if (!std::isfinite(c.collision_buffer) || c.collision_buffer < 0.0) return CILQR_ERR_ARG;
    if (int rc = check_carry_arguments(c.layout, c.n_rows, c.max_advance)) return rc;
    int32_t nq = 0;
    if (int rc = cilqr_dp_path_samples(&dp_cfg, &sb, n_knots, &nq)) return rc;
    n_live = std::min<int>(nq, n_knots);
    return CILQR_OK;
  }

  int run(const CoarseArgs& a) override {
    cilqr_solver* h = a.h;
    hipStream_t st = h->stream;
    const cilqr_scene_batch& dv = *a.dv;
    const size_t B = (size_t)dv.batch, K = (size_t)a.n_knots, R = (size_t)c.n_rows;
    const size_t F = (size_t)trajectory_queries::columns_of(c.layout).fields;
    const bool on_host = c.memory == CILQR_MEM_HOST;
    // ---- work space of the stage: what it keeps of the whole batch, then (HOST arrays) the rows and advances on their way
    block_layout l;
    const slot s_state = l.add(B * 4), s_first = l.add(B * 4), s_sel = l.add(B * 4), s_nsel = l.add(4);
    const slot s_c9 = l.add(a.d_coarse9 ? 0 : B * K * CILQR_COARSE_FIELDS * 8);
    const slot s_src = l.add(on_host && source ? B * 4 : 0);
    const slot s_rows = l.add(on_host ? B * R * F * 8 : 0), s_adv = l.add(on_host ? B * 8 : 0);
    HIP_TRY(h->cy_work.grow(l.bytes() + 256, &h->grown_bytes));
    HIP_TRY(h->cy_sel_host.grow(64));
    char* w = h->cy_work.as<char>();
    int *d_state = s_state.in<int>(w), *d_first = s_first.in<int>(w), *d_sel = s_sel.in<int>(w), *d_nsel = s_nsel.in<int>(w);
    double* d_c9 = a.d_coarse9 ? a.d_coarse9 : s_c9.in<double>(w);
    int* d_src = source;
    const double *d_rows = c.rows, *d_adv = c.advance;
    if (on_host) {
      if (int rc = copy_in(w, s_rows, c.rows, st)) return rc;
      if (int rc = copy_in(w, s_adv, c.advance, st)) return rc;
      d_rows = s_rows.in<const double>(w);
      d_adv = s_adv.in<const double>(w);
      if (source) d_src = s_src.in<int>(w);
    }

    // ---- 1. carry, 2. audit, 3. select
    if (int rc = carry_rows_batch_impl(h, dv.batch, c.layout, d_rows, c.n_rows, d_adv, c.max_advance, a.n_knots, n_live,
                                       a.dp_cfg->delta_t, d_c9, a.d_coarse6, a.d_knots3, a.d_station, d_state, nullptr,
                                       CILQR_MEM_DEVICE))
      return rc;
    if (int rc = cilqr_check_collisions_batch(h, a.dp_cfg, &dv, CILQR_ROWS_COARSE, d_c9, a.n_knots, c.collision_buffer, nullptr,
                                              d_first, nullptr, nullptr))
      return rc;
    launch_carry_select((int)B, a.n_knots, d_state, a.d_start4, d_c9, d_first, c.max_start_offset, d_src, a.d_found, d_sel,
                        d_nsel, st);
    HIP_TRY(hipGetLastError());
    if (on_host && source) HIP_TRY(hipMemcpyAsync(source, d_src, B * 4, hipMemcpyDeviceToHost, st));
    int* nsel_host = h->cy_sel_host.as<int>();
    HIP_TRY(hipMemcpyAsync(nsel_host, d_nsel, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // this stream alone: how many scenes the planner gets decides what is launched next
    n_sel = *nsel_host;
    for (size_t k = 0; k < K; ++k) a.times[k] = (int)k < n_live ? a.dp_cfg->delta_t * (double)k : 0.0;   // the planner's time column

    // ---- 4. DpPlanner::Plan for the listed scenes
    if (n_sel == 0) return CILQR_OK;
    launch_plan_start3((int)B, a.d_start4, a.d_start3, st);
    HIP_TRY(hipGetLastError());
    if ((size_t)n_sel == B)   // the batch as it lies
      return cilqr_dp_plan_batch_impl(h, a.dp_cfg, &dv, a.d_start3, a.n_knots, a.d_coarse9, a.d_coarse6, a.d_knots3,
                                      a.d_station, a.d_found, nullptr, nullptr);
    const size_t b_sp = (size_t)dv.max_static * dv.max_vertices * 2 * 8, b_sc = (size_t)dv.max_static * 4;
    const size_t b_dp = (size_t)dv.max_dynamic * dv.max_vertices * 2 * 8, b_dc = (size_t)dv.max_dynamic * 4;
    const size_t b_dt = (size_t)dv.max_dynamic * dv.max_samples * 4 * 8;
    const size_t per_scene = b_sp + b_sc + b_dp + 2 * b_dc + b_dt + 3 * 8 + K * 19 * 8 + 4;
    size_t chunk = std::min<size_t>((size_t)n_sel, std::max<size_t>(1, kGatherBytesCap / per_scene));
    if (h->scene_chunk > 0) chunk = std::min<size_t>((size_t)n_sel, (size_t)h->scene_chunk);
    block_layout lc;
    cilqr_scene_batch cv = dv;   // a chunk of listed scenes as a batch of its own, with the batch's max_*
    cv.batch = (int32_t)chunk;
    const SceneImage im(lc, cv);
    const slot c_s3 = lc.add(chunk * 3 * 8), c_c9 = lc.add(a.d_coarse9 ? chunk * K * CILQR_COARSE_FIELDS * 8 : 0);
    const slot c_c6 = lc.add(chunk * K * 6 * 8), c_k3 = lc.add(chunk * K * 3 * 8), c_stn = lc.add(chunk * K * 8);
    const slot c_found = lc.add(chunk * 4);
    HIP_TRY(h->cy_chunk.grow(lc.bytes() + 256, &h->grown_bytes));
    char* g = h->cy_chunk.as<char>();
    cv.static_points = im.sp.in<const double>(g); cv.static_counts = im.sc.in<const int32_t>(g);
    cv.dynamic_polygon_points = im.dp.in<const double>(g); cv.dynamic_polygon_counts = im.dpc.in<const int32_t>(g);
    cv.dynamic_trajectories = im.dt.in<const double>(g); cv.dynamic_trajectory_counts = im.dtc.in<const int32_t>(g);
    double *g_s3 = c_s3.in<double>(g), *g_c9 = a.d_coarse9 ? c_c9.in<double>(g) : nullptr, *g_c6 = c_c6.in<double>(g);
    double *g_k3 = c_k3.in<double>(g), *g_stn = c_stn.in<double>(g);
    int* g_found = c_found.in<int>(g);
    for (size_t first = 0; first < (size_t)n_sel; first += chunk) {
      const int n = (int)std::min(chunk, (size_t)n_sel - first), f = (int)first;
      launch_carry_gather(dv.static_points, im.sp.in<char>(g), b_sp, d_sel, f, n, st);
      launch_carry_gather(dv.static_counts, im.sc.in<char>(g), b_sc, d_sel, f, n, st);
      launch_carry_gather(dv.dynamic_polygon_points, im.dp.in<char>(g), b_dp, d_sel, f, n, st);
      launch_carry_gather(dv.dynamic_polygon_counts, im.dpc.in<char>(g), b_dc, d_sel, f, n, st);
      launch_carry_gather(dv.dynamic_trajectories, im.dt.in<char>(g), b_dt, d_sel, f, n, st);
      launch_carry_gather(dv.dynamic_trajectory_counts, im.dtc.in<char>(g), b_dc, d_sel, f, n, st);
      launch_carry_gather(a.d_start3, g_s3, 3 * 8, d_sel, f, n, st);
      HIP_TRY(hipGetLastError());
      cv.batch = n;
      if (int rc = cilqr_dp_plan_batch_impl(h, a.dp_cfg, &cv, g_s3, a.n_knots, g_c9, g_c6, g_k3, g_stn, g_found, nullptr, nullptr))
        return rc;
      launch_carry_scatter(a.d_coarse9, g_c9, K * CILQR_COARSE_FIELDS * 8, d_sel, f, n, st);
      launch_carry_scatter(a.d_coarse6, g_c6, K * 6 * 8, d_sel, f, n, st);
      launch_carry_scatter(a.d_knots3, g_k3, K * 3 * 8, d_sel, f, n, st);
      launch_carry_scatter(a.d_station, g_stn, K * 8, d_sel, f, n, st);
      launch_carry_scatter(a.d_found, g_found, 4, d_sel, f, n, st);
      HIP_TRY(hipGetLastError());
    }
    return CILQR_OK;
  }
};

}  // namespace

extern "C" int cilqr_plan_scenes_batch_carry(cilqr_handle h, const cilqr_dp_config* dp_cfg,
                                             const cilqr_corridor_config* corridor_cfg, const cilqr_scene_batch* scenes,
                                             const double* start4, int32_t n_knots, const cilqr_carry* carry,
                                             const cilqr_warm_start* warm, cilqr_solution_batch* out, double* plan,
                                             double* coarse9, int32_t* outcome, int32_t* source, int32_t* n_dp_failed,
                                             int32_t* n_corridor_failed, int32_t* n_kept) {
  if (carry == nullptr)   // cilqr_plan_scenes_batch_warm: source and n_kept are left as they are
    return plan_scenes(h, dp_cfg, corridor_cfg, scenes, start4, n_knots, warm, nullptr, out, plan, coarse9, outcome,
                       n_dp_failed, n_corridor_failed);
  CarryStage stage(*carry, source);
  const int rc = plan_scenes(h, dp_cfg, corridor_cfg, scenes, start4, n_knots, warm, &stage, out, plan, coarse9, outcome,
                             n_dp_failed, n_corridor_failed);
  if (rc == CILQR_OK && n_kept) *n_kept = scenes->batch - stage.n_sel;
  return rc;
}
