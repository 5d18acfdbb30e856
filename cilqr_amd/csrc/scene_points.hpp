// Private to cilqr_amd/csrc: what scene_pipeline.hip (host side of cilqr_scene_points_batch / cilqr_plan_scenes_batch)
// and kernels_scene_points.hip share -- the sizes of a points launch and the launch functions.  Every pointer is device
// memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"

namespace cilqr {

struct ScenePointsParams {
  int n_knots;
  int max_static, max_dynamic, max_vertices, max_samples;   // of the cilqr_scene_batch
  int max_points;                                           // points stored per knot in the output
  int per_vertex;                                           // 1: the polygons' corners; 6: Polygon2d::sample_points
};

// Scenes [first, first + n_scenes) of `dv`, the batch with its arrays on the device; the outputs start at the FIRST of
// these scenes: points [n_scenes][K][max_points][2], point_count [n_scenes][K], scene_ok [n_scenes] (may be null).
void launch_scene_points(const ScenePointsParams& P, const cilqr_scene_batch& dv, int first, int n_scenes,
                         const double* times, double* points, int* point_count, int* scene_ok, hipStream_t st);

// start4 [B][4] x y theta v  ->  start3 [B][3] x y theta (the start of cilqr_dp_plan_batch)
void launch_plan_start3(int B, const double* start4, double* start3, hipStream_t st);
// outcome [B] of the batched TrajectoryPlanner::Plan from found [B] and corridor_count [B][K]; a scene the DP found no
// path for gets corridor_count -5 at knot 0; counts [2] += the scenes with outcome 1 / 2
void launch_plan_outcome(int B, int K, const int* found, int* corridor_count, int* outcome, int* counts, hipStream_t st);
// traj [B][K][CILQR_TRAJ_FIELDS] -> plan [B][K][CILQR_PLAN_FIELDS] (trajectory_planner.cpp:101-125)
void launch_plan_rows(int B, int K, const double* traj, double* plan, hipStream_t st);

}  // namespace cilqr
