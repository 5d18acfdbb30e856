// Private to cilqr_amd/csrc: what scene_pipeline.hip (cilqr_plan_scenes_batch / _warm) and carry_pipeline.hip
// (cilqr_plan_scenes_batch_carry) share -- the body of the pipeline, and the place where a caller may put another coarse
// stage than the DP planner on the whole batch.
#pragma once
#include "scene_batch.hpp"

namespace cilqr {

// what the pipeline hands its coarse stage: the scenes as the caller gave them (`sb`) and with their arrays on the device
// (`dv`), the start states, and where the stage's results go -- all device memory, all of the whole batch
struct CoarseArgs {
  cilqr_solver* h;
  const cilqr_dp_config* dp_cfg;
  const cilqr_scene_batch *sb, *dv;
  int n_knots;
  const double* d_start4;   // [B][4]
  double* d_start3;         // [B][3] work space for the planner's start states
  double *d_coarse9;        // [B][K][9] or null: the caller did not ask for it
  double *d_coarse6, *d_knots3, *d_station;
  int* d_found;             // [B]
  double* times;            // HOST [K]: the time column every scene's coarse trajectory has
};

// A coarse stage fills every array of CoarseArgs as cilqr_dp_plan_batch_impl does and leaves the stream waited for.
struct CoarseStage {
  virtual ~CoarseStage() = default;
  // with the pipeline's other checks, before anything is launched
  virtual int check(const cilqr_dp_config& dp_cfg, const cilqr_scene_batch& sb, int n_knots) = 0;
  virtual int run(const CoarseArgs& a) = 0;
};

// the body of the pipeline's entry points; `warm` NULL: the plain call; `coarse` NULL: DpPlanner::Plan for every scene
int plan_scenes(cilqr_handle h, const cilqr_dp_config* dp_cfg, const cilqr_corridor_config* corridor_cfg,
                const cilqr_scene_batch* scenes, const double* start4, int32_t n_knots, const cilqr_warm_start* warm,
                CoarseStage* coarse, cilqr_solution_batch* out, double* plan, double* coarse9, int32_t* outcome,
                int32_t* n_dp_failed, int32_t* n_corridor_failed);

}  // namespace cilqr
