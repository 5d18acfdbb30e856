// Private to cilqr_amd/csrc: what scene_predict_batch.hip (the entry point), host_planner.hip (the host call) and
// kernels_scene_predict.hip share -- the checks on the rule's arguments, the parameters of a launch and the launch function.
// Every pointer of the launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/cilqr.h"
#include "../../include/cilqr/scene_predict.hpp"

namespace cilqr {

// what both prediction calls check about the rule's arguments (include/cilqr.h, "scene prediction")
inline int check_prediction(double span, int mode, double max_age, double sample_dt, int out_samples) {
  if (!std::isfinite(span) || span < 0.0) return CILQR_ERR_ARG;
  if (mode != CILQR_PREDICT_HOLD && mode != CILQR_PREDICT_CONSTANT_VELOCITY) return CILQR_ERR_ARG;
  if (!std::isfinite(max_age) || max_age < 0.0) return CILQR_ERR_ARG;
  if (!std::isfinite(sample_dt) || !(sample_dt > 0.0) || out_samples < 2) return CILQR_ERR_ARG;
  if (!scene_predict::covers(out_samples, sample_dt, span)) return CILQR_ERR_ARG;
  return CILQR_OK;
}

struct ScenePredictParams {
  int batch, max_dynamic;   // B, D slots per scene
  int max_samples;          // samples stored per source trajectory (any positive value)
  int out_samples;          // samples written per predicted trajectory
  int mode;                 // CILQR_PREDICT_*
  double max_age, sample_dt;
};

// src [B][D][max_samples][4] with src_counts [B][D], t0 [B]; out [B][D][out_samples][4] with out_counts [B][D]; ok [B]
// (NULL to skip); *n_failed += the scenes with a count < 0.  Aligned as doubles, no more is assumed.
void launch_scene_predict(const ScenePredictParams& P, const double* src, const int* src_counts, const double* t0, double* out,
                          int* out_counts, int* ok, int* n_failed, hipStream_t st);

}  // namespace cilqr
