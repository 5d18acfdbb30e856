// Private to cilqr_amd/csrc: what scene_window_batch.hip (the entry point) and kernels_scene_window.hip share -- the
// parameters of a launch and the launch function.  Every pointer of the launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"

namespace cilqr {

struct SceneWindowParams {
  int batch, max_dynamic;   // B, D slots per scene
  int max_samples;          // samples stored per source trajectory (any positive value)
  int out_samples;          // samples stored per window
  double span;
};

// src [B][D][max_samples][4] with src_counts [B][D], t0 [B]; out [B][D][out_samples][4] with out_counts [B][D]; ok [B]
// (NULL to skip); *n_failed += the scenes with a window count < 0.  Aligned as doubles, no more is assumed.
void launch_scene_window(const SceneWindowParams& P, const double* src, const int* src_counts, const double* t0, double* out,
                         int* out_counts, int* ok, int* n_failed, hipStream_t st);
// its second kernel alone (k_scene_window_ok), for the other calls that report counts this way (kernels_scene_predict.hip)
void launch_scene_window_ok(int batch, int max_dynamic, const int* out_counts, int* ok, int* n_failed, hipStream_t st);

}  // namespace cilqr
