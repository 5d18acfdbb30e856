// Private to cilqr_amd/csrc: what stop_batch.hip (cilqr_stop_rows / cilqr_stop_rows_batch), stop_pipeline.hip
// (cilqr_stop_scenes_batch) and kernels_stop.hip share -- the parameters of a launch and the launch functions.  Every
// pointer of a launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"

struct cilqr_solver;

namespace cilqr {

struct StopParams {
  int batch, n_knots;     // B, rows per trajectory (2 ... CILQR_DP_MAX_KNOTS)
  int fields;             // 9, 10 or 11: the layout (row_layouts.hpp)
  int n_profiles, n_out;  // M (1 ... CILQR_STOP_MAX_PROFILES), rows per chain (1 ... CILQR_DP_MAX_KNOTS)
  double delta_t;
  double profile[CILQR_STOP_MAX_PROFILES][2];   // a_target, jerk
};

// rows [B][n_knots][fields], start_va [B][2] or null -> out_rows [M][B][n_out][11], status / stop_knot / travel [M][B] (each
// may be null).  Aligned as doubles, no more is assumed.
void launch_stop(const StopParams& P, const double* rows, const double* start_va, double* out_rows, int* status,
                 int* stop_knot, double* travel, hipStream_t st);

// choice [B] from status / first_hit [M][B]: the smallest m with STOPPED and no hit, else -1; out_rows [B][per] = slice
// choice[b] of slices [M][B][per], slice M - 1 where there is none; *n_none (may be null) = the scenes without a choice
void launch_stop_choose(int B, int M, size_t per, const int* status, const int* first_hit, const double* slices, int* choice,
                        double* out_rows, int* n_none, hipStream_t st);

// what the stop calls check about one trajectory's shape, the profiles (HOST) and the rows asked for
int check_stop_arguments(int32_t layout, int32_t n_knots, int32_t n_profiles, const double* profiles, double delta_t,
                         int32_t n_out);
// the body of cilqr_stop_rows_batch (stop_batch.hip), which the pipeline calls on device views
int stop_rows_batch_impl(cilqr_solver* h, int32_t batch, int32_t layout, const double* rows, int32_t n_knots,
                         int32_t n_profiles, const double* profiles, const double* start_va, double delta_t, int32_t n_out,
                         double* out_rows, int32_t* status, int32_t* stop_knot, double* travel, int32_t memory);

}  // namespace cilqr
