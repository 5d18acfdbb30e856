// Private to cilqr_amd/csrc: what carry_batch.hip (cilqr_carry_rows / cilqr_carry_rows_batch), carry_pipeline.hip
// (cilqr_plan_scenes_batch_carry) and kernels_carry.hip share -- the parameters of a launch and the launch functions.  Every
// pointer of a launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"

struct cilqr_solver;

namespace cilqr {

struct CarryParams {
  int batch, n_rows;      // B, rows per trajectory (2 ... CILQR_DP_MAX_KNOTS)
  int fields;             // 9, 10 or 11: the layout (row_layouts.hpp)
  int n_knots, n_live;    // rows per trajectory in the outputs; the first n_live are produced, the others are zero
  double max_advance, delta_t;
};

// rows [B][n_rows][fields], advance [B] -> coarse9 / coarse6 / knots3 / station [B][n_knots][9 | 6 | 3 | 1] (each may be
// null), state [B]; *n_kept += the trajectories with state 0.  Aligned as doubles, no more is assumed.
void launch_carry(const CarryParams& P, const double* rows, const double* advance, double* coarse9, double* coarse6,
                  double* knots3, double* station, int* state, int* n_kept, hipStream_t st);

// source [B] of cilqr_plan_scenes_batch_carry (include/cilqr.h, "select") from state [B], start4 [B][4], the carried
// coarse9 [B][n_knots][9] and the audit's first_hit [B]; sel: the scenes with a non-zero source in ascending order,
// *n_sel: how many.  `found` [B] = 1 for a kept scene, 0 for a listed one (the planner writes those).
void launch_carry_select(int B, int n_knots, const int* state, const double* start4, const double* coarse9,
                         const int* first_hit, double max_start_offset, int* source, int* found, int* sel, int* n_sel,
                         hipStream_t st);

// n blocks of `per` elements of T between a packed array and the places sel[first ... first + n) name in a full one:
// gather (full -> packed) or scatter (packed -> full).  Nothing for a null array.
void launch_carry_gather(const void* full, void* packed, size_t per_bytes, const int* sel, int first, int n, hipStream_t st);
void launch_carry_scatter(void* full, const void* packed, size_t per_bytes, const int* sel, int first, int n, hipStream_t st);

// cilqr_carry_rows_batch with n_live of the n_knots rows produced (carry_batch.hip); the public call passes n_knots
int carry_rows_batch_impl(cilqr_solver* h, int32_t batch, int32_t layout, const double* rows, int32_t n_rows,
                          const double* advance, double max_advance, int32_t n_knots, int32_t n_live, double delta_t,
                          double* coarse9, double* coarse6, double* knots3, double* station, int32_t* state,
                          int32_t* n_kept, int32_t memory);
// what the carry calls check about one trajectory's shape and the limits
int check_carry_arguments(int32_t layout, int32_t n_rows, double max_advance);

}  // namespace cilqr
