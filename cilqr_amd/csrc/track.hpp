// Private to cilqr_amd/csrc: what track_batch.hip (the two entry points) and kernels_track.hip share -- the parameters of
// a launch, the follow table and the launch functions.  Every pointer of a launch is device memory; nothing here
// synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"
#include "state.hpp"

namespace cilqr {

// The follow table of a call: what the tracker's rule reads of the caller's rows, batch-fastest, so that the 64 lanes of a
// wave (one problem each) read one contiguous kilobyte per load -- the layout k_init_guess_tracker reads `goals` in.
// stride = the batch rounded up to 64 problems.
struct FollowTable {
  int stride;
  double2* xy;      // [K][stride]  x, y
  double2* thv;     // [K][stride]  theta, v
  double2* ts;      // [K][stride]  time, station
  double2* start;   // [3][stride]  (x, y) (theta, v) (a, delta) of the start state
};
inline size_t follow_table_stride(int batch) { return ((size_t)batch + 63) / 64 * 64; }
inline size_t follow_table_bytes(int batch, int n_knots) { return follow_table_stride(batch) * (3 * (size_t)n_knots + 3) * 16; }
// the table's arrays laid out in `block` (256-byte aligned, follow_table_bytes long)
inline FollowTable follow_table_in(void* block, int batch, int n_knots) {
  FollowTable t;
  const size_t S = follow_table_stride(batch), K = (size_t)n_knots;
  t.stride = (int)S;
  t.xy = static_cast<double2*>(block);
  t.thv = t.xy + K * S;
  t.ts = t.thv + K * S;
  t.start = t.ts + K * S;
  return t;
}

struct TrackParams {
  int batch, n_knots, n_drive;   // B, K >= 2, 1 ... K
  int fields;                    // 10, 11 or 9: the layout (CILQR_ROWS_TRAJ / _PLAN / _COARSE)
  int max_steps;                 // CILQR_TRACKER_MAX_SIM_STEPS
};

// rows [B][K][fields], start6 [B][6] or nullptr -> the table; aligned as doubles, no more is assumed
void launch_track_gather(const TrackParams& P, const double* rows, const double* start6, const FollowTable& tab, hipStream_t st);
// the table -> driven [B][n_drive][10], ok [B]; *n_failed (zeroed by the caller) += the problems with ok = 0
void launch_track_rows(const TrackParams& P, const Params& vehicle, const TrackerParams& tp, const FollowTable& tab,
                       double* driven, int* ok, int* n_failed, hipStream_t st);

}  // namespace cilqr
