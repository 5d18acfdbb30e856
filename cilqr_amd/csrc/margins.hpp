// Private to cilqr_amd/csrc: what margins_batch.hip (the entry points) and kernels_margins.hip share -- the parameters of
// a launch, the launch functions -- and the device statement of the plane
// arithmetic the margins are taken from: ShrinkConstraints + NormalizeHalfPlane as k_load_corridor / k_load_lanes
// (kernels_load.hip) evaluate them, written a second time here so that the load kernels stay as they are;
// tests/test_gpu_margins.py pins the two copies to each other through cilqr_stage_read.
// Every pointer of a launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"
#include "dev_model.hpp"

namespace cilqr {

constexpr int kMgLanes = 256;       // lanes of a workgroup
constexpr int kMgKnotTile = 128;    // knots of a problem in LDS at a time

struct MarginParams {
  Params p;              // the handle's: bounds, disc_off, shrink_corridor, shrink_lane
  int exact_ties;        // CILQR_OPT_EXACT_LANE_TIES as in force
  int n_knots, cmax;     // of the call's problem batch
  StateColumns rows;     // what the rule reads of a row (row_layouts.hpp)
  double tol[CILQR_MARGIN_FIELDS];
};

// the problems [b0, b0 + n) of a call and the prepared lane rows they share: [nl + nr][kLaneFields], left rows first
struct MarginGroup {
  int b0, n, nl, nr;
  const double* lanes;
};

// raw [n][7] rows of the left and of the right table -> prepared rows (the eleven fields of k_load_lanes)
void launch_margin_lanes(const double* raw_left, int nl, const double* raw_right, int nr, double shrink, double* prepared,
                         hipStream_t st);
// one workgroup per problem of the group.  margins [B][K][8] and which [B][K][6] may be null; n_violating (one int, zeroed
// by the caller) += the problems with a non-zero mask
void launch_margins(const MarginParams& P, const MarginGroup& G, const double* rows, const double* corridor, const int* count,
                    double* margins, int* which, double* min_margin, int* min_knot, uint32_t* violated, int* n_violating,
                    hipStream_t st);

// ---- the plane arithmetic (cc:438-495)
// (a, b, c) moved inwards by `shrink` metres and divided by its 3-norm
CILQR_DEV void mg_shrink_normalise(double a, double b, double c, double shrink, double* pa, double* pb, double* pc) {
  c = c - shrink * (a * a + b * b) / hypot_ref(a, b);     // cc:448, 463
  const double nrm = hypot_ref(hypot_ref(a, b), c);       // cc:479
  *pa = a / nrm;
  *pb = b / nrm;
  *pc = c / nrm;
}
// the corridor's rule for a live plane with a non-finite coefficient (k_load_corridor): kept as (0, 0, -inf)
CILQR_DEV void mg_guard_plane(double* pa, double* pb, double* pc) {
  if (!(__builtin_isfinite(*pa) && __builtin_isfinite(*pb) && __builtin_isfinite(*pc))) {
    *pa = 0.0;
    *pb = 0.0;
    *pc = -__builtin_huge_val();
  }
}
CILQR_DEV double mg_no_nan(double m) { return m != m ? -__builtin_huge_val() : m; }
// metres by which (px, py) is inside the normalised plane; h = hypot_ref(a, b)
CILQR_DEV double mg_plane_margin(double a, double b, double c, double h, double px, double py) {
  const double g = a * px + b * py - c;
  return mg_no_nan(-g / h);
}
// min(-g1, -g2) of a bound family, the first of equals
CILQR_DEV double mg_pair_margin(double g1, double g2) {
  const double m1 = mg_no_nan(-g1), m2 = mg_no_nan(-g2);
  return m2 < m1 ? m2 : m1;
}

}  // namespace cilqr
