// cilqr_constraint_margins / cilqr_constraint_margins_batch (include/cilqr.h, "constraint margins"): the host call around
// include/cilqr/constraint_margins.hpp, and the host side of the batched one -- argument checks, the lane tables of every
// group on their way to the device, staging of HOST arrays, the launches of kernels_margins.hip, the count's way back.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/cilqr/constraint_margins.hpp"
#include "scene_batch.hpp"
#include "margins.hpp"

using namespace cilqr;
namespace cm = cilqr::constraint_margins;

namespace {

// the lane groups of a problem batch, as cilqr_solve_batch reads them: problems [b0, b1) use nl rows of left_lane from row
// l0 and nr rows of right_lane from row r0
struct LaneGroup {
  int b0, b1, nl, nr;
  size_t l0, r0;
};

// What both calls check on their own arguments, in the order of the audit calls; *groups on success.  smax < 0: no limit.
int check_margin_call(const cilqr_problem_batch* in, int32_t layout, const double* rows, const double* min_margin,
                      const int32_t* min_knot, const double* tol, const uint32_t* violated, int cmax_cap, int smax,
                      std::vector<LaneGroup>* groups) {
  if (in == nullptr || rows == nullptr || min_margin == nullptr || min_knot == nullptr || violated == nullptr)
    return CILQR_ERR_NULL;
  if (in->batch < 1 || in->n_knots < 1 || state_columns(layout).fields == 0) return CILQR_ERR_ARG;
  if (in->memory != CILQR_MEM_HOST && in->memory != CILQR_MEM_DEVICE) return CILQR_ERR_ARG;
  if (tol != nullptr)
    for (int f = 0; f < CILQR_MARGIN_FIELDS; ++f)
      if (!std::isfinite(tol[f]) || !(tol[f] >= 0.0)) return CILQR_ERR_ARG;
  if (in->corridor == nullptr || in->corridor_count == nullptr || in->left_lane == nullptr || in->right_lane == nullptr ||
      in->cmax <= 0)
    return CILQR_ERR_CONSTRAINTS;   // as a solve (cc:68-73)
  groups->clear();
  if (in->n_lane_groups <= 1) {
    if (in->n_left <= 0 || in->n_right <= 0) return CILQR_ERR_CONSTRAINTS;
    groups->push_back(LaneGroup{0, in->batch, in->n_left, in->n_right, 0, 0});
  } else {
    if (in->lane_group_start == nullptr || in->lane_group_left == nullptr || in->lane_group_right == nullptr)
      return CILQR_ERR_CONSTRAINTS;
    if (in->lane_group_start[0] != 0 || in->lane_group_start[in->n_lane_groups] != in->batch) return CILQR_ERR_ARG;
    size_t l0 = 0, r0 = 0;
    for (int g = 0; g < in->n_lane_groups; ++g) {
      const int b0 = in->lane_group_start[g], b1 = in->lane_group_start[g + 1];
      const int nl = in->lane_group_left[g], nr = in->lane_group_right[g];
      if (b0 < 0 || b1 < b0 || b1 > in->batch || nl <= 0 || nr <= 0) return CILQR_ERR_ARG;
      groups->push_back(LaneGroup{b0, b1, nl, nr, l0, r0});
      l0 += (size_t)nl;
      r0 += (size_t)nr;
    }
  }
  if (cmax_cap >= 0 && in->cmax > cmax_cap) return CILQR_ERR_CAPACITY;
  if (smax >= 0)
    for (const LaneGroup& g : *groups)
      if (g.nl > smax || g.nr > smax) return CILQR_ERR_CAPACITY;
  return CILQR_OK;
}

}  // namespace

extern "C" int cilqr_constraint_margins(const cilqr_config* cfg, int32_t exact_lane_ties, const cilqr_problem_batch* in,
                                        int32_t layout, const double* rows, double* margins, int32_t* which,
                                        double* min_margin, int32_t* min_knot, const double* tol, uint32_t* violated,
                                        int32_t* n_violating) {
  if (cfg == nullptr) return CILQR_ERR_NULL;
  std::vector<LaneGroup> groups;
  if (int rc = check_margin_call(in, layout, rows, min_margin, min_knot, tol, violated, -1, -1, &groups)) return rc;
  if (in->memory != CILQR_MEM_HOST) return CILQR_ERR_ARG;
  if (cfg->num_of_disc < 1 || cfg->num_of_disc > CILQR_MAX_DISCS) return CILQR_ERR_ARG;
  const cm::Vehicle V = cm::vehicle_of(*cfg);
  const size_t K = (size_t)in->n_knots, C = (size_t)in->cmax, F = (size_t)cm::columns_of(layout).fields;
  int32_t n_bad = 0;
  std::vector<cm::Segment> left, right;
  for (const LaneGroup& g : groups) {
    cm::prepare_lane(in->left_lane + g.l0 * CILQR_LANE_FIELDS, g.nl, V.shrink_lane, &left);
    cm::prepare_lane(in->right_lane + g.r0 * CILQR_LANE_FIELDS, g.nr, V.shrink_lane, &right);
    for (size_t b = (size_t)g.b0; b < (size_t)g.b1; ++b) {
      cm::problem_margins(V, exact_lane_ties != 0, layout, rows + b * K * F, in->n_knots, in->corridor + b * K * C * 3,
                          in->corridor_count + b * K, in->cmax, left, right,
                          margins ? margins + b * K * CILQR_MARGIN_FIELDS : nullptr,
                          which ? which + b * K * CILQR_MARGIN_WHICH_FIELDS : nullptr, min_margin + b * CILQR_MARGIN_FIELDS,
                          min_knot + b * CILQR_MARGIN_FIELDS);
      violated[b] = cm::violated_mask(min_margin + b * CILQR_MARGIN_FIELDS, tol);
      if (violated[b] != 0) ++n_bad;
    }
  }
  if (n_violating != nullptr) *n_violating = n_bad;
  return CILQR_OK;
}

extern "C" int cilqr_constraint_margins_batch(cilqr_handle h, const cilqr_problem_batch* in, int32_t layout, const double* rows,
                                              double* margins, int32_t* which, double* min_margin, int32_t* min_knot,
                                              const double* tol, uint32_t* violated, int32_t* n_violating) {
  if (h == nullptr) return CILQR_ERR_NULL;
  std::vector<LaneGroup> groups;
  if (int rc = check_margin_call(in, layout, rows, min_margin, min_knot, tol, violated, h->cmax, h->smax, &groups)) return rc;
  if (solves_in_flight(h)) return CILQR_ERR_STATE;

  MarginParams P;
  std::memset(&P, 0, sizeof(P));
  P.p = h->ds.p;
  P.exact_ties = h->ds.exact_ties;
  P.n_knots = in->n_knots;
  P.cmax = in->cmax;
  P.rows = state_columns(layout);
  for (int f = 0; f < CILQR_MARGIN_FIELDS; ++f) P.tol[f] = tol ? tol[f] : 0.0;

  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t B = (size_t)in->batch, K = (size_t)in->n_knots, C = (size_t)in->cmax, F = (size_t)P.rows.fields;
  size_t n_left = 0, n_right = 0;
  for (const LaneGroup& g : groups) {
    n_left += (size_t)g.nl;
    n_right += (size_t)g.nr;
  }
  // ---- the count, the lane tables (raw on their way in, prepared behind them) and, HOST arrays, a block in and a block
  // out: the handle's work space (grown, never shrunk)
  staged_call c(h, h->mg, in->memory == CILQR_MEM_HOST, st);
  const double *d_rows, *d_cor, *d_left, *d_right;
  const int* d_cnt;
  double *d_marg, *d_min, *d_prepared;
  int *d_which, *d_knot, *d_count;
  uint32_t* d_viol;
  c.counter(&d_count);
  c.table(in->left_lane, n_left * CILQR_LANE_FIELDS, &d_left);
  c.table(in->right_lane, n_right * CILQR_LANE_FIELDS, &d_right);
  c.scratch((n_left + n_right) * kLaneFields, &d_prepared);
  c.in(rows, B * K * F, &d_rows);
  c.in(in->corridor, B * K * C * 3, &d_cor);
  c.in(in->corridor_count, B * K, &d_cnt);
  c.out(margins, B * K * CILQR_MARGIN_FIELDS, &d_marg);
  c.out(which, B * K * CILQR_MARGIN_WHICH_FIELDS, &d_which);
  c.out(min_margin, B * CILQR_MARGIN_FIELDS, &d_min);
  c.out(min_knot, B * CILQR_MARGIN_FIELDS, &d_knot);
  c.out(violated, B, &d_viol);
  if (int rc = c.stage()) return rc;
  for (const LaneGroup& g : groups) {
    if (g.b1 == g.b0) continue;
    double* prepared = d_prepared + (g.l0 + g.r0) * kLaneFields;
    launch_margin_lanes(d_left + g.l0 * CILQR_LANE_FIELDS, g.nl, d_right + g.r0 * CILQR_LANE_FIELDS, g.nr, P.p.shrink_lane,
                        prepared, st);
    const MarginGroup G{g.b0, g.b1 - g.b0, g.nl, g.nr, prepared};
    launch_margins(P, G, d_rows, d_cor, d_cnt, d_marg, d_which, d_min, d_knot, d_viol, d_count, st);
  }
  HIP_TRY(hipGetLastError());
  return c.finish(n_violating);
}
