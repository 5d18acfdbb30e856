// Total cost of a trajectory from its per-knot partials (dev_model.hpp declares reduce_cost), and the rows of the line
// search's candidate arena: where a candidate's knots and partials live, stated once for the kernels that write, cost, sum
// and adopt them (search_core.hpp, kernels_quad.hip, kernels_search.hip, kernels_tail.hip).
#pragma once
#include "dev_model.hpp"
#include "ref_order.hpp"

namespace cilqr {

// Sum of a trajectory's knot partials in index order -> c5 (total, J, dynamics, corridor, lane).  pb: pair 0 of knot 0;
// the three pairs of a knot lie `stride` apart, knots kPartPairs x stride (quad_core.hpp, knot_cost, writes them).
CILQR_DEV void sum_partials(const double2* pb, size_t stride, int K, int N, double* c5) {
  double j = 0.0, dx = 0.0, du = 0.0, cc = 0.0, lc = 0.0;
  // loads of several knots in flight; the sums stay in knot order
#pragma unroll 8
  for (int i = 0; i < K; ++i) {
    const double2* o = pb + (size_t)i * kPartPairs * stride;
    const double2 a = o[0], c = o[2 * stride];     // (J, bounds) of the state; (corridor, lane)
    j += a.x;
    dx += a.y;
    cc += c.x;
    lc += c.y;
  }
#pragma unroll 8
  for (int i = 0; i < N; ++i) {   // control terms follow the state terms (cc:510-513)
    const double2 b = pb[((size_t)i * kPartPairs + 1) * stride];   // (J, bounds) of the control
    j += b.x;
    du += b.y;
  }
  const double dyn = dx + du;                      // cc:550
  c5[0] = j + dyn + cc + lc;                       // cc:429
  c5[1] = j; c5[2] = dyn; c5[3] = cc; c5[4] = lc;
}

CILQR_DEV void reduce_cost(const DeviceState& s, int slot, int cand, double* c5) {
#ifdef CILQR_REF_ORDER
  const int buf = s.cur[slot] ^ cand;
  reforder::total_cost(
      s, slot, [&](int i, double* x) { load_x(s, buf, i, slot, x); }, [&](int i, double* u) { load_u(s, buf, i, slot, u); }, c5);
#else
  (void)cand;
  sum_partials(s.part + slot, (size_t)s.Bcap, s.p.K, s.p.N, c5);
#endif
}

// ---- the candidate arena (DeviceState::Xs, Us, parts): [r][K][3][cap], [r][N][cap], [r][K][kPartPairs][cap] ----
// r: step size, i: knot, j: list position, cap: row stride -- s.spec_cap, or the literal 1 (with j = 0) where a problem is
// alone in its arena and the strides are to be compile-time constants (kernels_tail.hip).  Offsets in pairs: of pair 0 of
// the knot's three, which lie `cap` apart (Xs, parts), or of its one pair (Us).  The host's views of the arena (kernels_search.hip,
// spec_view) move the base pointers by whole rows of these.
__host__ __device__ __forceinline__ size_t cand_x_at(const Params& p, size_t cap, int r, int i, int j) {
  return ((size_t)r * p.K + i) * 3 * cap + j;
}
__host__ __device__ __forceinline__ size_t cand_u_at(const Params& p, size_t cap, int r, int i, int j) {
  return ((size_t)r * p.N + i) * cap + j;
}
__host__ __device__ __forceinline__ size_t cand_parts_at(const Params& p, size_t cap, int r, int i, int j) {
  return ((size_t)r * p.K + i) * kPartPairs * cap + j;
}

// knot i of candidate alpha_r at position j; the last knot has no control
CILQR_DEV void load_candidate_knot(const DeviceState& s, size_t cap, int r, int i, int j, double* x, double* u) {
  const double2* xb = s.Xs + cand_x_at(s.p, cap, r, i, j);
  const double2 p0 = xb[0], p1 = xb[cap], p2 = xb[2 * cap];
  x[0] = p0.x; x[1] = p0.y; x[2] = p1.x; x[3] = p1.y; x[4] = p2.x; x[5] = p2.y;
  u[0] = 0.0; u[1] = 0.0;
  if (i < s.p.N) {
    const double2 q = s.Us[cand_u_at(s.p, cap, r, i, j)];
    u[0] = q.x; u[1] = q.y;
  }
}
// where knot_cost puts the partials of that knot
CILQR_DEV double2* candidate_parts(const DeviceState& s, size_t cap, int r, int i, int j) {
  return s.parts + cand_parts_at(s.p, cap, r, i, j);
}
// the accepted candidate becomes the iterate: its knot i -> buffer nb of slot (Bc: the iterates' stride, s.Bcap or the literal 1)
CILQR_DEV void adopt_candidate_knot(const DeviceState& s, size_t cap, size_t Bc, int r, int i, int j, int nb, int slot) {
  const double2* xb = s.Xs + cand_x_at(s.p, cap, r, i, j);
  double2* o = s.X + ((size_t)nb * s.p.K + i) * 3 * Bc + slot;
  o[0] = xb[0];
  o[Bc] = xb[cap];
  o[2 * Bc] = xb[2 * cap];
  if (i < s.p.N) s.U[((size_t)nb * s.p.N + i) * Bc + slot] = s.Us[cand_u_at(s.p, cap, r, i, j)];
}

// total cost of candidate alpha_r at list position j (of `slot`): its knot partials summed in index order
CILQR_DEV void candidate_total(const DeviceState& s, int slot, int r, int j, double* c5) {
#ifdef CILQR_REF_ORDER
  const size_t cap = (size_t)s.spec_cap;
  double x_[6], u_[2];   // the half of a knot the other walk reads
  reforder::total_cost(
      s, slot, [&](int i, double* x) { load_candidate_knot(s, cap, r, i, j, x, u_); },
      [&](int i, double* u) { load_candidate_knot(s, cap, r, i, j, x_, u); }, c5);
#else
  (void)slot;
  sum_partials(candidate_parts(s, (size_t)s.spec_cap, r, 0, j), (size_t)s.spec_cap, s.p.K, s.p.N, c5);
#endif
}

// ---- entries of a pre-rolled round (kernels_search.hip): round r0 works on the problems that rejected alpha_0 .. alpha_{r0-1} ----
// Round 0 takes the active list itself (entry e is position e); a later round takes pending list r0, which holds POSITIONS
// in the active list -- a candidate's place in the arena -- on lists 1 .. R-1 of R pre-rolled rounds and SLOTS on list R,
// which is what the speculative pass over the remaining step sizes takes (k_round_pick's `last`).  The round-by-round
// schedule (k_search_round) rolls into the iterates' own buffers and keeps slots on every list.
CILQR_DEV int round_count(const DeviceState& s, int r0, int n_max) {
  return (r0 == 0) ? active_count(s, n_max) : min(s.counters[r0], n_max);
}
// entry e of round r0 -> its position (returned) and slot
CILQR_DEV int round_entry(const DeviceState& s, int r0, int e, int& slot) {
  const int j = (r0 == 0) ? e : s.pend[(size_t)r0 * s.Bcap + e];
  slot = s.act[j];
  return j;
}

}  // namespace cilqr
