// How far every knot of a batch of trajectories stays inside the constraints of its own solve (C-ABI:
// cilqr_constraint_margins_batch; the rule is stated once, in include/cilqr.h under "constraint margins"; the host statement
// is include/cilqr/constraint_margins.hpp).  The plane arithmetic is margins.hpp's, the heading goes through the cost
// kernels' lean_sincos, hypot is dev_model.hpp's libm-identical hypot_ref, the nearest lane segment is
// nearest_segment_scan, the reference's linear scan with its exact-tie rule.
//
// k_margin_lanes.  One lane per lane row of a group: the eleven fields of k_load_lanes (shrunk, normalised plane, the
// segment's frame, the identities of its end points).
//
// k_margins.  ONE WORKGROUP PER PROBLEM.  The bytes are the planes: [K][cmax][3] doubles per problem, 19.6 KB at K = 51,
// cmax = 16, against 4 KB of rows -- they are read where they lie, once, as contiguous 24-byte records.
//   * the group's prepared lane rows are staged in LDS once (dynamic: (nl + nr) rows of eleven doubles);
//   * the knots pass in tiles of kMgKnotTile: one lane per knot reads its row, leaves x, y, cos, sin in LDS and the five
//     bound families in the knot's result row;
//   * the lanes stride over the (knot, plane) pairs of the tile, the planes of a knot padded to a power of two G <= 64:
//     pair p = knot * G + plane, so consecutive lanes read consecutive records.  A pair's lane shrinks and normalises its
//     plane ONCE and applies it to the D discs.  The rule's order -- discs outside, planes inside, strict `<` from +inf --
//     is the lexicographic minimum of (margin, disc * cmax + plane): kept per lane, then taken over the G neighbouring
//     lanes by log2 G butterfly steps (__shfl_xor).  No atomic, no dependence on the order of lanes or on the batch;
//   * the lanes stride over the (knot, side, disc) triples, as many whole groups of D discs per pass as the workgroup
//     holds (255 triples at D = 5: no lane is padding): a triple's lane scans the side's rows in LDS and takes the margin
//     to the nearest segment's plane; the D values of a group meet in LDS, where one lane walks them in the rule's own
//     order with its strict `<`;
//   * the tile's rows leave flat; eight groups of 32 lanes keep the running (margin, knot) minimum of the eight columns
//     over the tiles (ascending knots, strict `<`), and a last butterfly leaves the problem's minima, from which lane 0
//     takes the mask.
// Every index is bounded by the call's n_knots and cmax and by the group's nl + nr; a count is clamped to 0 ... cmax as
// k_load_corridor clamps it.  Built with -ffp-contract=off like every other file.
#include <climits>

#include "margins.hpp"

namespace cilqr {

namespace {

constexpr int kMgNone = INT_MAX;
static_assert(CILQR_MAX_DISCS <= kMgLanes, "a pass of the lane scan holds at least one group of discs");
static_assert(kMgKnotTile <= kMgLanes, "one lane per knot of a tile");

// the smallest (value, index) pair, compared lexicographically, among `group` neighbouring lanes (a power of two <= 64,
// every lane of the wavefront active): left in every lane of the group.  (+inf, kMgNone) is "nothing taken".
CILQR_DEV void mg_group_min(double* value, int* index, int group) {
  double v = *value;
  int at = *index;
  for (int w = 1; w < group; w <<= 1) {
    const double ov = __shfl_xor(v, w);
    const int oat = __shfl_xor(at, w);
    const bool take = ov < v || (ov == v && oat < at);
    v = take ? ov : v;
    at = take ? oat : at;
  }
  *value = v;
  *index = at;
}

CILQR_DEV int mg_log2_ceil(int n) {   // the power of two n items are padded to, as a shift
  int s = 0;
  while ((1 << s) < n) ++s;
  return s;
}

}  // namespace

__global__ __launch_bounds__(512) void k_margin_lanes(const double* __restrict__ raw_left, int nl,
                                                      const double* __restrict__ raw_right, int nr, double shrink,
                                                      double* __restrict__ prepared) {
  const int t = threadIdx.x;
  if (t >= nl + nr) return;
  const bool is_left = t < nl;
  const double* side = is_left ? raw_left : raw_right;
  const int n_side = is_left ? nl : nr, k_own = is_left ? t : t - nl;
  const double* r = side + (size_t)k_own * CILQR_LANE_FIELDS;
  double a, b, c;
  mg_shrink_normalise(r[0], r[1], r[2], shrink, &a, &b, &c);
  const double sx = r[3], sy = r[4], ex = r[5], ey = r[6];
  const double dx = ex - sx, dy = ey - sy;
  const double len = hypot_ref(dx, dy);
  double* o = prepared + (size_t)t * kLaneFields;
  o[0] = a; o[1] = b; o[2] = c;
  o[3] = sx; o[4] = sy;
  o[5] = (len <= kMathEps) ? 0.0 : dx / len;
  o[6] = (len <= kMathEps) ? 0.0 : dy / len;
  o[7] = len;
  o[8] = ex; o[9] = ey;
  // identities of the two end points within the side's table (see k_load_lanes): the smallest index of a point with
  // bitwise equal coordinates, which the exact-tie rule compares instead of coordinates
  auto same = [](double ax, double ay, double bx, double by) {
    return __double_as_longlong(ax) == __double_as_longlong(bx) && __double_as_longlong(ay) == __double_as_longlong(by);
  };
  int sid = 2 * k_own, eid = 2 * k_own + 1;
  for (int k = n_side - 1; k >= 0; --k) {
    const double* q = side + (size_t)k * CILQR_LANE_FIELDS;
    if (same(q[5], q[6], sx, sy)) sid = min(sid, 2 * k + 1);
    if (same(q[3], q[4], sx, sy)) sid = min(sid, 2 * k);
    if (same(q[5], q[6], ex, ey)) eid = min(eid, 2 * k + 1);
    if (same(q[3], q[4], ex, ey)) eid = min(eid, 2 * k);
  }
  o[10] = __longlong_as_double((long long)(unsigned)sid | ((long long)eid << 32));
}

__global__ __launch_bounds__(kMgLanes) void k_margins(MarginParams P, MarginGroup G, const double* __restrict__ rows,
                                                      const double* __restrict__ corridor, const int* __restrict__ count,
                                                      double* __restrict__ margins, int* __restrict__ which,
                                                      double* __restrict__ min_margin, int* __restrict__ min_knot,
                                                      uint32_t* __restrict__ violated, int* __restrict__ n_violating) {
  extern __shared__ double s_lanes[];                      // [nl + nr][kLaneFields]
  __shared__ double s_pose[kMgKnotTile * 4];               // x, y, cos, sin
  __shared__ double s_m[kMgKnotTile * CILQR_MARGIN_FIELDS];
  __shared__ int s_w[kMgKnotTile * CILQR_MARGIN_WHICH_FIELDS];
  __shared__ double s_disc_m[kMgLanes];                    // a pass of the lane scan: every disc's margin and segment
  __shared__ int s_disc_seg[kMgLanes];
  __shared__ double s_col_min[CILQR_MARGIN_FIELDS];
  __shared__ int s_col_knot[CILQR_MARGIN_FIELDS];

  const int tid = threadIdx.x;
  const size_t b = (size_t)G.b0 + blockIdx.x;
  const int K = P.n_knots, C = P.cmax, D = P.p.num_of_disc;
  const int F = P.rows.fields;
  const double inf = __builtin_huge_val();

  for (int i = tid; i < (G.nl + G.nr) * kLaneFields; i += kMgLanes) s_lanes[i] = G.lanes[i];

  const int plane_shift = mg_log2_ceil(min(C, 64)), plane_group = 1 << plane_shift;
  const int per_pass = (kMgLanes / D) * D;   // (knot, side, disc) triples of a pass: whole groups of D
  const int col = tid >> 5, col_lane = tid & 31;   // the running minimum of column `col`
  double run_m = inf;
  int run_k = kMgNone;

  for (int k0 = 0; k0 < K; k0 += kMgKnotTile) {
    const int kt = min(kMgKnotTile, K - k0);
    __syncthreads();   // the lane rows are there; the tile before this one has been read
    // ---- the poses and the bound families (cc:523-528, 543-546)
    if (tid < kt) {
      const double* __restrict__ row = rows + (b * K + (k0 + tid)) * F;
      double sn, cs;
      lean_sincos(row[P.rows.theta], &sn, &cs);
      double* pose = s_pose + tid * 4;
      pose[0] = row[P.rows.x]; pose[1] = row[P.rows.y]; pose[2] = cs; pose[3] = sn;
      const double v = row[P.rows.v], a = row[P.rows.a], delta = row[P.rows.delta];
      double* m = s_m + tid * CILQR_MARGIN_FIELDS;
      m[3] = mg_pair_margin(-v, v - P.p.max_velocity);
      m[4] = mg_pair_margin(a - P.p.max_acc, P.p.min_acc - a);
      m[5] = mg_pair_margin(delta - P.p.delta_max, P.p.delta_min - delta);
      if (P.rows.jerk >= 0 && k0 + tid < K - 1) {
        const double jerk = row[P.rows.jerk], rate = row[P.rows.rate];
        m[6] = mg_pair_margin(jerk - P.p.jerk_max, P.p.jerk_min - jerk);
        m[7] = mg_pair_margin(rate - P.p.delta_rate_max, P.p.delta_rate_min - rate);
      } else {
        m[6] = inf;
        m[7] = inf;
      }
    }
    __syncthreads();

    // ---- (knot, plane): cc:559-578.  The same trips in every lane: the butterfly needs them all
    for (int base = 0; base < (kt << plane_shift); base += kMgLanes) {
      const int p = base + tid;
      const int k = p >> plane_shift, c_first = p & (plane_group - 1);
      double best = inf;
      int at = kMgNone;
      if (k < kt) {
        const size_t knot = b * K + (k0 + k);
        const int n = max(0, min(count[knot], C));
        const double x = s_pose[4 * k], y = s_pose[4 * k + 1], cs = s_pose[4 * k + 2], sn = s_pose[4 * k + 3];
        const double* __restrict__ planes = corridor + knot * C * 3;
        for (int c = c_first; c < n; c += plane_group) {   // more than 64 planes: a lane takes several
          double pa, pb, pc;
          mg_shrink_normalise(planes[3 * c], planes[3 * c + 1], planes[3 * c + 2], P.p.shrink_corridor, &pa, &pb, &pc);
          mg_guard_plane(&pa, &pb, &pc);
          const double h = hypot_ref(pa, pb);
          for (int j = 0; j < D; ++j) {
            const double px = x + P.p.disc_off[j] * cs, py = y + P.p.disc_off[j] * sn;
            const double m = mg_plane_margin(pa, pb, pc, h, px, py);
            const int idx = j * C + c;
            if (m < best || (m == best && m < inf && idx < at)) {
              best = m;
              at = idx;
            }
          }
        }
      }
      mg_group_min(&best, &at, plane_group);
      if (k < kt && c_first == 0) {
        s_m[k * CILQR_MARGIN_FIELDS] = best;
        s_w[k * CILQR_MARGIN_WHICH_FIELDS] = at == kMgNone ? -1 : at / C;
        s_w[k * CILQR_MARGIN_WHICH_FIELDS + 1] = at == kMgNone ? -1 : at % C;
      }
    }

    // ---- (knot, side, disc): cc:589-618.  A pass takes as many whole (knot, side) groups of D discs as the workgroup holds
    for (int base = 0; base < kt * 2 * D; base += per_pass) {
      const int p = base + tid;
      double m = inf;
      int seg = 0;
      if (tid < per_pass && p < kt * 2 * D) {
        const int ks = p / D, j = p - ks * D;
        const int side = ks & 1, k = ks >> 1;
        const double px = s_pose[4 * k] + P.p.disc_off[j] * s_pose[4 * k + 2];
        const double py = s_pose[4 * k + 1] + P.p.disc_off[j] * s_pose[4 * k + 3];
        const double* tab = s_lanes + (side ? G.nl * kLaneFields : 0);
        seg = nearest_segment_scan(tab, side ? G.nr : G.nl, px, py, P.exact_ties != 0);
        const double* r = tab + seg * kLaneFields;
        const double a = r[0], bb = r[1], c = r[2];
        m = mg_plane_margin(a, bb, c, hypot_ref(a, bb), px, py);
      }
      s_disc_m[tid] = m;
      s_disc_seg[tid] = seg;
      __syncthreads();
      // one lane per group: the rule's own loop over the discs, strict `<` from +inf
      const int ks = base / D + tid;
      if (tid < per_pass / D && ks < kt * 2) {
        const int side = ks & 1, k = ks >> 1;
        double best = inf;
        int disc = -1, at = -1;
        for (int j = 0; j < D; ++j) {
          const double v = s_disc_m[tid * D + j];
          if (v < best) {
            best = v;
            disc = j;
            at = s_disc_seg[tid * D + j];
          }
        }
        s_m[k * CILQR_MARGIN_FIELDS + 1 + side] = best;
        s_w[k * CILQR_MARGIN_WHICH_FIELDS + 2 + 2 * side] = disc;
        s_w[k * CILQR_MARGIN_WHICH_FIELDS + 3 + 2 * side] = at;
      }
      __syncthreads();
    }

    // ---- the tile's rows leave flat
    if (margins != nullptr) {
      double* __restrict__ dst = margins + (b * K + k0) * CILQR_MARGIN_FIELDS;
      for (int i = tid; i < kt * CILQR_MARGIN_FIELDS; i += kMgLanes) dst[i] = s_m[i];
    }
    if (which != nullptr) {
      int* __restrict__ dst = which + (b * K + k0) * CILQR_MARGIN_WHICH_FIELDS;
      for (int i = tid; i < kt * CILQR_MARGIN_WHICH_FIELDS; i += kMgLanes) dst[i] = s_w[i];
    }
    // ---- the running minimum of every column: a lane meets its knots in ascending order, a strict `<` keeps the first
    for (int k = col_lane; k < kt; k += 32) {
      const double v = s_m[k * CILQR_MARGIN_FIELDS + col];
      if (v < run_m) {
        run_m = v;
        run_k = k0 + k;
      }
    }
  }
  mg_group_min(&run_m, &run_k, 32);
  if (col_lane == 0) {
    s_col_min[col] = run_m;
    s_col_knot[col] = run_k;
  }
  __syncthreads();
  if (tid < CILQR_MARGIN_FIELDS) {
    min_margin[b * CILQR_MARGIN_FIELDS + tid] = s_col_min[tid];
    min_knot[b * CILQR_MARGIN_FIELDS + tid] = s_col_knot[tid] == kMgNone ? -1 : s_col_knot[tid];
  }
  if (tid == 0) {
    uint32_t mask = 0;
    for (int f = 0; f < CILQR_MARGIN_FIELDS; ++f)
      if (s_col_min[f] < -P.tol[f]) mask |= 1u << f;
    violated[b] = mask;
    if (mask != 0) atomicAdd(n_violating, 1);
  }
}

void launch_margin_lanes(const double* raw_left, int nl, const double* raw_right, int nr, double shrink, double* prepared,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_margin_lanes, dim3(1), dim3(512), 0, st, raw_left, nl, raw_right, nr, shrink, prepared);
}

void launch_margins(const MarginParams& P, const MarginGroup& G, const double* rows, const double* corridor, const int* count,
                    double* margins, int* which, double* min_margin, int* min_knot, uint32_t* violated, int* n_violating,
                    hipStream_t st) {
  if (G.n <= 0) return;
  const size_t lds = (size_t)(G.nl + G.nr) * kLaneFields * sizeof(double);   // <= 2 x 256 x 88 B = 45 056 B
  hipLaunchKernelGGL(k_margins, dim3(G.n), dim3(kMgLanes), lds, st, P, G, rows, corridor, count, margins, which, min_margin,
                     min_knot, violated, n_violating);
}

}  // namespace cilqr
