// Which knots of a batch of trajectories touch their scenes (C-ABI: cilqr_check_collisions_batch):
// Environment::CheckOptimizationCollision (algorithm/utils/environment.cpp:92-111) with a collision buffer, as
// DpEnvironment::CollisionMask (include/cilqr/dp_planner.hpp) states it -- every one of the six (disc, kind of obstacle)
// tests, none short-circuited.  The geometry is dp_core.hpp's, the functions the DP kernels decide with; the steps on the
// scene's arrays (counts, staging, sample choice, placement, disc centres, barrier window) are scene_core.hpp's.
//
// ONE WORKGROUP PER SCENE, and everything a scene's knots share stays in LDS:
//   * the static polygons with their boxes and the body-frame polygons of the dynamic obstacles are staged once;
//   * one lane per knot reads the pose from the row (the only columns touched: time, x, y, theta) and leaves the time
//     and the two disc centres in LDS;
//   * the lanes stride over the (knot, dynamic slot) pairs: a pair's lane picks the sample, places and boxes the polygon
//     and tests it against both discs of the knot -- the placed polygon lives in the lane's own record in LDS, so
//     nothing is indexed in registers and nothing goes to scratch;
//   * the same lanes stride over the (knot, static slot) pairs;
//   * one lane per disc finds its barrier window, then every wavefront takes discs in turn and its 64 lanes stride over
//     the window's points;
//   * bits are OR-ed into one LDS word per knot; after the last pass the row is written with consecutive addresses and
//     first_hit / n_hit are reduced with LDS atomics.
// Every index is bounded by the max_* of the call and by n_knots <= CILQR_DP_MAX_KNOTS; a scene whose counts leave them gets
// first_hit -2, n_hit 0 and a zero mask row (DEVICE arrays; HOST arrays are refused before the launch).
// Built with -ffp-contract=off like every other file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collision.hpp"
#include "dp_core.hpp"

namespace cilqr {

namespace {

constexpr int kCcBlock = 256;
constexpr int kCcWave = 64;
constexpr int kCcMaxK = CILQR_DP_MAX_KNOTS;
constexpr int kCcMaxS = CILQR_DP_MAX_STATIC;
constexpr int kCcMaxD = CILQR_DP_MAX_DYNAMIC;
constexpr int kCcLaneRec = kDpRec + 1;   // a lane's placed polygon; the odd stride spreads the lanes over the LDS banks
static_assert(kDpMaxV == CILQR_DP_MAX_VERTICES, "a polygon record holds the declared number of vertices");

constexpr unsigned kRearStatic = 1u, kRearBarrier = 2u, kRearDynamic = 4u;   // CILQR_HIT_*; the front disc: << 3

}  // namespace

__global__ __launch_bounds__(kCcBlock) void k_check_collisions(CollisionParams P, const double* __restrict__ rows,
                                                               const double* __restrict__ static_points,
                                                               const int* __restrict__ static_counts,
                                                               const double* __restrict__ dyn_poly,
                                                               const int* __restrict__ dyn_poly_counts,
                                                               const double* __restrict__ dyn_traj,
                                                               const int* __restrict__ dyn_traj_counts,
                                                               uint8_t* __restrict__ mask, int* __restrict__ first_hit,
                                                               int* __restrict__ n_hit, int* __restrict__ n_colliding) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int K = P.n_knots, S = P.max_static, D = P.max_dynamic, V = P.max_vertices;

  __shared__ double s_static[kCcMaxS * kDpRec];        // box, vertices
  __shared__ double s_body[kCcMaxD * kDpMaxV * 2];     // body-frame polygons
  __shared__ double s_placed[kCcBlock * kCcLaneRec];   // per lane: the polygon it placed
  __shared__ double s_disc[kCcMaxK * 4];               // rear x y, front x y
  __shared__ double s_time[kCcMaxK];
  __shared__ unsigned s_mask[kCcMaxK];
  __shared__ int s_window[2 * kCcMaxK][2];             // barrier points [first, last) of a disc; empty: first = last
  __shared__ int s_static_n[kCcMaxS], s_m[kCcMaxD], s_T[kCcMaxD];
  __shared__ int s_ok, s_first, s_count;

  if (tid == 0) {
    s_ok = scene_counts_valid(b, S, D, V, P.max_samples, static_counts, dyn_poly_counts, dyn_traj_counts) ? 1 : 0;
    s_first = K;
    s_count = 0;
  }
  __syncthreads();
  if (s_ok == 0) {   // (uniform)
    if (mask)
      for (int k = tid; k < K; k += kCcBlock) mask[(size_t)b * K + k] = 0;
    if (tid == 0) {
      first_hit[b] = -2;
      if (n_hit) n_hit[b] = 0;
    }
    return;
  }

  // ---- the scene and the knots
  if (tid < S) {
    const int n = static_counts[(size_t)b * S + tid];
    s_static_n[tid] = n;
    if (n > 0) scene_stage_static(static_points + ((size_t)b * S + tid) * V * 2, n, s_static + tid * kDpRec);
  }
  scene_stage_dynamic(b, D, V, kCcBlock, dyn_poly, dyn_poly_counts, dyn_traj_counts, s_m, s_T, s_body);
  for (int k = tid; k < K; k += kCcBlock) {
    const double* row = rows + ((size_t)b * K + k) * P.rows.fields;
    s_time[k] = row[P.rows.time];
    scene_discs_of_pose(row[P.rows.x], row[P.rows.y], row[P.rows.theta], P.r2x, P.f2x, s_disc + 4 * k);
    s_mask[k] = 0u;
  }
  __syncthreads();

  // ---- (knot, dynamic slot): environment.cpp:113-130
  double* placed = s_placed + tid * kCcLaneRec;
  for (int p = tid; p < K * D; p += kCcBlock) {
    const int k = p / D, d = p - k * D;
    const int m = s_m[d];
    if (m < 1) continue;
    const double* traj = dyn_traj + ((size_t)b * D + d) * P.max_samples * 4;
    const int T = s_T[d];
    const double t = s_time[k];
    if (!scene_present<false>(traj, T, t)) continue;
    const double* tp = traj + (size_t)scene_sample_index<false>(traj, T, t) * 4;
    scene_place(s_body + d * V * 2, m, tp[1], tp[2], cos(tp[3]), sin(tp[3]), placed + 4);
    dp_bounding_box(placed + 4, m, placed);
    unsigned bits = 0u;
    if (dp_overlap(placed, placed + 4, m, dp_square_of(P.h, s_disc[4 * k], s_disc[4 * k + 1]))) bits |= kRearDynamic;
    if (dp_overlap(placed, placed + 4, m, dp_square_of(P.h, s_disc[4 * k + 2], s_disc[4 * k + 3]))) bits |= kRearDynamic << 3;
    if (bits) atomicOr(&s_mask[k], bits);
  }

  // ---- (knot, static slot): environment.cpp:47-52
  for (int p = tid; p < K * S; p += kCcBlock) {
    const int k = p / S, o = p - k * S;
    const int n = s_static_n[o];
    if (n < 1) continue;
    const double* rec = s_static + o * kDpRec;
    unsigned bits = 0u;
    if (dp_overlap(rec, rec + 4, n, dp_square_of(P.h, s_disc[4 * k], s_disc[4 * k + 1]))) bits |= kRearStatic;
    if (dp_overlap(rec, rec + 4, n, dp_square_of(P.h, s_disc[4 * k + 2], s_disc[4 * k + 3]))) bits |= kRearStatic << 3;
    if (bits) atomicOr(&s_mask[k], bits);
  }

  // ---- the road barriers, environment.cpp:54-80: the window of every disc, then the points of the windows
  for (int p = tid; p < 2 * K; p += kCcBlock) {
    const DpSquare sq = dp_square_of(P.h, s_disc[2 * p], s_disc[2 * p + 1]);   // disc p & 1 of knot p >> 1
    int first, last;
    scene_barrier_window(P.barrier, P.n_barrier, sq.min_x, sq.max_x, &first, &last);
    s_window[p][0] = first;
    s_window[p][1] = last;
  }
  __syncthreads();
  const int wave = tid / kCcWave, lane = tid - wave * kCcWave;
  for (int p = wave; p < 2 * K; p += kCcBlock / kCcWave) {
    const int first = s_window[p][0], last = s_window[p][1];
    const DpSquare sq = dp_square_of(P.h, s_disc[2 * p], s_disc[2 * p + 1]);
    bool hit = false;
    for (int i = first + lane; i < last; i += kCcWave)
      hit = hit || dp_square_has_point(sq, P.barrier[(size_t)i * 2], P.barrier[(size_t)i * 2 + 1]);
    if (hit) atomicOr(&s_mask[p >> 1], (p & 1) ? (kRearBarrier << 3) : kRearBarrier);
  }
  __syncthreads();

  // ---- the row, the first knot that touches something, how many do
  for (int k = tid; k < K; k += kCcBlock) {
    const unsigned m = s_mask[k];
    if (mask) mask[(size_t)b * K + k] = (uint8_t)m;
    if (m != 0u) {
      atomicMin(&s_first, k);
      atomicAdd(&s_count, 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int first = s_first < K ? s_first : -1;
    first_hit[b] = first;
    if (n_hit) n_hit[b] = s_count;
    if (first >= 0) atomicAdd(n_colliding, 1);
  }
}

void launch_check_collisions(const CollisionParams& P, const cilqr_scene_batch& dv, const double* rows, uint8_t* mask,
                             int* first_hit, int* n_hit, int* n_colliding, hipStream_t st) {
  if (dv.batch <= 0) return;
  hipLaunchKernelGGL(k_check_collisions, dim3(dv.batch), dim3(kCcBlock), 0, st, P, rows, dv.static_points, dv.static_counts,
                     dv.dynamic_polygon_points, dv.dynamic_polygon_counts, dv.dynamic_trajectories,
                     dv.dynamic_trajectory_counts, mask, first_hit, n_hit, n_colliding);
}

}  // namespace cilqr
