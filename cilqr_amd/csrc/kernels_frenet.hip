// cilqr_frenet_rows_batch / cilqr_cartesian_points_batch (include/cilqr.h, "frenet"): DiscretizedTrajectory::GetProjection
// for every row of a batch of trajectories, and GetCartesian for a list of (station, lateral) pairs.  The host statement is
// include/cilqr/trajectory_queries.hpp; the interpolation is dp_core.hpp's (dp_interpolate, the exact normalize_angle, the
// libm-identical hypot_ref), which the DP kernel already holds to that arithmetic (-ffp-contract=off, IEEE division).
//
// k_frenet.  The rule's nearest point is the FIRST minimum of a full scan: B K queries x n_center points, about eight fp64
// instructions each (two differences, two products, a sum, a compare, the selects) -- the kernel is bound by the fp64
// pipe, not by memory.  The work items are the queries, flattened in the order of the output.  A workgroup of 256 lanes
// takes 256 R consecutive queries; lane t owns queries t, t + 256, ... of them, px / py / the running (distance, index) in
// registers.  The centre line's packed (x, y) pairs pass through LDS in tiles of kFrTile points; in the scan every lane
// reads the SAME 16 bytes per step (one ds_read_b128, a broadcast: no bank conflict), which then serve 64 R distance
// evaluations per wavefront.  Tiles and points are walked in ascending index with a strict `<`, so the running minimum IS
// the reference's first minimum and no tie-break is needed.  R = kFrWide for calls that fill the chip that way, 1 below.
// Rows enter and leave through one LDS tile: the 256 F input doubles of a run of queries are loaded flat (consecutive lanes,
// consecutive doubles) and each lane picks its x, y out of LDS; the 8-double results are put down at a row stride of 9
// doubles (odd: a ds_write_b64 group spreads over all banks) and leave flat.
// The epilogue runs once per query: the rows at-1, at, at+1 of the [n][7] table (L2), the interpolation, the offset.
//
// k_cartesian.  One lane per pair; it bisects the station column through L2 (1952 points: 11 dependent loads of a 15.6 KB
// column) and writes its [3] row.  It is small and bound by those loads.
#include <cfloat>

#include "dp_core.hpp"
#include "frenet.hpp"

namespace cilqr {

constexpr int kFrOutStride = CILQR_FRENET_FIELDS + 1;
constexpr int kFrTileDoubles = kFrLanes * CILQR_PLAN_FIELDS;   // the widest input rows of a run
static_assert(kFrLanes * kFrOutStride <= kFrTileDoubles, "the results of a run fit where its input rows were");

// hypot as the C library returns it: an infinite component wins over a NaN; everything else is hypot_ref's
CILQR_DEV double fr_hypot(double x, double y) {
  if (isinf(x) || isinf(y)) return HUGE_VAL;
  return hypot_ref(x, y);
}

// F: doubles per input row (2 points, 9 coarse, 10 traj, 11 plan); R: queries per lane
template <int F, int R>
__global__ __launch_bounds__(kFrLanes) void k_frenet(FrenetParams P, size_t n_groups, const double* __restrict__ rows,
                                                     double* __restrict__ frenet) {
  constexpr RowColumns C = columns_of_fields(F);
  static_assert(F <= CILQR_PLAN_FIELDS, "a run's rows must fit the tile");
  __shared__ double2 s_xy[kFrTile];
  __shared__ double s_tile[kFrTileDoubles];
  const int tid = threadIdx.x;
  const int N = P.n_center;
  DpParams road;   // of the DP planner's parameters the centre line alone is read
  road.center = P.center;
  road.n_center = N;

  for (size_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const size_t q0 = g * (size_t)(kFrLanes * R);   // < n_queries
    double px[R], py[R], nearest[R];
    int at[R];
    // ---- the queries of this group: R runs of up to 256
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t qr = q0 + (size_t)r * kFrLanes;
      const int n = qr < P.n_queries ? (int)min((size_t)kFrLanes, P.n_queries - qr) : 0;
      if (n > 0) {
        const double* __restrict__ src = rows + qr * F;
        for (int i = tid; i < n * F; i += kFrLanes) s_tile[i] = src[i];
      }
      __syncthreads();
      px[r] = tid < n ? s_tile[tid * F + C.x] : 0.0;
      py[r] = tid < n ? s_tile[tid * F + C.y] : 0.0;
      nearest[r] = DBL_MAX;
      at[r] = 0;
      __syncthreads();
    }
    // ---- QueryNearestPoint (discretized_trajectory.cpp:138-157)
    for (int t0 = 0; t0 < N; t0 += kFrTile) {
      const int cnt = min(kFrTile, N - t0);
      for (int i = tid; i < cnt; i += kFrLanes) s_xy[i] = reinterpret_cast<const double2*>(P.xy)[t0 + i];
      __syncthreads();
#pragma unroll 4
      for (int j = 0; j < cnt; ++j) {
        const double2 c = s_xy[j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double dx = c.x - px[r], dy = c.y - py[r];
          const double d = dx * dx + dy * dy;
          if (d < nearest[r]) {
            at[r] = t0 + j;
            nearest[r] = d;
          }
        }
      }
      __syncthreads();
    }
    // ---- GetProjection (cpp:159-190), run by run
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t qr = q0 + (size_t)r * kFrLanes;
      const int n = qr < P.n_queries ? (int)min((size_t)kFrLanes, P.n_queries - qr) : 0;
      if (tid < n) {
        const int a = at[r];
        DpRef proj = dp_center_point(road, a);
        const int i0 = a > 0 ? a - 1 : 0;
        const int i1 = min(N - 1, a + 1);
        if (i0 < i1) {
          const DpRef p0 = dp_center_point(road, i0), p1 = dp_center_point(road, i1);
          const double v0x = px[r] - p0.x, v0y = py[r] - p0.y;
          const double v1x = p1.x - p0.x, v1y = p1.y - p0.y;
          const double v1_norm = sqrt(v1x * v1x + v1y * v1y);
          const double dot = v0x * v1x + v0y * v1y;
          const double delta_s = dot / v1_norm;
          proj = dp_interpolate(p0, p1, p0.s + delta_s);
        }
        const double nr_x = px[r] - proj.x, nr_y = py[r] - proj.y;
        double sn, cs;
        lean_sincos(proj.theta, &sn, &cs);   // the sign of the side alone
        double* o = s_tile + tid * kFrOutStride;
        o[0] = proj.s;
        o[1] = copysign(fr_hypot(nr_x, nr_y), nr_y * cs - nr_x * sn);
        o[2] = proj.x;
        o[3] = proj.y;
        o[4] = proj.theta;
        o[5] = proj.kappa;
        o[6] = proj.left_bound;
        o[7] = proj.right_bound;
      }
      __syncthreads();
      if (n > 0) {   // the run leaves: n * 8 consecutive doubles of `frenet`
        double* __restrict__ dst = frenet + qr * CILQR_FRENET_FIELDS;
        for (int i = tid; i < n * CILQR_FRENET_FIELDS; i += kFrLanes)
          dst[i] = s_tile[(i >> 3) * kFrOutStride + (i & 7)];
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kFrLanes) void k_cartesian(const double* __restrict__ center, int n_center, int n,
                                                        const double* __restrict__ sl, double* __restrict__ xyt) {
  const size_t i = (size_t)blockIdx.x * kFrLanes + threadIdx.x;
  if (i >= (size_t)n) return;
  DpParams road;
  road.center = center;
  road.n_center = n_center;
  const double station = sl[2 * i], lateral = sl[2 * i + 1];
  const DpRef ref = dp_evaluate_station(road, station);   // cpp:112-123
  xyt[3 * i] = ref.x - lateral * sin(ref.theta);          // the device library's, as the points kernel's
  xyt[3 * i + 1] = ref.y + lateral * cos(ref.theta);
  xyt[3 * i + 2] = ref.theta;
}

template <int F>
static void launch_frenet_rows(const FrenetParams& P, const double* rows, double* frenet, hipStream_t st) {
  const bool wide = P.n_queries >= kFrWideFrom;
  const size_t per_group = (size_t)kFrLanes * (wide ? kFrWide : 1);
  const size_t n_groups = (P.n_queries + per_group - 1) / per_group;
  const dim3 grid((unsigned)min(n_groups, (size_t)0x7fffffff));   // the kernel strides over what a grid cannot hold
  if (wide) hipLaunchKernelGGL((k_frenet<F, kFrWide>), grid, dim3(kFrLanes), 0, st, P, n_groups, rows, frenet);
  else hipLaunchKernelGGL((k_frenet<F, 1>), grid, dim3(kFrLanes), 0, st, P, n_groups, rows, frenet);
}

void launch_frenet(const FrenetParams& P, const double* rows, double* frenet, hipStream_t st) {
  switch (P.fields) {
    case 2: launch_frenet_rows<2>(P, rows, frenet, st); break;
    case 9: launch_frenet_rows<9>(P, rows, frenet, st); break;
    case 10: launch_frenet_rows<10>(P, rows, frenet, st); break;
    case 11: launch_frenet_rows<11>(P, rows, frenet, st); break;
  }
}

void launch_cartesian(const double* center, int n_center, int n, const double* sl, double* xyt, hipStream_t st) {
  const dim3 grid((unsigned)(((size_t)n + kFrLanes - 1) / kFrLanes));
  hipLaunchKernelGGL(k_cartesian, grid, dim3(kFrLanes), 0, st, center, n_center, n, sl, xyt);
}

}  // namespace cilqr
