// The obstacle points of every knot for a batch of scenes (C-ABI: cilqr_scene_points_batch; inside
// cilqr_plan_scenes_batch the link between the DP planner and the corridor producer):
// Environment::QueryStaticObstaclesPoints + QueryDynamicObstaclesPoints (algorithm/utils/environment.cpp:133-182) as
// cilqr_amd/scene_io.py::environment_points restates them, Polygon2d::sample_points (algorithm/math/polygon2d.cpp:259-271)
// for is_multiple_sample.
//
// The kernel computes next to nothing and writes a lot -- [B][K][max_points][2] doubles, 2.35 GB for 65536 scenes of
// 51 knots and 44 points -- so the mapping is chosen for its stores.  ONE WORKGROUP PER SCENE:
//   * the static points are the same at every knot: they are produced once (corners, or the six samples per edge) and
//     kept in LDS as the packed front of a row; the body-frame polygons of the dynamic obstacles are staged beside them;
//   * the knots are taken eight at a time: 8 knots x 32 obstacle slots = one (knot, obstacle) pair per lane, which does
//     the one search (scene_core.hpp's, with the 1e-10 of the Query...Points rule), the one cos / sin and,
//     with is_multiple_sample, the one orientation test of the pair, and leaves pose and point count in LDS;
//   * eight lanes turn the counts of their knot into offsets (a 32-entry running sum) and write point_count;
//   * then the lanes stride over the live points of the eight rows together: lane i builds point i from LDS and stores
//     its 16 bytes, so a wavefront's store covers 1 KiB of consecutive addresses inside a row and steps over the unused
//     tail of a row only where one row ends and the next begins.  Nothing behind point_count is written.
// One thread per (scene, knot) walking its row would store 16 bytes per lane at a stride of a whole row.
// Every index is bounded by the max_* of the call; a scene whose counts leave them gets point_count 0 at every knot and
// scene_ok 0 (DEVICE arrays; HOST arrays are refused before the launch).
//
// The arithmetic is environment_points' in its order, with the device library's cos / sin (what k_dp_place calls and
// cilqr_device_math fn 7 / 8 exposes); counts, staging, sample choice, placement and area sign are scene_core.hpp's.
//
// Behind it, three small kernels of the batched TrajectoryPlanner::Plan (cilqr_plan_scenes_batch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cilqr.h"
#include "scene_core.hpp"
#include "scene_points.hpp"

namespace cilqr {

namespace {

constexpr int kSpBlock = 256;
constexpr int kSpTile = 8;                          // knots per pass
constexpr int kSpMaxV = CILQR_DP_MAX_VERTICES;
constexpr int kSpMaxS = CILQR_DP_MAX_STATIC;
constexpr int kSpMaxD = CILQR_DP_MAX_DYNAMIC;
constexpr int kSpSamples = 6;                       // ratio = 0, 0.2, ... while ratio < 1 + 1e-10
static_assert(kSpTile * kSpMaxD == kSpBlock, "one (knot, obstacle) pair per lane");

// point q of the polygon's contribution: corner q, or sample q % 6 of edge q / 6 of the counter-clockwise polygon
template <class Vertex>
__device__ __forceinline__ void sp_point(Vertex vertex, int m, bool reversed, int per_vertex, int q, const double* ratio,
                                         double* ox, double* oy) {
  if (per_vertex == 1) {
    vertex(q, ox, oy);
    return;
  }
  const int e = q / kSpSamples, j = q - e * kSpSamples;
  const int e1 = e + 1 == m ? 0 : e + 1;
  double px, py, qx, qy;
  vertex(reversed ? m - 1 - e : e, &px, &py);
  vertex(reversed ? m - 1 - e1 : e1, &qx, &qy);
  const double r = ratio[j];
  *ox = px * (1 - r) + qx * r;
  *oy = py * (1 - r) + qy * r;
}

template <bool kWide>
__device__ __forceinline__ void sp_store(double* at, double x, double y) {
  if (kWide) {
    *reinterpret_cast<double2*>(at) = make_double2(x, y);
  } else {
    at[0] = x;
    at[1] = y;
  }
}

}  // namespace

// kWide: `points` is 16-byte aligned, a point is one store
template <bool kWide>
__global__ __launch_bounds__(kSpBlock) void k_scene_points(ScenePointsParams P, int first, const double* __restrict__ times,
                                                           const double* __restrict__ static_points,
                                                           const int* __restrict__ static_counts,
                                                           const double* __restrict__ dyn_poly,
                                                           const int* __restrict__ dyn_poly_counts,
                                                           const double* __restrict__ dyn_traj,
                                                           const int* __restrict__ dyn_traj_counts,
                                                           double* __restrict__ points, int* __restrict__ point_count,
                                                           int* __restrict__ scene_ok) {
  const int tid = threadIdx.x;
  const int local = blockIdx.x, b = first + local;
  const int K = P.n_knots, S = P.max_static, D = P.max_dynamic, V = P.max_vertices, per = P.per_vertex;

  __shared__ double s_static[kSpMaxS * kSpMaxV * kSpSamples * 2];   // the static points, packed: the front of every row
  __shared__ double s_body[kSpMaxD * kSpMaxV * 2];                  // body-frame polygons
  __shared__ double s_pose[kSpTile * kSpMaxD * 4];                  // x, y, cos, sin of a pair's trajectory sample
  __shared__ int s_count[kSpTile * kSpMaxD];                        // points a pair contributes (0: not there)
  __shared__ int s_offset[kSpTile][kSpMaxD + 1];                    // where they start in the knot's row
  __shared__ int s_row[kSpTile];                                    // live points of the knot
  __shared__ unsigned char s_reversed[kSpTile * kSpMaxD], s_static_reversed[kSpMaxS];
  __shared__ int s_static_n[kSpMaxS], s_static_offset[kSpMaxS + 1];
  __shared__ int s_m[kSpMaxD], s_T[kSpMaxD];
  __shared__ double s_ratio[kSpSamples];
  __shared__ int s_ok;

  if (tid == 0) {
    s_ok = scene_counts_valid(b, S, D, V, P.max_samples, static_counts, dyn_poly_counts, dyn_traj_counts) ? 1 : 0;
    double ratio = 0.0;   // polygon2d.cpp:264-268: accumulated, not i / 5
    for (int j = 0; j < kSpSamples; ++j) {
      s_ratio[j] = ratio;
      ratio += 1.0 / 5.0;
    }
    if (scene_ok) scene_ok[local] = s_ok;
  }
  __syncthreads();
  if (s_ok == 0) {   // (uniform)
    for (int k = tid; k < K; k += kSpBlock) point_count[(size_t)local * K + k] = 0;
    return;
  }

  // ---- the scene: static points once, body polygons
  const double* st_pts = static_points + (size_t)b * S * V * 2;
  if (tid < S) {
    const int n = static_counts[(size_t)b * S + tid];
    s_static_reversed[tid] = (per != 1 && n > 0 && scene_area_negative(ScenePolygon{st_pts + (size_t)tid * V * 2}, n)) ? 1 : 0;
    s_static_n[tid] = n;
  }
  __syncthreads();
  if (tid == 0) {
    int off = 0;
    for (int o = 0; o < S; ++o) {
      s_static_offset[o] = off;
      off += s_static_n[o] * per;
    }
    s_static_offset[S] = off;
  }
  __syncthreads();
  const int n_static = s_static_offset[S];
  for (int p = tid; p < n_static; p += kSpBlock) {
    int o = 0;
    while (o + 1 < S && p >= s_static_offset[o + 1]) ++o;
    const int n = s_static_n[o];
    auto vertex = [&](int i, double* x, double* y) {
      *x = st_pts[((size_t)o * V + i) * 2];
      *y = st_pts[((size_t)o * V + i) * 2 + 1];
    };
    sp_point(vertex, n, s_static_reversed[o] != 0, per, p - s_static_offset[o], s_ratio, &s_static[2 * p], &s_static[2 * p + 1]);
  }
  __syncthreads();
  scene_stage_dynamic(b, D, V, kSpBlock, dyn_poly, dyn_poly_counts, dyn_traj_counts, s_m, s_T, s_body);
  __syncthreads();

  // ---- eight knots at a time
  const int kk_own = D > 0 ? tid / D : kSpTile, d_own = D > 0 ? tid - kk_own * D : 0;
  for (int k0 = 0; k0 < K; k0 += kSpTile) {
    if (kk_own < kSpTile && k0 + kk_own < K) {   // one (knot, obstacle) pair
      const int m = s_m[d_own];
      int count = 0;
      bool reversed = false;
      if (m >= 1) {
        const double* traj = dyn_traj + ((size_t)b * D + d_own) * P.max_samples * 4;
        const int at = scene_sample<true>(traj, s_T[d_own], times[k0 + kk_own]);
        if (at >= 0) {
          const double* tp = traj + (size_t)at * 4;
          const double x = tp[1], y = tp[2], c = cos(tp[3]), s = sin(tp[3]);
          double* pose = s_pose + (size_t)(kk_own * kSpMaxD + d_own) * 4;
          pose[0] = x;
          pose[1] = y;
          pose[2] = c;
          pose[3] = s;
          count = m * per;
          if (per != 1) {
            const double* body = s_body + d_own * V * 2;
            auto vertex = [&](int i, double* ox, double* oy) { scene_place_vertex(body, i, x, y, c, s, ox, oy); };
            reversed = scene_area_negative(vertex, m);
          }
        }
      }
      s_count[kk_own * kSpMaxD + d_own] = count;
      s_reversed[kk_own * kSpMaxD + d_own] = reversed ? 1 : 0;
    }
    __syncthreads();
    if (tid < kSpTile) {
      int off = 0;
      if (k0 + tid < K) {
        off = n_static;
        for (int d = 0; d < D; ++d) {
          s_offset[tid][d] = off;
          off += s_count[tid * kSpMaxD + d];
        }
        s_offset[tid][D] = off;
        point_count[(size_t)local * K + k0 + tid] = off;
      }
      s_row[tid] = off;
    }
    __syncthreads();
    int row_start[kSpTile + 1];
    row_start[0] = 0;
#pragma unroll
    for (int kk = 0; kk < kSpTile; ++kk) row_start[kk + 1] = row_start[kk] + s_row[kk];
    for (int i = tid; i < row_start[kSpTile]; i += kSpBlock) {
      int kk = 0, base = 0;
#pragma unroll
      for (int j = 1; j < kSpTile; ++j)
        if (i >= row_start[j]) {
          kk = j;
          base = row_start[j];
        }
      const int p = i - base;
      double x, y;
      if (p < n_static) {
        x = s_static[2 * p];
        y = s_static[2 * p + 1];
      } else {
        int d = 0;
        while (d + 1 < D && p >= s_offset[kk][d + 1]) ++d;
        const double* pose = s_pose + (size_t)(kk * kSpMaxD + d) * 4;
        const double ox = pose[0], oy = pose[1], c = pose[2], s = pose[3];
        const double* body = s_body + d * V * 2;
        auto vertex = [&](int v, double* vx, double* vy) { scene_place_vertex(body, v, ox, oy, c, s, vx, vy); };
        sp_point(vertex, s_m[d], s_reversed[kk * kSpMaxD + d] != 0, per, p - s_offset[kk][d], s_ratio, &x, &y);
      }
      if (p < P.max_points)
        sp_store<kWide>(points + (((size_t)local * K + k0 + kk) * P.max_points + p) * 2, x, y);
    }
    __syncthreads();
  }
}

void launch_scene_points(const ScenePointsParams& P, const cilqr_scene_batch& dv, int first, int n_scenes,
                         const double* times, double* points, int* point_count, int* scene_ok, hipStream_t st) {
  if (n_scenes <= 0) return;
  const auto kernel = (reinterpret_cast<uintptr_t>(points) & 15) == 0 ? k_scene_points<true> : k_scene_points<false>;
  hipLaunchKernelGGL(kernel, dim3(n_scenes), dim3(kSpBlock), 0, st, P, first, times, dv.static_points, dv.static_counts,
                     dv.dynamic_polygon_points, dv.dynamic_polygon_counts, dv.dynamic_trajectories,
                     dv.dynamic_trajectory_counts, points, point_count, scene_ok);
}

// ------------------------------------------------------------------------------------------
// the batched TrajectoryPlanner::Plan: what lies between its stages
// ------------------------------------------------------------------------------------------
__global__ void k_plan_start3(int B, const double* __restrict__ start4, double* __restrict__ start3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 3) return;
  const int b = i / 3, e = i - b * 3;
  start3[i] = start4[(size_t)b * 4 + e];
}

// one lane per scene: trajectory_planner.cpp:32-35 ("DP failed") and :49-57 ("Corridor failed")
__global__ void k_plan_outcome(int B, int K, const int* __restrict__ found, int* __restrict__ corridor_count,
                               int* __restrict__ outcome, int* __restrict__ counts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int what = 0;
  if (found[b] == 0) {
    what = CILQR_PLAN_DP_FAILED;
    corridor_count[(size_t)b * K] = -5;
  } else {
    for (int k = 0; k < K; ++k) {
      const int n = corridor_count[(size_t)b * K + k];
      if (n <= -2 && n >= -4) what = CILQR_PLAN_CORRIDOR_FAILED;
    }
  }
  if (outcome) outcome[b] = what;
  if (what != 0) atomicAdd(counts + (what - 1), 1);
}

// One wavefront per scene: the chord lengths of its K - 1 steps in parallel, their running sum by one lane (the
// reference adds them in order), then the rows with the lanes striding over the 11 K doubles of the scene.
constexpr int kPlanBlock = 64;
__global__ __launch_bounds__(kPlanBlock) void k_plan_rows(int K, const double* __restrict__ traj, double* __restrict__ plan) {
  __shared__ double s_len[CILQR_DP_MAX_KNOTS];
  const int tid = threadIdx.x;
  const double* in = traj + (size_t)blockIdx.x * K * CILQR_TRAJ_FIELDS;
  double* out = plan + (size_t)blockIdx.x * K * CILQR_PLAN_FIELDS;
  constexpr RowColumns kTraj = row_columns(CILQR_ROWS_TRAJ), kPlan = row_columns(CILQR_ROWS_PLAN);
  for (int k = tid; k < K; k += kPlanBlock)
    s_len[k] = k > 0 ? hypot_ref(in[k * CILQR_TRAJ_FIELDS + kTraj.x] - in[(k - 1) * CILQR_TRAJ_FIELDS + kTraj.x],
                                 in[k * CILQR_TRAJ_FIELDS + kTraj.y] - in[(k - 1) * CILQR_TRAJ_FIELDS + kTraj.y])
                     : 0.0;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
      s += s_len[k];
      s_len[k] = s;
    }
  }
  __syncthreads();
  // every column of a plan row from the CILQR_ROWS_TRAJ column of the same name; the station is the running chord length
  constexpr ColumnMap from = column_map(kPlan, kTraj);
  for (int i = tid; i < K * CILQR_PLAN_FIELDS; i += kPlanBlock) {
    const int k = i / CILQR_PLAN_FIELDS, c = i - k * CILQR_PLAN_FIELDS;
    out[i] = c == kPlan.station ? s_len[k] : in[k * CILQR_TRAJ_FIELDS + from.col[c]];
  }
}

void launch_plan_start3(int B, const double* start4, double* start3, hipStream_t st) {
  hipLaunchKernelGGL(k_plan_start3, dim3((B * 3 + 255) / 256), dim3(256), 0, st, B, start4, start3);
}

void launch_plan_outcome(int B, int K, const int* found, int* corridor_count, int* outcome, int* counts, hipStream_t st) {
  hipLaunchKernelGGL(k_plan_outcome, dim3((B + 255) / 256), dim3(256), 0, st, B, K, found, corridor_count, outcome, counts);
}

void launch_plan_rows(int B, int K, const double* traj, double* plan, hipStream_t st) {
  hipLaunchKernelGGL(k_plan_rows, dim3(B), dim3(kPlanBlock), 0, st, K, traj, plan);
}

}  // namespace cilqr
