// cilqr_track_rows_batch (include/cilqr.h, "track"): the closed-loop Tracker on caller's rows, one lane per problem.  The
// steps are tracker_core.hpp's, the ones k_init_guess_tracker runs; the host statement is include/cilqr/tracker.hpp, which
// this follows operation by operation except for sin / cos / tan (the device's lean routines instead of the C library's)
// and the division by the wheel base (a product with its reciprocal).
//
// The work per problem is one chain of about 10 (K - 1) dependent simulation steps, each with a DARE loop and a scan of all
// K followed points for the nearest.  Read where the caller's rows lie -- problem-major, 72 to 88 bytes per row -- the 64
// lanes of a wave would touch 64 different cache lines per load of that scan and use 16 bytes of each.  So the call runs
// in two kernels:
//   k_track_gather  transposes the columns the rule reads (time, station, x, y, theta, v; the start state) into the
//                   batch-fastest follow table of track.hpp.  A workgroup of 256 lanes takes 64 problems: per tile of 8
//                   knots it stages their rows into LDS with flat consecutive loads (a problem's tile is one contiguous
//                   piece of `rows`), then lane p of the first wave walks problem p's rows in LDS and stores the table's
//                   pairs -- 64 lanes, one contiguous kilobyte per store.  The chord stations of CILQR_ROWS_TRAJ are
//                   accumulated there, knot by knot in the lane that owns the problem.  The LDS row stride is odd in
//                   doubles, so the 64 lanes' reads spread over the banks.
//   k_track_rows    runs the simulation on the table with the access pattern of k_init_guess_tracker and writes every kept
//                   row straight into `driven` (80 bytes per lane, n_drive times per problem: nothing beside the scans).
// The loop of the simulation is bounded by P.max_steps whatever the time column holds.
#include "track.hpp"
#include "tracker_core.hpp"

namespace cilqr {

constexpr int kTgLanes = 256;
constexpr int kTgProblems = 64;   // per workgroup: the lanes of the wave that writes the table
constexpr int kTgKnots = 8;       // per tile

// F: doubles per row (10 traj, 11 plan, 9 coarse)
template <int F>
__global__ __launch_bounds__(kTgLanes) void k_track_gather(TrackParams P, const double* __restrict__ rows,
                                                           const double* __restrict__ start6, FollowTable tab) {
  constexpr int S = kTgKnots * F + 1;            // odd for every F here (81, 89, 73)
  constexpr RowColumns C = columns_of_fields(F);
  constexpr bool kChord = C.station < 0;         // CILQR_ROWS_TRAJ has no station column
  __shared__ double tile[kTgProblems * S];
  const int tid = threadIdx.x;
  const int K = P.n_knots;
  const int b0 = (int)blockIdx.x * kTgProblems;   // < batch: the grid is ceil(batch / 64) wide
  const int np = min(kTgProblems, P.batch - b0);
  double px = 0.0, py = 0.0, acc = 0.0;           // lane p < np: the chord so far of problem b0 + p
  for (int k0 = 0; k0 < K; k0 += kTgKnots) {
    const int kt = min(kTgKnots, K - k0), n = kt * F;
    for (int e = tid; e < np * n; e += kTgLanes) {
      const int q = e / n, j = e - q * n;
      tile[q * S + j] = rows[((size_t)(b0 + q) * K + k0) * F + j];
    }
    __syncthreads();
    if (tid < np) {
      const size_t col = (size_t)b0 + tid;
      for (int kk = 0; kk < kt; ++kk) {
        const double* r = tile + tid * S + kk * F;
        const int k = k0 + kk;
        const double x = r[C.x], y = r[C.y];
        double station;
        if constexpr (kChord) {
          if (k > 0) acc = acc + hypot_ref(x - px, y - py);
          station = acc;
          px = x;
          py = y;
        } else {
          station = r[C.station];
        }
        const size_t at = (size_t)k * tab.stride + col;
        tab.xy[at] = make_double2(x, y);
        tab.thv[at] = make_double2(r[C.theta], r[C.v]);
        tab.ts[at] = make_double2(r[C.time], station);
        if (k == 0) {
          double s6[6] = {x, y, r[C.theta], r[C.v], r[C.a], r[C.delta]};
          if (start6 != nullptr) {
#pragma unroll
            for (int c = 0; c < 6; ++c) s6[c] = start6[col * 6 + c];
          }
          tab.start[col] = make_double2(s6[0], s6[1]);
          tab.start[(size_t)tab.stride + col] = make_double2(s6[2], s6[3]);
          tab.start[(size_t)2 * tab.stride + col] = make_double2(s6[4], s6[5]);
        }
      }
    }
    __syncthreads();
  }
}

void launch_track_gather(const TrackParams& P, const double* rows, const double* start6, const FollowTable& tab, hipStream_t st) {
  const dim3 grid(((unsigned)P.batch + kTgProblems - 1u) / kTgProblems);
  switch (P.fields) {
    case 9: hipLaunchKernelGGL(k_track_gather<9>, grid, dim3(kTgLanes), 0, st, P, rows, start6, tab); break;
    case 10: hipLaunchKernelGGL(k_track_gather<10>, grid, dim3(kTgLanes), 0, st, P, rows, start6, tab); break;
    case 11: hipLaunchKernelGGL(k_track_gather<11>, grid, dim3(kTgLanes), 0, st, P, rows, start6, tab); break;
  }
}

namespace {

// one lane's view of the follow table
struct TableFollow {
  const FollowTable& t;
  size_t col;
  int K;
  CILQR_DEV void xy(int i, double& x, double& y) const {
    const double2 a = t.xy[(size_t)i * t.stride + col];
    x = a.x;
    y = a.y;
  }
  CILQR_DEV tracker_core::FollowPt pt(int i) const {
    const size_t at = (size_t)i * t.stride + col;
    const double2 a = t.xy[at], b = t.thv[at], c = t.ts[at];
    tracker_core::FollowPt f;
    f.s = c.y; f.x = a.x; f.y = a.y; f.theta = b.x; f.v = b.y;
    return f;
  }
  CILQR_DEV double time(int i) const { return t.ts[(size_t)i * t.stride + col].x; }
  // the bracket of include/cilqr.h ("resample") on the time column, before its `i == 0 -> 1`
  CILQR_DEV int locate(double q) const {
    return min(bracket(K, q, [&](int i) { return time(i); }), K - 1);   // (not reached beyond K - 1: q < time[K-1] here)
  }
};

// the kept rows of one problem, in CILQR_TRAJ_FIELDS layout
struct RowSink {
  double* out;   // [n_drive][10]
  double wheel_base;
  CILQR_DEV void row(int i, const double* x, double time) const {
    double* o = out + (size_t)i * CILQR_TRAJ_FIELDS;
    o[0] = time;
    o[1] = x[0]; o[2] = x[1]; o[3] = x[2]; o[4] = x[3]; o[5] = x[4]; o[6] = x[5];
    o[7] = tan(x[5]) / wheel_base;   // as write_traj_point (dev_model.hpp)
    o[8] = 0.0; o[9] = 0.0;          // until the next row is kept; the last row's stay, as the export's last knot
  }
  CILQR_DEV void keep(int i, const double* x, const double* u, double time) const {
    double* prev = out + (size_t)(i - 1) * CILQR_TRAJ_FIELDS;
    prev[8] = u[0];
    prev[9] = u[1];
    row(i, x, time);
  }
};

}  // namespace

__global__ __launch_bounds__(64) void k_track_rows(TrackParams P, Params p, TrackerParams tp, FollowTable tab,
                                                   double* __restrict__ driven, int* __restrict__ ok,
                                                   int* __restrict__ n_failed) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  const TableFollow follow{tab, (size_t)b, P.n_knots};
  double x6[6];
  {
    const double2 a = tab.start[b], c = tab.start[(size_t)tab.stride + b], d = tab.start[(size_t)2 * tab.stride + b];
    x6[0] = a.x; x6[1] = a.y; x6[2] = c.x; x6[3] = c.y; x6[4] = d.x; x6[5] = d.y;
  }
  RowSink sink{driven + (size_t)b * P.n_drive * CILQR_TRAJ_FIELDS, p.wheel_base};
  sink.row(0, x6, follow.time(0));
  const int kept = tracker_core::tracker_drive(follow, p, tp, x6, P.n_drive, P.max_steps, sink);
  const bool good = kept == P.n_drive;
  if (!good) {   // "tacker failed" (tracker.cc:205-208): this problem's rows are zero
    for (size_t e = 0; e < (size_t)P.n_drive * CILQR_TRAJ_FIELDS; ++e) sink.out[e] = 0.0;
    atomicAdd(n_failed, 1);
  }
  ok[b] = good ? 1 : 0;
}

void launch_track_rows(const TrackParams& P, const Params& vehicle, const TrackerParams& tp, const FollowTable& tab,
                       double* driven, int* ok, int* n_failed, hipStream_t st) {
  hipLaunchKernelGGL(k_track_rows, dim3(((unsigned)P.batch + 63u) / 64u), dim3(64), 0, st, P, vehicle, tp, tab, driven, ok,
                     n_failed);
}

}  // namespace cilqr
