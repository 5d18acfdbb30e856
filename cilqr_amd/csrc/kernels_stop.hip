// cilqr_stop_rows_batch and what cilqr_stop_scenes_batch puts behind its audits (include/cilqr.h, "stop").  The host
// statement is include/cilqr/trajectory_queries.hpp: stop_rows.  Its stop_step, and the bracket and the pair step of
// include/cilqr/row_math.hpp (bracket_pair, pair_step over pair_stop), are ONE function for both; the station keys
// (row_math.hpp's hypot_ref where the host statement takes std::hypot), the differenced controls and the statuses k_stop
// follows operation by operation (-ffp-contract=off, IEEE division), so the rows are its bits.
//
// k_stop moves memory: per trajectory it reads n_knots F doubles and writes 11 n_out per profile.  A workgroup of 256 lanes
// takes a run of whole trajectories -- as many as fit 32 KiB of LDS, at most 16 -- and
//   1. stages their rows (contiguous in `rows`) into LDS with flat consecutive loads, and their station keys beside them: the
//      station column, or for rows without one the running sum of the chord lengths (taken in parallel, summed by one lane
//      per trajectory in knot order); all profiles share both;
//   2. one lane per (trajectory, profile) runs the speed chain and puts s, velocity and a into an LDS image of the plan rows;
//   3. the (trajectory, profile, knot) triples are flattened over the lanes: each lane brackets its s in the keys (at most 8
//      steps in LDS), interpolates x y theta kappa delta and completes its row of the image;
//   4. jerk and delta_rate are differenced from the next row of the image; a wavefront that saw a non-finite value (one
//      ballot) marks the chains concerned as refused;
//   5. the rows leave flat: consecutive lanes store consecutive doubles of a chain's slice.
// An image of n_out rows for every profile may not fit (256 rows x 8 profiles are 176 KiB), and a small one pays: steps 2 - 5
// run per chunk of at most 12 knots, the chain lanes keeping their state in registers, with one row of look-ahead for the
// differences.  Short chunks leave LDS for more trajectories a workgroup -- more chains side by side in the wavefront that
// runs them, while the other lanes wait -- and for more workgroups a CU; 32 KiB and 12 knots against 48 KiB and the whole
// image are timed on 65536 plans of 51 knots in profiles/r20_stop.json (plan_variants; the figures: DESIGN.md, (f)-17).  A
// chain found non-finite in a later chunk has its earlier rows written over with zeros at the end.  The image's row stride
// is 11 doubles: odd, so the lanes of a ds_write_b64 group spread over all banks.
#include <algorithm>
#include <cstdlib>

#include "../../include/cilqr/trajectory_queries.hpp"
#include "dev_model.hpp"
#include "stop.hpp"

namespace cilqr {

constexpr int kStLanes = 256;
constexpr int kStMaxRun = 16;                 // trajectories per workgroup, at most
constexpr size_t kStLdsBudget = 32 * 1024;    // ... and what their rows, keys and images may take together
constexpr int kStChunk = 12;                  // knots a chunk, at the most
constexpr int kStMinImage = 4;                // image rows a chain always gets (three knots and the look-ahead)
constexpr int kStMaxChains = kStMaxRun * CILQR_STOP_MAX_PROFILES;
static_assert(kStMaxChains <= kStLanes, "one lane per chain of a run");
constexpr int kPF = CILQR_PLAN_FIELDS;

// The non-finite test of a round: ONE ballot per wavefront, and where all is finite -- nearly always -- nothing else.  Otherwise
// the wavefront's first lane marks the chains of the lanes the ballot names: lane l of the wavefront works on element
// e_wave + l, which belongs to chain (e_wave + l) / per.  (Every lane of the workgroup makes the same trips through a round, so
// whole wavefronts meet here.)
__device__ inline void mark_bad(bool bad, int e_wave, int per, int* s_bad) {
  unsigned long long m = __ballot(bad);
  if (m != 0ull && (threadIdx.x & 63) == 0)
    for (; m != 0ull; m &= m - 1) s_bad[(e_wave + __ffsll((long long)m) - 1) / per] = 1;
}

// F: doubles per row (9 coarse, 10 traj, 11 plan).  run: trajectories per workgroup; nc: knots per chunk; ni: rows of a
// chain's image (nc + 1 with look-ahead, n_out when one chunk holds all).
template <int F>
__global__ __launch_bounds__(kStLanes) void k_stop(StopParams P, int run, int nc, int ni, const double* __restrict__ rows,
                                                   const double* __restrict__ start_va, double* __restrict__ out_rows,
                                                   int* __restrict__ status, int* __restrict__ stop_knot,
                                                   double* __restrict__ travel) {
  constexpr RowColumns C = columns_of_fields(F);
  constexpr RowColumns O = row_columns(CILQR_ROWS_PLAN);
  constexpr PairColumns kFive = trajectory_queries::pair_stop(C, O);   // x y theta kappa delta, to where a plan row keeps them
  constexpr PairColumns kFiveV = pair_packed(kFive);                   // ... and to v[0 ... 4]
  extern __shared__ double s_mem[];
  __shared__ int s_refused0[kStMaxChains];   // by the start values: nothing is produced
  __shared__ int s_bad[kStMaxChains];        // a non-finite value was produced
  const int K = P.n_knots, M = P.n_profiles, N = P.n_out;
  double* s_rows = s_mem;                               // [run][K][F]
  double* s_key = s_rows + (size_t)run * K * F;         // [run][K]
  double* s_img = s_key + (size_t)run * K;              // [run][M][ni][11]
  const int tid = threadIdx.x;
  const size_t b0 = (size_t)blockIdx.x * run;           // < batch: the grid is ceil(batch / run) wide
  const int np = (int)min((size_t)run, (size_t)P.batch - b0);
  const int nch = np * M;                               // the chains of this workgroup: chain pm = p * M + m

  // ---- 1. the rows of the run and their station keys
  stage_in<kStLanes>(rows + b0 * K * F, s_rows, np * K * F);
  __syncthreads();
  for (int e = tid; e < np * K; e += kStLanes) {
    const double* r = s_rows + (size_t)e * F;
    if constexpr (C.station >= 0) {
      s_key[e] = r[C.station];
    } else {
      const int i = e % K;
      s_key[e] = i > 0 ? hypot_ref(r[C.x] - r[C.x - F], r[C.y] - r[C.y - F]) : 0.0;   // the chord behind knot i
    }
  }
  __syncthreads();
  if constexpr (C.station < 0) {
    if (tid < np) {
      double* key = s_key + tid * K;
      double s = 0.0;
      for (int i = 1; i < K; ++i) {   // in knot order, as the rule adds them
        s = s + key[i];
        key[i] = s;
      }
    }
    __syncthreads();
  }

  // ---- the chains: one lane each, its state in registers over the chunks
  trajectory_queries::StopState c{0.0, 0.0, 0.0};
  double key0 = 0.0, s_end = 0.0, a_target = 0.0, jd = 0.0;
  const double hd = 0.5 * P.delta_t;
  bool refused0 = true, overrun = false;
  int knot = -1;
  if (tid < nch) {
    const int p = tid / M, m = tid - p * M;
    const double* T = s_rows + (size_t)p * K * F;
    const double v0 = start_va ? start_va[(b0 + p) * 2] : T[C.v], a0 = start_va ? start_va[(b0 + p) * 2 + 1] : T[C.a];
    key0 = s_key[p * K];
    s_end = s_key[p * K + K - 1];
    a_target = P.profile[m][0];
    jd = P.profile[m][1] * P.delta_t;
    refused0 = !isfinite(v0) || !isfinite(a0) || v0 < 0.0;
    c = trajectory_queries::StopState{key0, v0, a0};
    s_refused0[tid] = refused0;
    s_bad[tid] = 0;
  }

  for (int k0 = 0; k0 < N; k0 += nc) {
    const int k1 = min(k0 + nc, N);               // rows k0 ... k1 - 1 leave in this chunk
    const int ne = min(k1, N - 1) - k0 + 1;       // image rows: those, and row k1 for the differences where it exists
    const int nw = k1 - k0;
    // ---- 2. s, velocity, a
    if (tid < nch && !refused0) {
      double* img = s_img + (size_t)tid * ni * kPF;
      for (int j = 0; j < ne; ++j) {
        if (j > 0) c = trajectory_queries::stop_step(c, a_target, jd, hd, P.delta_t);   // (j = 0: where the last chunk ended)
        if (c.s > s_end) overrun = true;
        if (knot < 0 && c.v == 0.0) knot = k0 + j;
        img[j * kPF + O.station] = c.s > s_end ? s_end : c.s;
        img[j * kPF + O.v] = c.v;
        img[j * kPF + O.a] = c.a;
      }
    }
    __syncthreads();
    // ---- 3. one image row per lane and round
    for (int e0 = 0; e0 < nch * ne; e0 += kStLanes) {
      const int e = e0 + tid;
      const int pm = e < nch * ne ? e / ne : 0, j = e - pm * ne;
      bool bad = false;
      if (e < nch * ne && !s_refused0[pm]) {
        const int p = pm / M;
        const double* T = s_rows + (size_t)p * K * F;
        const double* key = s_key + p * K;
        double* o = s_img + ((size_t)pm * ni + j) * kPF;
        const double q = o[O.station];
        const int i = bracket_pair(K, q, [&](int r) { return key[r]; });
        const double* p0 = T + (i - 1) * F;
        const double* p1 = p0 + F;
        double v[5];
        pair_step(kFiveV, -1,key[i - 1], key[i], q, p0, p1, v);
        const double t = T[C.time] + P.delta_t * (k0 + j);
        o[O.time] = t;
#pragma unroll
        for (int f = 0; f < 5; ++f) o[kFive.to[f]] = v[f];
        bad = !(isfinite(t) && isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]) && isfinite(v[4]));
      }
      mark_bad(bad, e0 + (tid & ~63), ne, s_bad);
    }
    __syncthreads();
    // ---- 4. the controls, from the next row of the image
    for (int e0 = 0; e0 < nch * nw; e0 += kStLanes) {
      const int e = e0 + tid;
      const int pm = e < nch * nw ? e / nw : 0, j = e - pm * nw;
      bool bad = false;
      if (e < nch * nw && !s_refused0[pm]) {
        double* o = s_img + ((size_t)pm * ni + j) * kPF;
        double jerk = 0.0, rate = 0.0;
        if (k0 + j < N - 1) {
          jerk = (o[O.a + kPF] - o[O.a]) / P.delta_t;
          rate = (o[O.delta + kPF] - o[O.delta]) / P.delta_t;
        }
        o[O.jerk] = jerk;
        o[O.rate] = rate;
        bad = !(isfinite(o[O.station]) && isfinite(o[O.v]) && isfinite(o[O.a]) && isfinite(jerk) && isfinite(rate));
      }
      mark_bad(bad, e0 + (tid & ~63), nw, s_bad);
    }
    __syncthreads();
    // ---- 5. the rows of the chunk: nw * 11 consecutive doubles per chain
    if (out_rows) {
      const int n = nw * kPF;
      for (int e = tid; e < nch * n; e += kStLanes) {
        const int pm = e / n, i = e - pm * n;
        const int p = pm / M, m = pm - p * M;
        double* __restrict__ g = out_rows + (((size_t)m * P.batch + b0 + p) * N + k0) * kPF;
        g[i] = s_refused0[pm] ? 0.0 : s_img[(size_t)pm * ni * kPF + i];
      }
    }
    __syncthreads();   // the image is written again, and s_bad is read below
  }

  // ---- a chain that produced a non-finite value: every row zero, whichever chunk wrote it
  if (out_rows) {
    for (int pm = 0; pm < nch; ++pm) {
      if (!s_bad[pm]) continue;
      const int p = pm / M, m = pm - p * M;
      double* __restrict__ g = out_rows + ((size_t)m * P.batch + b0 + p) * N * kPF;
      for (int i = tid; i < N * kPF; i += kStLanes) g[i] = 0.0;
    }
  }
  if (tid < nch) {
    const int p = tid / M, m = tid - p * M;
    const bool refused = refused0 || s_bad[tid];
    const size_t at = (size_t)m * P.batch + b0 + p;
    if (status)
      status[at] = refused ? CILQR_STOP_REFUSED : overrun ? CILQR_STOP_OVERRUN : c.v > 0.0 ? CILQR_STOP_MOVING : CILQR_STOP_STOPPED;
    if (stop_knot) stop_knot[at] = refused ? -1 : knot;
    if (travel) travel[at] = refused ? 0.0 : c.s - key0;
  }
}

void launch_stop(const StopParams& P, const double* rows, const double* start_va, double* out_rows, int* status,
                 int* stop_knot, double* travel, hipStream_t st) {
  // CILQR_STOP_LDS_KB, CILQR_STOP_CHUNK: tuning hooks (tools/stop_bench.py) -- the LDS a launch plans with and the knots of
  // a chunk at the most, which trade the chains a workgroup runs side by side against the passes over the knots; the rows
  // do not depend on them.  Read at every launch: the tool changes them between its timings.
  const char* forced_kb = std::getenv("CILQR_STOP_LDS_KB");
  const char* forced_nc = std::getenv("CILQR_STOP_CHUNK");
  const int kb = forced_kb ? std::atoi(forced_kb) : 0, cap = forced_nc ? std::atoi(forced_nc) : 0;
  const size_t fixed = (size_t)P.n_knots * (P.fields + 1);                     // rows and keys: at most 3072 doubles
  const size_t row = (size_t)P.n_profiles * kPF;                               // one knot in the image of every profile
  // (what one trajectory needs with kStMinImage image rows is always granted: at most 3072 + 88 * 4 doubles = 27 KiB)
  const size_t budget = std::max((kb > 0 ? (size_t)std::min(kb, 60) * 1024 : kStLdsBudget) / 8, fixed + row * kStMinImage);
  int nc = cap > 0 ? std::min(cap, P.n_out) : std::min(kStChunk, P.n_out);
  int ni = nc < P.n_out ? nc + 1 : P.n_out;                                    // (one row of look-ahead)
  if (fixed + row * ni > budget) {   // not even one trajectory: fewer knots a chunk
    ni = (int)((budget - fixed) / row);   // >= kStMinImage
    nc = ni - 1;
  }
  const int run = (int)std::min<size_t>(kStMaxRun, budget / (fixed + row * ni));
  const size_t lds = (fixed + row * ni) * run * 8;
  const dim3 grid((unsigned)(((long long)P.batch + run - 1) / run)), block(kStLanes);
  switch (P.fields) {
    case 9: hipLaunchKernelGGL(k_stop<9>, grid, block, lds, st, P, run, nc, ni, rows, start_va, out_rows, status, stop_knot, travel); break;
    case 10: hipLaunchKernelGGL(k_stop<10>, grid, block, lds, st, P, run, nc, ni, rows, start_va, out_rows, status, stop_knot, travel); break;
    case 11: hipLaunchKernelGGL(k_stop<11>, grid, block, lds, st, P, run, nc, ni, rows, start_va, out_rows, status, stop_knot, travel); break;
  }
}

// ------------------------------------------------------------------------------------------
// cilqr_stop_scenes_batch: choose and gather
// ------------------------------------------------------------------------------------------
// block (b, y): the choice of scene b (every lane finds it for itself: M <= 8 pairs of words), then words [y * 256, ...) of
// the chosen slice
__global__ __launch_bounds__(256) void k_stop_choose(int B, int M, size_t per, const int* __restrict__ status,
                                                      const int* __restrict__ first_hit, const double* __restrict__ slices,
                                                      int* __restrict__ choice, double* __restrict__ out_rows) {
  const size_t b = blockIdx.x;
  int pick = -1;
  for (int m = M - 1; m >= 0; --m)
    if (status[(size_t)m * B + b] == CILQR_STOP_STOPPED && first_hit[(size_t)m * B + b] == -1) pick = m;
  if (blockIdx.y == 0 && threadIdx.x == 0) choice[b] = pick;
  const double* __restrict__ from = slices + ((size_t)(pick < 0 ? M - 1 : pick) * B + b) * per;
  double* __restrict__ to = out_rows + b * per;
  for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.y * blockDim.x) to[i] = from[i];
}

// ONE workgroup counts the scenes without a choice: per-lane counts, then a tree over LDS -- no atomic takes part
constexpr int kCountLanes = 1024;
__global__ __launch_bounds__(kCountLanes) void k_stop_count_none(int B, const int* __restrict__ choice, int* __restrict__ n_none) {
  __shared__ int s_n[kCountLanes];
  const int tid = threadIdx.x;
  int n = 0;
  for (int b = tid; b < B; b += kCountLanes) n += choice[b] < 0;
  s_n[tid] = n;
  __syncthreads();
  for (int half = kCountLanes / 2; half > 0; half >>= 1) {
    if (tid < half) s_n[tid] += s_n[tid + half];
    __syncthreads();
  }
  if (tid == 0) *n_none = s_n[0];
}

void launch_stop_choose(int B, int M, size_t per, const int* status, const int* first_hit, const double* slices, int* choice,
                        double* out_rows, int* n_none, hipStream_t st) {
  const dim3 grid((unsigned)B, (unsigned)std::min<size_t>(64, (per + 255) / 256));
  hipLaunchKernelGGL(k_stop_choose, grid, dim3(256), 0, st, B, M, per, status, first_hit, slices, choice, out_rows);
  if (n_none) hipLaunchKernelGGL(k_stop_count_none, dim3(1), dim3(kCountLanes), 0, st, B, choice, n_none);
}

}  // namespace cilqr
