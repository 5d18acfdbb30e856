// cilqr_policy_gains_batch / cilqr_policy_rollout_batch (include/cilqr.h, "policy"): the kernels.
//
// k_policy_rollout is Forward (cc:392-415) from a start the caller chooses, for S starts per problem.  One lane per (problem,
// sample) chain, no arithmetic across lanes: a chain's bits are those of the solve's own rollout (forward_core) on the same
// operands, whatever tile it lands in.  The arithmetic is a dependent fp64 chain per lane; what the kernel is shaped around is
// memory:
//   in   the nominal rows and the gains of a problem (8 + 14 doubles per step, B N 22 8 bytes) are shared by its S samples.
//        A workgroup takes WHOLE problems -- np = Lanes / S of them, all S samples of each -- so they are read once per problem;
//        they come in through LDS in chunks of C steps (stage_pieces_in: 16-byte loads, consecutive lanes on consecutive
//        pairs of a piece of C F, C 12 and C 2 doubles), because a whole horizon of np problems does not fit beside the tile out;
//   out  S B n_out 80 bytes.  A lane's rows of a chunk go into an LDS tile and leave flat (stage_pieces_out): a piece of C 80
//        contiguous bytes per chain, consecutive lanes on consecutive pairs, instead of 80-byte rows at a stride of n_out 80.
// Lanes are dealt sample-major inside the workgroup (lane = s np + p): consecutive lanes hold consecutive problems, so the
// start states and the summaries, which are [S][B], move in runs of np chains.
// C is the largest number of steps whose images fit the LDS the launch plans with (policy.hpp), at most kPoMaxChunk: 2 for
// S = 1 (64 problems a workgroup: their images are what fills LDS), 3 to 4 for S = 8 ... 64, 2 for S > 64 (the tile out of
// 256 chains).  Nothing a chain computes depends on C.
#include <algorithm>
#include <cstdlib>

#include "policy.hpp"

namespace cilqr {

// ---------------------------------------------------------------------------------------------
// the gains call's two steps around the stage chain
// ---------------------------------------------------------------------------------------------
__global__ void k_policy_set_rows(DeviceState s, int B, RowColumns c, const double* __restrict__ rows) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = s.p.K, N = s.p.N;
  if (t >= B * K) return;
  const int slot = t / K, i = t - slot * K;
  const int buf = s.cur[slot];
  const double* r = rows + ((size_t)slot * K + i) * c.fields;
  const double x[6] = {r[c.x], r[c.y], r[c.theta], r[c.v], r[c.a], r[c.delta]};
  store_x(s, buf, i, slot, x);
  if (i < N) {
    const double u[2] = {r[c.jerk], r[c.rate]};
    store_u(s, buf, i, slot, u);
  }
  if (i == 0) s.upd[slot] = 1;
}
void launch_policy_set_rows(const DeviceState& s, int B, const RowColumns& cols, const double* rows, hipStream_t st) {
  const int n = B * s.p.K;
  hipLaunchKernelGGL(k_policy_set_rows, dim3((n + 255) / 256), dim3(256), 0, st, s, B, cols, rows);
}

__global__ void k_policy_mask(DeviceState s, int B, double* __restrict__ Kfb, double* __restrict__ kff,
                              double* __restrict__ dV, int* __restrict__ ok) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = s.p.N;
  if (t >= B * N) return;
  const int slot = t / N, i = t - slot * N;
  const bool dead = s.status[s.pid[slot]] == 6;   // CILQR_ST_NO_CORRIDOR
  if (i == 0 && ok != nullptr) ok[slot] = dead ? 0 : 1;
  if (!dead) return;
  double* o = Kfb + ((size_t)slot * N + i) * 12;
  for (int e = 0; e < 12; ++e) o[e] = 0.0;
  kff[((size_t)slot * N + i) * 2] = 0.0;
  kff[((size_t)slot * N + i) * 2 + 1] = 0.0;
  if (i == 0 && dV != nullptr) {
    dV[(size_t)slot * 2] = 0.0;
    dV[(size_t)slot * 2 + 1] = 0.0;
  }
}
void launch_policy_mask(const DeviceState& s, int B, double* Kfb, double* kff, double* dV, int* ok, hipStream_t st) {
  const int n = B * s.p.N;
  hipLaunchKernelGGL(k_policy_mask, dim3((n + 255) / 256), dim3(256), 0, st, s, B, Kfb, kff, dV, ok);
}

// ---------------------------------------------------------------------------------------------
// the rollout
// ---------------------------------------------------------------------------------------------
// LDS doubles of one problem's chunk image (rows | K | k, each C steps; + 1: an odd stride spreads the problems of a wave
// over the banks) and of one chain's tile out
__host__ __device__ constexpr int po_in_stride(int C, int F) { return (C * (F + 14)) | 1; }
__host__ __device__ constexpr int po_out_stride(int C) { return (C * CILQR_TRAJ_FIELDS) | 1; }

template <int Lanes>
__global__ __launch_bounds__(Lanes) void k_policy_rollout(PolicyParams P, int np_wg, int C, const double* __restrict__ rows,
                                                          const double* __restrict__ Kfb, const double* __restrict__ kff,
                                                          const double* __restrict__ start6, double* __restrict__ out_rows,
                                                          double* __restrict__ max_dev, double* __restrict__ end_dev,
                                                          int* __restrict__ n_clamped) {
  extern __shared__ double s_po[];
  const int tid = threadIdx.x;
  const RowColumns c = P.cols;
  const int F = c.fields, K = P.n_knots, N = K - 1, S = P.n_samples, n_out = P.n_out;
  const size_t B = (size_t)P.batch;
  const int b0 = (int)blockIdx.x * np_wg;              // < batch: the grid is ceil(batch / np_wg) wide
  const int np = min(np_wg, P.batch - b0);
  const int chains = np * S;                           // <= Lanes
  const int in_stride = po_in_stride(C, F), out_stride = po_out_stride(C);
  double* s_in = s_po;                                 // [np][in_stride]
  double* s_out = s_po + np_wg * in_stride;            // [Lanes][out_stride], with out_rows only

  const bool live = tid < chains;
  const int smp = live ? tid / np : 0, p = live ? tid - smp * np : 0;
  const size_t chain = (size_t)smp * B + (size_t)(b0 + p);   // its place in every [S][B] array

  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (live) {
#pragma unroll
    for (int e = 0; e < 6; ++e) x[e] = start6[chain * 6 + e];
  }
  double dev_max = 0.0, dev_last = 0.0;
  int clamped = 0;

  for (int i0 = 0; i0 < n_out; i0 += C) {
    const int cn = min(C, n_out - i0);                 // rows recorded in this chunk: i0 ... i0 + cn - 1
    const int gn = min(cn, n_out - 1 - i0);            // ... of which steps are taken from: those before the last row
    // ---- the chunk of every problem of the workgroup: rows i0 ... of [K], gains i0 ... of [N] (i0 + gn <= n_out - 1 <= N)
    stage_pieces_in<Lanes>(rows + ((size_t)b0 * K + i0) * F, (size_t)K * F, s_in, in_stride, np, cn * F);
    stage_pieces_in<Lanes>(Kfb + ((size_t)b0 * N + i0) * 12, (size_t)N * 12, s_in + C * F, in_stride, np, gn * 12);
    if (P.has_kff) stage_pieces_in<Lanes>(kff + ((size_t)b0 * N + i0) * 2, (size_t)N * 2, s_in + C * (F + 12), in_stride, np, gn * 2);
    __syncthreads();
    if (live) {
      const double* img = s_in + p * in_stride;
      for (int d = 0; d < cn; ++d) {
        const int i = i0 + d;
        const double* r = img + d * F;
        const double xs[6] = {r[c.x], r[c.y], r[c.theta], r[c.v], r[c.a], r[c.delta]};
        double dx[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) dx[e] = x[e] - xs[e];                       // theta NOT wrapped (cc:407)
        const double d2 = dx[0] * dx[0] + dx[1] * dx[1];
        dev_max = i == 0 ? d2 : policy_max(dev_max, d2);
        dev_last = d2;
        double u[2] = {0.0, 0.0};
        double xn[6] = {x[0], x[1], x[2], x[3], x[4], x[5]};
        if (i < n_out - 1) {
          FwdStep f;
          f.u = make_double2(r[c.jerk], r[c.rate]);
          const double* g = img + C * F + d * 12;
#pragma unroll
          for (int q = 0; q < 6; ++q) f.kk[q] = make_double2(g[2 * q], g[2 * q + 1]);
          if (P.has_kff) {
            const double* kf = img + C * (F + 12) + d * 2;
            f.kk[6] = make_double2(kf[0], kf[1]);
            control_law(f, dx, P.alpha, u);
          } else {
            policy_feedback(f, dx, u);
          }
          if (P.clamp) {
            bool hit = false;
            u[0] = policy_clamp(u[0], P.jerk_min, P.jerk_max, &hit);
            u[1] = policy_clamp(u[1], P.rate_min, P.rate_max, &hit);
            clamped += hit ? 1 : 0;
          }
          closed_loop_step<false>(P.dyn, x, u, xn);                             // cc:408-410
        }
        if (out_rows != nullptr) {                                              // write_traj_point's expressions
          double* o = s_out + tid * out_stride + d * CILQR_TRAJ_FIELDS;
          o[0] = i * P.dyn.dt;
          o[1] = x[0]; o[2] = x[1]; o[3] = x[2]; o[4] = x[3]; o[5] = x[4]; o[6] = x[5];
          o[7] = tan(x[5]) / P.dyn.wheel_base;
          o[8] = u[0]; o[9] = u[1];
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) x[e] = xn[e];
      }
    }
    __syncthreads();
    if (out_rows != nullptr) {
      // ---- the tile leaves: chain t's cn rows are one piece of out_rows [S][B][n_out][10]
      stage_pieces_out<Lanes>(out_rows, [&](int t) {
        const int ts = t / np, tp = t - ts * np;
        return (((size_t)ts * B + (size_t)(b0 + tp)) * n_out + i0) * CILQR_TRAJ_FIELDS;
      }, s_out, out_stride, chains, cn * CILQR_TRAJ_FIELDS);
      __syncthreads();
    }
  }
  if (live) {
    if (max_dev != nullptr) max_dev[chain] = sqrt(dev_max);
    if (end_dev != nullptr) end_dev[chain] = sqrt(dev_last);
    if (n_clamped != nullptr) n_clamped[chain] = clamped;
  }
}

namespace {
// the steps per chunk whose images fit `budget` bytes of LDS
int po_chunk(int np_wg, int lanes, int F, bool with_rows, size_t budget) {
  int C = kPoMaxChunk;
  while (C > 1 && ((size_t)np_wg * po_in_stride(C, F) + (with_rows ? (size_t)lanes * po_out_stride(C) : 0)) * 8 > budget) --C;
  return C;
}
}  // namespace

void launch_policy_rollout(const PolicyParams& P, const double* rows, const double* Kfb, const double* kff, const double* start6,
                           double* out_rows, double* max_dev, double* end_dev, int* n_clamped, hipStream_t st) {
  const bool small = P.n_samples <= kPoLanesSmall;
  const int lanes = small ? kPoLanesSmall : kPoLanesLarge;
  const int np_wg = lanes / P.n_samples;               // >= 1: n_samples <= CILQR_POLICY_MAX_SAMPLES
  const int F = P.cols.fields;
  const bool with_rows = out_rows != nullptr;
  // CILQR_POLICY_LDS_KB: a tuning hook (tools/policy_bench.py) -- the LDS a launch plans with, which trades the length of the
  // pieces that leave (C 80 bytes) against the workgroups a CU holds; the rows do not depend on it
  const char* forced = std::getenv("CILQR_POLICY_LDS_KB");   // read at every launch: the tool changes it between its timings
  const int forced_kb = forced ? std::atoi(forced) : 0;
  const size_t budget = forced_kb > 0 ? (size_t)std::min(forced_kb, 60) * 1024 : (!small ? kPoLdsLarge : P.n_samples < kPoFewSamples ? kPoLdsFewSamples : kPoLdsSmall);
  const int C = po_chunk(np_wg, lanes, F, with_rows, budget);
  // (C = 1 always fits: 64 problems x 26 doubles + 64 x 11 doubles = 19 KiB; 3 x 26 + 256 x 11 doubles = 23 KiB)
  const size_t lds = ((size_t)np_wg * po_in_stride(C, F) + (with_rows ? (size_t)lanes * po_out_stride(C) : 0)) * 8;
  const dim3 grid((unsigned)((P.batch + np_wg - 1) / np_wg));
  if (small)
    hipLaunchKernelGGL(k_policy_rollout<kPoLanesSmall>, grid, dim3(kPoLanesSmall), lds, st, P, np_wg, C, rows, Kfb, kff, start6,
                       out_rows, max_dev, end_dev, n_clamped);
  else
    hipLaunchKernelGGL(k_policy_rollout<kPoLanesLarge>, grid, dim3(kPoLanesLarge), lds, st, P, np_wg, C, rows, Kfb, kff, start6,
                       out_rows, max_dev, end_dev, n_clamped);
}

}  // namespace cilqr
