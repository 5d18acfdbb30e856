// Warm start (cilqr_warm_start, include/cilqr.h): the first iterate from control rows the caller already has, in place
// of the init guess (iqr cc:793-842 / InitGuess cc:107-139) for the problems that ask for it.
//
// Two kernels.  The controls arrive problem-major, one problem's rows kilobytes apart, and the rollout runs one lane per
// problem on the batch-fastest arena: gathered inside the rollout chain, the 64 lanes of a wave would touch 64 lines per
// step behind a dependent load.  So k_warm_gather applies the shift rule over (problem x step) and writes U of buffer 0
// through an LDS tile (as k_load_corridor does for the planes); k_warm_rollout then reads U as every rollout does.
#include "dev_model.hpp"

namespace cilqr {

// One block = 64 problems x kWarmSteps steps.  Reads: consecutive threads take consecutive rows of one problem (what
// contiguity the caller's layout has: 16 of every 80 / 88 bytes, or all of them for CILQR_ROWS_CONTROLS); writes: 64
// consecutive slots of one step, 1 KiB per wave.  The two doubles of a row are loaded one by one: the caller's rows are
// only known to be aligned as doubles.  The bits travel untouched (loads and stores, no arithmetic).
// For problem b with s = shift[b] (no shift array: 0):  s < 0: nothing is written (the init guess owns the problem);
// otherwise U_i = row i + s if s < N and i < N - s (compared without adding: any s is valid), else (0, 0).
constexpr int kWarmSteps = 16;   // 16 x 65 double2 = 16.25 KiB
__global__ __launch_bounds__(256) void k_warm_gather(DeviceState s, int B, WarmView w, int* __restrict__ shift_out) {
  __shared__ double2 tile[kWarmSteps][64 + 1];
  __shared__ int sh[64];
  const int N = s.p.N;
  const int b0 = blockIdx.x * 64, i0 = blockIdx.y * kWarmSteps;
  const int nb = min(64, B - b0), ni = min(kWarmSteps, N - i0);
  if (threadIdx.x < 64) {
    int v = -1;
    if ((int)threadIdx.x < nb) {
      v = (w.shift != nullptr) ? w.shift[b0 + threadIdx.x] : 0;
      if (blockIdx.y == 0) shift_out[b0 + threadIdx.x] = v;
    }
    sh[threadIdx.x] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nb * ni; e += blockDim.x) {
    const int q = e / ni, j = e - q * ni;
    const int i = i0 + j, sft = sh[q];
    double2 u = make_double2(0.0, 0.0);
    if (sft >= 0 && sft < N && i < N - sft) {
      const double* r = w.rows + ((size_t)(b0 + q) * w.rows_per + (size_t)(i + sft)) * w.stride + w.col;
      u = make_double2(r[0], r[1]);
    }
    tile[j][q] = u;
  }
  __syncthreads();
  const int q = threadIdx.x & 63;
  if (q >= nb || sh[q] < 0) return;
  for (int j = threadIdx.x >> 6; j < ni; j += 4) s.U[(size_t)(i0 + j) * s.Bcap + b0 + q] = tile[j][q];   // buffer 0
}

void launch_warm_gather(const DeviceState& s, int B, const WarmView& w, int* shift_out, hipStream_t st) {
  dim3 g((B + 63) / 64, (s.p.N + kWarmSteps - 1) / kWarmSteps);
  hipLaunchKernelGGL(k_warm_gather, g, dim3(256), 0, st, s, B, w, shift_out);
}

// X_0 = goals_[0], X_{i+1} = Dynamics(X_i, U_i) (OpenLoopRollout, algorithm/slover/ilqr.h:363-370): the step of k_rollout and
// of the last loop of k_init_guess, without its clamp.  One lane per warm-started problem; the others leave at once.
__global__ __launch_bounds__(64) void k_warm_rollout(DeviceState s, int B, const int* __restrict__ warm_shift) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= B) return;
  if (warm_shift[slot] < 0) return;
  const int N = s.p.N, Bc = s.Bcap;
  double x[6];
  {
    const double2* gp = s.goals + slot;
    const double2 g0 = gp[0], g1 = gp[(size_t)Bc], g2 = gp[(size_t)2 * Bc];
    x[0] = g0.x; x[1] = g0.y; x[2] = g1.x; x[3] = g1.y; x[4] = g2.x; x[5] = g2.y;
  }
  store_x(s, 0, 0, slot, x);
  for (int i = 0; i < N; ++i) {
    double u[2];
    load_u(s, 0, i, slot, u);
    dynamics(s.p, x, u, x);
    store_x(s, 0, i + 1, slot, x);
  }
}

void launch_warm_rollout(const DeviceState& s, int B, const int* warm_shift, hipStream_t st) {
  hipLaunchKernelGGL(k_warm_rollout, dim3((B + 63) / 64), dim3(64), 0, st, s, B, warm_shift);
}

}  // namespace cilqr
