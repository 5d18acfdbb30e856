// Private to cilqr_amd/csrc: what policy_batch.hip (the entry points cilqr_policy_gains_batch / cilqr_policy_rollout_batch,
// include/cilqr.h "policy") and kernels_policy.hip share -- the parameters of a launch, the launch functions -- and the
// device statement of what the rollout adds to the solve's own step (search_core.hpp: control_law; dev_model.hpp:
// closed_loop_step): the control law without its feed-forward term, the clamp, the squared deviation, and the movement of
// several equal pieces between global memory and LDS.  Every pointer of a launch is device memory; nothing here synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cilqr.h"
#include "../../include/cilqr/row_layouts.hpp"
#include "search_core.hpp"

namespace cilqr {

constexpr int kPoLanesSmall = 64;    // lanes of a workgroup for up to 64 samples per problem
constexpr int kPoLanesLarge = 256;   // ... for up to CILQR_POLICY_MAX_SAMPLES
static_assert(CILQR_POLICY_MAX_SAMPLES <= kPoLanesLarge, "the samples of a problem share ONE workgroup");
constexpr int kPoMaxChunk = 8;       // steps of a problem in LDS at a time, at most
// dynamic LDS a launch plans with.  It trades the length of the pieces that leave (C 80 bytes) against the workgroups a CU
// holds, and the second matters more once the samples multiply the waves (tools/policy_bench.py, 65536 plans, all rows, two
// runs: S = 8 1.91 / 1.86 ms at 40 KiB, 1.40 / 1.35 at 24, 1.23 / 1.18 at 16; S = 32 6.01 / 5.79, 4.11 / 3.86, 4.48 / 3.28);
// below 8 samples a launch has few waves anyway and the longer pieces win (S = 1: 0.62 / 0.59 ms at 40 KiB, 0.69 / 0.65 at 16)
constexpr size_t kPoLdsFewSamples = 40 * 1024, kPoLdsSmall = 24 * 1024, kPoLdsLarge = 60 * 1024;
constexpr int kPoFewSamples = 8;     // below this many samples per problem: kPoLdsFewSamples

struct PolicyParams {
  DynP dyn;                                   // the handle's dt and wheel base
  double jerk_min, jerk_max, rate_min, rate_max;
  double alpha;
  int batch, n_knots, n_samples, n_out;
  int clamp, has_kff;
  RowColumns cols;                            // of the nominal rows (row_layouts.hpp)
};

// the gains call: the state columns of all K rows and the control columns of the first N of rows [B][K][fields] become the
// current iterate of the problems the handle has loaded (what k_set_trajectory does with X and U cut out on the host)
void launch_policy_set_rows(const DeviceState& s, int B, const RowColumns& cols, const double* rows, hipStream_t st);
// ... and its last step: ok [B] (nullable) = 0 for a problem the load flagged CILQR_ST_NO_CORRIDOR, whose K, k and dV
// (nullable) become zeros; 1 for every other, whose outputs stay as they are
void launch_policy_mask(const DeviceState& s, int B, double* Kfb, double* kff, double* dV, int* ok, hipStream_t st);
// the rollout; out_rows, max_dev, end_dev, n_clamped: each nullable
void launch_policy_rollout(const PolicyParams& P, const double* rows, const double* Kfb, const double* kff, const double* start6,
                           double* out_rows, double* max_dev, double* end_dev, int* n_clamped, hipStream_t st);

// ---- the rule (include/cilqr.h, "policy")
// control_law (cc:407) without the feed-forward term: u = u* + K dx, the feedback summed in control_law's order
CILQR_DEV void policy_feedback(const FwdStep& c, const double* dx, double* u) {
  const double us[2] = {c.u.x, c.u.y};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    double acc = c.kk[r * 3].x * dx[0];
    acc += c.kk[r * 3].y * dx[1];
    acc += c.kk[r * 3 + 1].x * dx[2];
    acc += c.kk[r * 3 + 1].y * dx[3];
    acc += c.kk[r * 3 + 2].x * dx[4];
    acc += c.kk[r * 3 + 2].y * dx[5];
    u[r] = us[r] + acc;
  }
}
// u limited to [lo, hi]; a NaN passes.  *hit |= the limit was applied
CILQR_DEV double policy_clamp(double u, double lo, double hi, bool* hit) {
  *hit |= (u < lo) || (u > hi);
  return u < lo ? lo : (u > hi ? hi : u);
}
// the larger of two squared deviations, a NaN staying once it is there
CILQR_DEV double policy_max(double m, double d2) { return (d2 > m || d2 != d2) ? d2 : m; }

// `pieces` pieces of n doubles each, piece q at g + q * gstride in global memory and at s + q * sstride in LDS, moved in by
// the Lanes lanes of a workgroup: stage_in's rule (dev_model.hpp) for every piece -- 16 bytes per lane and load where the
// piece's address allows, its first and last double alone where it starts on an odd double -- with the pairs of ALL pieces
// dealt to the lanes at once, so that short pieces still fill the wave
template <int Lanes>
CILQR_DEV void stage_pieces_in(const double* __restrict__ g, size_t gstride, double* s, int sstride, int pieces, int n) {
  if (n <= 0) return;
  const int per = (n >> 1) + 1;   // work items of a piece: its pairs, and one for the doubles that travel alone
  for (int j = threadIdx.x; j < pieces * per; j += Lanes) {
    const int q = j / per, w = j - q * per;
    const double* gp = g + (size_t)q * gstride;
    double* sp = s + q * sstride;
    const int head = (int)((reinterpret_cast<uintptr_t>(gp) >> 3) & 1);   // n >= 1
    const int pairs = (n - head) >> 1;                                     // <= per - 1
    if (w < pairs) {
      const int i = head + 2 * w;
      const double2 v = *reinterpret_cast<const double2*>(gp + i);
      sp[i] = v.x;
      sp[i + 1] = v.y;
    } else if (w == per - 1) {
      if (head) sp[0] = gp[0];
      if ((n - head) & 1) sp[n - 1] = gp[n - 1];
    }
  }
}
// the way out: piece q of LDS (s + q * sstride, n doubles) to g + off(q), off in doubles
template <int Lanes, class Off>
CILQR_DEV void stage_pieces_out(double* __restrict__ g, Off off, const double* s, int sstride, int pieces, int n) {
  if (n <= 0) return;
  const int per = (n >> 1) + 1;
  for (int j = threadIdx.x; j < pieces * per; j += Lanes) {
    const int q = j / per, w = j - q * per;
    double* gp = g + off(q);
    const double* sp = s + q * sstride;
    const int head = (int)((reinterpret_cast<uintptr_t>(gp) >> 3) & 1);
    const int pairs = (n - head) >> 1;
    if (w < pairs) {
      const int i = head + 2 * w;
      *reinterpret_cast<double2*>(gp + i) = make_double2(sp[i], sp[i + 1]);
    } else if (w == per - 1) {
      if (head) gp[0] = sp[0];
      if ((n - head) & 1) gp[n - 1] = sp[n - 1];
    }
  }
}

}  // namespace cilqr
