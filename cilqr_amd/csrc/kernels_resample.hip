// cilqr_resample_rows_batch (include/cilqr.h, "resample"): DiscretizedTrajectory::EvaluateTime / EvaluateStation for
// every (trajectory, query) pair of a batch.  The host statement is include/cilqr/trajectory_queries.hpp: resample_rows.
// The bracket and the pair step are ONE function for both (include/cilqr/row_math.hpp: bracket_pair, pair_step over
// pair_all, built with -ffp-contract=off and IEEE division here as there), so the rows are its bits; what this file adds
// is where the rows lie while that runs.
//
// The kernel moves memory: it reads B K F doubles once and writes B M F.  A lane per query working on global memory would
// store F-double rows at an F-double stride and bisect through HBM behind dependent loads.  Instead the work items are the
// (problem, query) pairs flattened -- problem-major, which is also the order of `out`, so a run of items is ONE contiguous
// piece of the output -- and a workgroup of 256 lanes
//   1. takes a run of whole problems and stages their rows (contiguous in `rows`) into LDS with flat consecutive loads;
//   2. per tile of 256 items: each lane bisects its problem's key column in LDS (at most 8 steps for K <= 256, no global
//      load depends on another), computes its row and puts it into an LDS tile;
//   3. the tile leaves flat: consecutive lanes store consecutive doubles of `out`.
// Global accesses are 16 bytes wide where the address allows: the caller's arrays are only known to be aligned as doubles,
// so a piece that starts on an odd double moves its first (and, as it comes, last) double alone.
// LDS: rows 24 KiB (one problem at K = 256 in the 11-column layout is 22 KiB) + tile 256 x 11 doubles = 22 KiB.  The tile's
// row stride is F | 1 doubles: an odd number of doubles is an even, non-multiple-of-4 number of dwords, which spreads the 16
// lanes of a ds_write_b64 group over all 32 banks (stride 10 would put lanes l and l + 8 on one bank pair).
#include "dev_model.hpp"
#include "resample.hpp"

namespace cilqr {

constexpr int kRsLanes = 256;
constexpr int kRsRowDoubles = 3072;   // >= CILQR_DP_MAX_KNOTS * CILQR_PLAN_FIELDS = 2816
constexpr int kRsItems = 2048;        // items a workgroup aims for (8 tiles): what its staged rows are shared among
static_assert(kRsRowDoubles >= CILQR_DP_MAX_KNOTS * CILQR_PLAN_FIELDS, "one problem must fit the row image");

// F: doubles per row (9 coarse, 10 traj, 11 plan)
template <int F>
__global__ __launch_bounds__(kRsLanes) void k_resample(ResampleParams P, int probs_per_wg, unsigned chunk,
                                                       const double* __restrict__ rows, const double* __restrict__ queries,
                                                       double* __restrict__ out) {
  constexpr PairColumns kAll = pair_all(columns_of_fields(F));   // every column in place
  constexpr int FS = F | 1;
  __shared__ double s_rows[kRsRowDoubles];
  __shared__ double s_out[kRsLanes * FS];
  const int tid = threadIdx.x;
  const int K = P.n_knots, kc = P.key_col;
  const unsigned M = (unsigned)P.n_queries;
  const int b0 = (int)blockIdx.x * probs_per_wg;   // < batch: the grid is ceil(batch / probs_per_wg) wide
  const int np = min(probs_per_wg, P.batch - b0);
  // items of this workgroup: [c0, c1) of the run's np * M (the host chose probs_per_wg so that this fits 32 bits)
  const unsigned n_items = (unsigned)np * M;
  const unsigned c0 = min(n_items, blockIdx.y * chunk);
  const unsigned c1 = (n_items - c0 < chunk) ? n_items : c0 + chunk;
  if (c0 >= c1) return;   // the last run of a batch can be shorter than the grid's second dimension covers

  stage_in<kRsLanes>(rows + (size_t)b0 * K * F, s_rows, np * K * F);
  __syncthreads();

  for (unsigned t0 = c0; t0 < c1; t0 += kRsLanes) {
    const int n = (int)min((unsigned)kRsLanes, c1 - t0);
    if (tid < n) {
      const unsigned e = t0 + tid;
      const unsigned p = e / M, m = e - p * M;
      const double q = P.per_problem ? queries[(size_t)(b0 + p) * M + m] : queries[m];
      const double* R = s_rows + (int)p * K * F;
      const int i = bracket_pair(K, q, [&](int r) { return R[r * F + kc]; });
      const double* p0 = R + (i - 1) * F;
      const double* p1 = p0 + F;
      pair_step(kAll, kc, p0[kc], p1[kc], q, p0, p1, s_out + tid * FS);
    }
    __syncthreads();
    // ---- the tile leaves: n * F consecutive doubles of `out`
    {
      double* __restrict__ g = out + ((size_t)b0 * M + t0) * F;
      const int nd = n * F;
      const int head = min((int)((reinterpret_cast<uintptr_t>(g) >> 3) & 1), nd);
      if (head && tid == 0) g[0] = s_out[0];
      const int pairs = (nd - head) >> 1;
      for (int j = tid; j < pairs; j += kRsLanes) {
        const int i0 = head + 2 * j, i1 = i0 + 1;
        const int r0 = i0 / F, r1 = i1 / F;
        *reinterpret_cast<double2*>(g + i0) = make_double2(s_out[r0 * FS + (i0 - r0 * F)], s_out[r1 * FS + (i1 - r1 * F)]);
      }
      if (((nd - head) & 1) && tid == kRsLanes - 1) {
        const int il = nd - 1, rl = il / F;
        g[il] = s_out[rl * FS + (il - rl * F)];
      }
    }
    __syncthreads();
  }
}

void launch_resample(const ResampleParams& P, const double* rows, const double* queries, double* out, hipStream_t st) {
  const unsigned M = (unsigned)P.n_queries;
  // whole problems per workgroup: as many as the row image holds, no more than it takes to reach kRsItems items
  const int fit = kRsRowDoubles / (P.n_knots * P.fields);
  const int want = (int)((kRsItems + M - 1) / M);   // 1 for M >= kRsItems: probs_per_wg * M then is M, which fits 32 bits
  const int probs_per_wg = max(1, min(fit, want));
  const unsigned long long run_items = (unsigned long long)probs_per_wg * M;   // < 2^31 + kRsItems
  unsigned long long chunk = (run_items + 32767) / 32768;                      // the grid's second dimension stays <= 32768
  chunk = (chunk + kRsLanes - 1) / kRsLanes * kRsLanes;
  if (chunk < (unsigned)kRsItems) chunk = kRsItems;
  const dim3 grid((unsigned)(((long long)P.batch + probs_per_wg - 1) / probs_per_wg), (unsigned)((run_items + chunk - 1) / chunk));
  const unsigned ch = (unsigned)chunk;
  switch (P.fields) {
    case 9: hipLaunchKernelGGL(k_resample<9>, grid, dim3(kRsLanes), 0, st, P, probs_per_wg, ch, rows, queries, out); break;
    case 10: hipLaunchKernelGGL(k_resample<10>, grid, dim3(kRsLanes), 0, st, P, probs_per_wg, ch, rows, queries, out); break;
    case 11: hipLaunchKernelGGL(k_resample<11>, grid, dim3(kRsLanes), 0, st, P, probs_per_wg, ch, rows, queries, out); break;
  }
}

}  // namespace cilqr
