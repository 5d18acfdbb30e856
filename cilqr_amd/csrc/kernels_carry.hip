// cilqr_carry_rows_batch and what cilqr_plan_scenes_batch_carry puts between its stages (include/cilqr.h, "carry").  The
// host statement is include/cilqr/trajectory_queries.hpp: carry_rows.  The bracket and the pair step are ONE function for
// both (include/cilqr/row_math.hpp: bracket_pair, pair_step over pair_carry); the checks of the advance, the chord
// lengths (row_math.hpp's hypot_ref where the host statement takes std::hypot) and their sum in knot order k_carry follows
// operation by operation (-ffp-contract=off, IEEE division), so the rows are its bits.
//
// k_carry moves memory: per trajectory it reads n_rows F doubles and writes 19 n_knots.  A workgroup of 256 lanes takes a
// run of whole trajectories -- as many as fit 48 KiB of LDS, at most 16: five for 51 plan rows and 51 knots -- so that the
// grid is a few thousand fat workgroups rather than one thin one per trajectory, and
//   1. stages their rows (contiguous in `rows`) into LDS with flat consecutive loads, 16 bytes wide where the address allows;
//   2. the (trajectory, knot) pairs are flattened over the lanes: each lane brackets its knot's time in LDS (at most 8 steps,
//      no global load depends on another), interpolates the seven columns a coarse row takes and puts them into an LDS image
//      of coarse9; a wavefront that saw a non-finite value (one ballot) marks the trajectories concerned as refused;
//   3. the chord lengths are taken in parallel; their running sums by one lane per trajectory, side by side in one wavefront,
//      over LDS values fetched eight at a time (the rule adds them in knot order);
//   4. the four outputs leave flat: consecutive lanes store consecutive doubles, all read from the LDS image.
// The image's row stride is 9 doubles: odd, so the lanes of a ds_write_b64 group spread over all banks.
#include <algorithm>

#include "../../include/cilqr/trajectory_queries.hpp"
#include "carry.hpp"
#include "dev_model.hpp"

namespace cilqr {

constexpr int kCyLanes = 256;
constexpr int kCyMaxRun = 16;                 // trajectories per workgroup, at most
constexpr size_t kCyLdsBudget = 48 * 1024;    // ... and what their rows and images may take together

// doubles of LDS one trajectory takes: its rows, its coarse9 image, its chord lengths
inline size_t carry_lds_doubles(const CarryParams& P) {
  return (size_t)P.n_rows * P.fields + (size_t)P.n_live * (CILQR_COARSE_FIELDS + 1);
}

// F: doubles per row (9 coarse, 10 traj, 11 plan).  run: trajectories per workgroup.
template <int F>
__global__ __launch_bounds__(kCyLanes) void k_carry(CarryParams P, int run, const double* __restrict__ rows,
                                                    const double* __restrict__ advance, double* __restrict__ coarse9,
                                                    double* __restrict__ coarse6, double* __restrict__ knots3,
                                                    double* __restrict__ station, int* __restrict__ state,
                                                    int* __restrict__ n_kept) {
  constexpr RowColumns C = columns_of_fields(F);
  constexpr int TC = C.time;
  constexpr PairColumns kSeven = trajectory_queries::pair_carry(C);   // x y theta kappa v a delta -> v[0 ... 6]
  extern __shared__ double s_mem[];
  __shared__ int s_state[kCyMaxRun];
  const int R = P.n_rows, K = P.n_knots, L = P.n_live;
  double* s_rows = s_mem;                                     // [run][R][F]
  double* s_out = s_rows + (size_t)run * R * F;               // [run][L][9]
  double* s_len = s_out + (size_t)run * L * CILQR_COARSE_FIELDS;   // [run][L]
  const int tid = threadIdx.x;
  const size_t b0 = (size_t)blockIdx.x * run;                 // < batch: the grid is ceil(batch / run) wide
  const int np = (int)min((size_t)run, (size_t)P.batch - b0);

  // ---- 1. the rows of the run, and what the advances say
  stage_in<kCyLanes>(rows + b0 * R * F, s_rows, np * R * F);
  __syncthreads();
  if (tid < np) {
    const double adv = advance[b0 + tid];
    const double* T = s_rows + tid * R * F;
    int st = 0;
    if (adv < 0.0) st = 1;
    else if (!(adv <= P.max_advance)) st = 2;   // a NaN, or above the limit
    else if (!(T[(R - 1) * F + TC] - T[TC] > 0.0)) st = 2;
    s_state[tid] = st;
  }
  __syncthreads();

  // ---- 2. one (trajectory, knot) pair per lane and round
  for (int e0 = 0; e0 < np * L; e0 += kCyLanes) {   // the same trips for every lane: the ballot below is met by whole waves
    const int e = e0 + tid;
    const int p = e < np * L ? e / L : 0, k = e - p * L;
    bool bad = false;
    if (e < np * L && s_state[p] == 0) {
      const double* T = s_rows + p * R * F;
      const double q = (T[TC] + advance[b0 + p]) + k * P.delta_t;
      const int i = bracket_pair(R, q, [&](int r) { return T[r * F + TC]; });
      const double* p0 = T + (i - 1) * F;
      const double* p1 = p0 + F;
      double* o = s_out + (size_t)e * CILQR_COARSE_FIELDS;
      double v[7];
      pair_step(kSeven, TC, p0[TC], p1[TC], q, p0, p1, v);
      o[0] = P.delta_t * k;
#pragma unroll
      for (int c = 0; c < 7; ++c) o[2 + c] = v[c];
      bad = !(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[4]) && isfinite(v[5]) && isfinite(v[6]));
    }
    if (__ballot(bad) != 0ull && bad) s_state[p] = 2;   // rarely: every writer of a trajectory's word writes the same value
  }
  __syncthreads();

  // ---- 3. chord lengths, then the running station: one lane per trajectory
  for (int e = tid; e < np * L; e += kCyLanes) {
    const int p = e / L, k = e - p * L;
    const double* o = s_out + (size_t)e * CILQR_COARSE_FIELDS;
    s_len[e] = (k > 0 && s_state[p] == 0) ? hypot_ref(o[2] - o[2 - CILQR_COARSE_FIELDS], o[3] - o[3 - CILQR_COARSE_FIELDS]) : 0.0;
  }
  __syncthreads();
  if (tid < np && s_state[tid] == 0) {
    const double* len = s_len + tid * L;
    double* o = s_out + (size_t)tid * L * CILQR_COARSE_FIELDS + 1;
    double s = 0.0;
    for (int k0 = 0; k0 < L; k0 += 8) {
      double t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = k0 + j < L ? len[k0 + j] : 0.0;   // eight independent loads, then the chain of sums
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s = s + t[j];
        if (k0 + j < L) o[(k0 + j) * CILQR_COARSE_FIELDS] = s;
      }
    }
  }
  __syncthreads();

  // ---- 4. the outputs: zero rows unless the trajectory is kept, and past the rows produced
  for (int p = 0; p < np; ++p) {
    const bool kept = s_state[p] == 0;
    const double* img = s_out + (size_t)p * L * CILQR_COARSE_FIELDS;
    const size_t at = (b0 + p) * K;
    if (coarse9) {
      double* __restrict__ g = coarse9 + at * 9;
      for (int i = tid; i < K * 9; i += kCyLanes) g[i] = (kept && i < L * 9) ? img[i] : 0.0;
    }
    if (coarse6) {   // x y theta velocity a delta
      double* __restrict__ g = coarse6 + at * 6;
      for (int i = tid; i < K * 6; i += kCyLanes) {
        const int k = i / 6, c = i - k * 6;
        g[i] = (kept && k < L) ? img[k * 9 + (c < 3 ? 2 + c : 3 + c)] : 0.0;
      }
    }
    if (knots3) {
      double* __restrict__ g = knots3 + at * 3;
      for (int i = tid; i < K * 3; i += kCyLanes) {
        const int k = i / 3, c = i - k * 3;
        g[i] = (kept && k < L) ? img[k * 9 + 2 + c] : 0.0;
      }
    }
    if (station) {
      double* __restrict__ g = station + at;
      for (int k = tid; k < K; k += kCyLanes) g[k] = (kept && k < L) ? img[k * 9 + 1] : 0.0;
    }
  }
  if (tid < np) state[b0 + tid] = s_state[tid];
  if (tid == 0 && n_kept) {
    int kept = 0;
    for (int p = 0; p < np; ++p) kept += s_state[p] == 0;
    if (kept) atomicAdd(n_kept, kept);
  }
}

void launch_carry(const CarryParams& P, const double* rows, const double* advance, double* coarse9, double* coarse6,
                  double* knots3, double* station, int* state, int* n_kept, hipStream_t st) {
  const size_t per = carry_lds_doubles(P) * 8;   // at most 42 KiB: one trajectory always fits
  const int run = (int)std::max<size_t>(1, std::min<size_t>(kCyMaxRun, kCyLdsBudget / per));
  const size_t lds = per * run;
  const dim3 grid((unsigned)(((long long)P.batch + run - 1) / run)), block(kCyLanes);
  switch (P.fields) {
    case 9: hipLaunchKernelGGL(k_carry<9>, grid, block, lds, st, P, run, rows, advance, coarse9, coarse6, knots3, station, state, n_kept); break;
    case 10: hipLaunchKernelGGL(k_carry<10>, grid, block, lds, st, P, run, rows, advance, coarse9, coarse6, knots3, station, state, n_kept); break;
    case 11: hipLaunchKernelGGL(k_carry<11>, grid, block, lds, st, P, run, rows, advance, coarse9, coarse6, knots3, station, state, n_kept); break;
  }
}

// ------------------------------------------------------------------------------------------
// cilqr_plan_scenes_batch_carry: select, gather, scatter
// ------------------------------------------------------------------------------------------
// ONE workgroup walks the batch in tiles of its 1024 lanes.  A listed scene's place in `sel` is the count of listed scenes
// before it: those of earlier tiles (s_base), of earlier wavefronts of its tile (their ballots' population counts) and of
// lower lanes of its own wavefront (its ballot below the lane).  No atomic takes part, so the list is in scene order.
constexpr int kSelLanes = 1024;
__global__ __launch_bounds__(kSelLanes) void k_carry_select(int B, int K, const int* __restrict__ state,
                                                            const double* __restrict__ start4,
                                                            const double* __restrict__ coarse9,
                                                            const int* __restrict__ first_hit, double max_start_offset,
                                                            int* __restrict__ source, int* __restrict__ found,
                                                            int* __restrict__ sel, int* __restrict__ n_sel) {
  __shared__ int s_wave[kSelLanes / 64];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += kSelLanes) {
    const int b = b0 + tid;
    int src = CILQR_CARRY_KEPT;
    if (b < B) {
      const double* row0 = coarse9 + (size_t)b * K * CILQR_COARSE_FIELDS;
      const double* s4 = start4 + (size_t)b * 4;
      if (state[b] == CILQR_CARRY_NOT_ASKED) src = CILQR_CARRY_NOT_ASKED;
      else if (state[b] != CILQR_CARRY_KEPT) src = CILQR_CARRY_REFUSED;
      else if (!(hypot_ref(s4[0] - row0[2], s4[1] - row0[3]) <= max_start_offset)) src = CILQR_CARRY_OFF_START;
      else if (first_hit[b] != -1) src = CILQR_CARRY_HIT;
      if (source) source[b] = src;
      found[b] = src == CILQR_CARRY_KEPT ? 1 : 0;
    }
    const bool listed = src != CILQR_CARRY_KEPT;
    const unsigned long long m = __ballot(listed);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = s_base;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (listed) sel[before + __popcll(m & ((1ull << lane) - 1ull))] = b;
    __syncthreads();
    if (tid == 0) {
      int all = 0;
      for (int w = 0; w < kSelLanes / 64; ++w) all += s_wave[w];
      s_base += all;
    }
    __syncthreads();
  }
  if (tid == 0) *n_sel = s_base;
}

void launch_carry_select(int B, int n_knots, const int* state, const double* start4, const double* coarse9,
                         const int* first_hit, double max_start_offset, int* source, int* found, int* sel, int* n_sel,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_carry_select, dim3(1), dim3(kSelLanes), 0, st, B, n_knots, state, start4, coarse9, first_hit,
                     max_start_offset, source, found, sel, n_sel);
}

// block (j, y): words [y * blockDim, ...) of packed block j <-> full block sel[first + j]; T = 8 or 4 bytes
template <typename T, bool Scatter>
__global__ __launch_bounds__(256) void k_carry_move(T* __restrict__ full, T* __restrict__ packed, size_t per,
                                                    const int* __restrict__ sel, int first) {
  const size_t j = blockIdx.x;
  const size_t at = (size_t)sel[first + j];
  for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.y * blockDim.x) {
    if (Scatter) full[at * per + i] = packed[j * per + i];
    else packed[j * per + i] = full[at * per + i];
  }
}

template <bool Scatter>
static void carry_move(void* full, void* packed, size_t per_bytes, const int* sel, int first, int n, hipStream_t st) {
  if (full == nullptr || packed == nullptr || per_bytes == 0 || n <= 0) return;
  const bool wide = per_bytes % 8 == 0 && (reinterpret_cast<uintptr_t>(full) & 7) == 0 && (reinterpret_cast<uintptr_t>(packed) & 7) == 0;
  const size_t per = per_bytes / (wide ? 8 : 4);
  const dim3 grid((unsigned)n, (unsigned)std::min<size_t>(64, (per + 255) / 256));
  if (wide)
    hipLaunchKernelGGL((k_carry_move<unsigned long long, Scatter>), grid, dim3(256), 0, st, static_cast<unsigned long long*>(full),
                       static_cast<unsigned long long*>(packed), per, sel, first);
  else
    hipLaunchKernelGGL((k_carry_move<unsigned, Scatter>), grid, dim3(256), 0, st, static_cast<unsigned*>(full),
                       static_cast<unsigned*>(packed), per, sel, first);
}

void launch_carry_gather(const void* full, void* packed, size_t per_bytes, const int* sel, int first, int n, hipStream_t st) {
  carry_move<false>(const_cast<void*>(full), packed, per_bytes, sel, first, n, st);
}
void launch_carry_scatter(void* full, const void* packed, size_t per_bytes, const int* sel, int first, int n, hipStream_t st) {
  carry_move<true>(full, const_cast<void*>(packed), per_bytes, sel, first, n, st);
}

}  // namespace cilqr
