// Private to cilqr_amd/csrc: the caller arrays of a solve, stated ONCE -- elements per problem, problems [b0, b1) of a batch,
// the two packed blocks HOST arrays travel through (solver.hip: stage_inputs, job_begin, job_finish) and the hand-out of the
// one that comes back.  Plain C++ without HIP: tests/cpp/solve_io_test.cc builds it with g++ alone.
#pragma once
#include <algorithm>
#include <cstring>

#include "../../include/cilqr.h"
#include "../../include/cilqr/row_layouts.hpp"

static_assert(cilqr::row_columns(CILQR_ROWS_TRAJ).fields == CILQR_TRAJ_FIELDS && cilqr::row_columns(CILQR_ROWS_PLAN).fields == CILQR_PLAN_FIELDS &&
                  cilqr::row_columns(CILQR_ROWS_COARSE).fields == CILQR_COARSE_FIELDS && cilqr::row_columns(CILQR_ROWS_CONTROLS).fields == CILQR_NU &&
                  cilqr::row_columns(CILQR_ROWS_POINTS).fields == 2 && cilqr::kMaxRowFields == CILQR_PLAN_FIELDS,
              "row_layouts.hpp states the layouts of cilqr.h");

// doubles per row, rows per problem and first control column of a warm layout (n_knots = N + 1); false: no such layout
inline bool cilqr_warm_geometry(int32_t layout, int32_t n_knots, int* stride, int* rows_per, int* col) {
  const cilqr::RowColumns c = cilqr::row_columns(layout);
  if (c.jerk < 0) return false;   // CILQR_ROWS_COARSE and CILQR_ROWS_POINTS carry no controls
  *stride = c.fields;
  *rows_per = layout == CILQR_ROWS_CONTROLS ? n_knots - 1 : n_knots;   // a control per step; a trajectory row per knot
  *col = c.jerk;
  return true;
}

namespace cilqr {

constexpr size_t kSmallTransfer = (size_t)4 << 20;   // host batches up to this many bytes travel as one pinned block each way

// one array's place in a block
struct slot {
  size_t off = 0, bytes = 0;
  template <typename T>
  T* in(void* block) const { return reinterpret_cast<T*>(static_cast<char*>(block) + off); }
};

// slots in the order asked for, each at the next multiple of `align` bytes (staging.hpp's blocks: 256; a solve's: packed)
class block_layout {
 public:
  explicit block_layout(size_t align = 256) : align_(align) {}
  slot add(size_t bytes) { const slot s{end_, bytes}; end_ += (bytes + align_ - 1) / align_ * align_; return s; }
  void pad_to(size_t n) { end_ = (end_ + n - 1) / n * n; }
  size_t bytes() const { return end_; }   // of all slots handed out so far

 private:
  size_t align_, end_ = 0;
};

// ---- elements per problem of every caller array: everything below is derived from these three functions
struct problem_widths { size_t start, coarse, corridor, corridor_count, coarse_station; };
struct solution_widths { size_t traj, cost_hist, iter_trajs, alpha_trace, count; };   // count: each of the four [B] arrays
struct warm_widths { size_t rows, shift; };
inline problem_widths widths(const cilqr_problem_batch& in) {
  const size_t K = (size_t)in.n_knots;
  return {4, K * 6, K * (size_t)in.cmax * 3, K, K};
}
inline solution_widths widths(const cilqr_solution_batch& out, int n_knots, int max_iter) {
  const size_t K = (size_t)n_knots, M = (size_t)max_iter;
  return {K * CILQR_TRAJ_FIELDS, (M + 1) * CILQR_COST_FIELDS, (size_t)std::max(out.max_iter_trajs, 0) * K * CILQR_TRAJ_FIELDS, M, 1};
}
inline warm_widths widths(const cilqr_warm_start& warm, int n_knots) {   // (an unknown layout: no rows)
  int stride = 0, rows_per = 0, col = 0;
  (void)cilqr_warm_geometry(warm.layout, n_knots, &stride, &rows_per, &col);
  return {(size_t)rows_per * stride, 1};
}

// ---- problems [b0, b1) of a batch (lane groups, shards): an array the caller did not give stays NULL
template <class T> T* from_problem(T* a, int b0, size_t width) { return a ? a + (size_t)b0 * width : nullptr; }

inline cilqr_problem_batch slice(cilqr_problem_batch s, int b0, int b1) {   // (the lane tables: the caller's business)
  const problem_widths w = widths(s);
  s.batch = b1 - b0;
  s.start = from_problem(s.start, b0, w.start);
  s.coarse = from_problem(s.coarse, b0, w.coarse);
  s.corridor = from_problem(s.corridor, b0, w.corridor);
  s.corridor_count = from_problem(s.corridor_count, b0, w.corridor_count);
  s.coarse_station = from_problem(s.coarse_station, b0, w.coarse_station);
  return s;
}
inline cilqr_solution_batch slice(cilqr_solution_batch s, int b0, int /*b1*/, int n_knots, int max_iter) {
  const solution_widths w = widths(s, n_knots, max_iter);
  s.traj = from_problem(s.traj, b0, w.traj);
  s.cost_hist = from_problem(s.cost_hist, b0, w.cost_hist);
  s.n_cost = from_problem(s.n_cost, b0, w.count);
  s.status = from_problem(s.status, b0, w.count);
  s.n_iter = from_problem(s.n_iter, b0, w.count);
  s.iter_trajs = from_problem(s.iter_trajs, b0, w.iter_trajs);
  s.n_iter_trajs = from_problem(s.n_iter_trajs, b0, w.count);
  s.alpha_trace = from_problem(s.alpha_trace, b0, w.alpha_trace);
  return s;
}
inline cilqr_warm_start slice(cilqr_warm_start s, int b0, int n_knots) {
  const warm_widths w = widths(s, n_knots);
  s.rows = from_problem(s.rows, b0, w.rows);
  s.shift = from_problem(s.shift, b0, w.shift);
  return s;
}

// ---- HOST inputs on their way in, packed, the ints behind the doubles; an array that does not travel has no bytes
struct solve_in_layout {
  enum { kStart, kCoarse, kCorridor, kStation, kWarmRows, kCount, kWarmShift, kArrays };
  struct entry { const void* host; slot s; };
  entry a[kArrays];
  block_layout l{1};
  solve_in_layout(const cilqr_config& cfg, const cilqr_problem_batch& in, const cilqr_warm_start* warm) {
    const size_t B = (size_t)in.batch;
    const problem_widths w = widths(in);
    const warm_widths ww = warm ? widths(*warm, in.n_knots) : warm_widths{0, 0};
    const bool want_station = cfg.init_guess == CILQR_INIT_TRACKER && in.coarse_station != nullptr;
    a[kStart] = {in.start, l.add(B * w.start * 8)};
    a[kCoarse] = {in.coarse, l.add(B * w.coarse * 8)};
    a[kCorridor] = {in.corridor, l.add(B * w.corridor * 8)};
    a[kStation] = {in.coarse_station, l.add(want_station ? B * w.coarse_station * 8 : 0)};
    a[kWarmRows] = {warm ? warm->rows : nullptr, l.add(B * ww.rows * 8)};
    a[kCount] = {in.corridor_count, l.add(B * w.corridor_count * 4)};
    a[kWarmShift] = {warm ? warm->shift : nullptr, l.add(warm && warm->shift && ww.rows ? B * ww.shift * 4 : 0)};
  }
  size_t payload_bytes() const { return l.bytes(); }
  bool is_small() const { return payload_bytes() <= kSmallTransfer; }   // one pinned block, one copy (else: array by array)
};

// ---- HOST outputs on their way out, packed: the iterates last, so that a small batch can fetch everything else (and the
// first few iterates) in one short copy.  alpha_trace and iter_trajs have bytes only when the caller gave them.
struct solve_out_layout {
  solution_widths w{};
  slot traj, cost_hist, n_cost, status, n_iter, n_iter_trajs, alpha_trace, iter_trajs;
  bool on_host = false;
  solve_out_layout() = default;
  solve_out_layout(const cilqr_config& cfg, int batch, const cilqr_solution_batch& out)
      : w(widths(out, cfg.n_steps + 1, cfg.max_iter)), on_host(out.memory == CILQR_MEM_HOST) {
    const size_t B = (size_t)batch;
    block_layout l(1);
    traj = l.add(B * w.traj * 8);
    cost_hist = l.add(B * w.cost_hist * 8);
    for (slot* s : {&n_cost, &status, &n_iter, &n_iter_trajs}) *s = l.add(B * w.count * 4);
    alpha_trace = l.add(out.alpha_trace ? B * w.alpha_trace : 0);
    l.pad_to(8);
    iter_trajs = l.add(out.iter_trajs ? B * w.iter_trajs * 8 : 0);
  }
  size_t counts_bytes() const { return n_iter_trajs.off + n_iter_trajs.bytes - n_cost.off; }   // the four arrays, back to back
  size_t head_bytes() const { return iter_trajs.off; }   // everything in front of the iterates
  size_t total_bytes() const { return iter_trajs.off + iter_trajs.bytes; }
  bool is_big() const { return on_host && total_bytes() > kSmallTransfer; }   // above the pinned block: ragged (job_finish)
};

// Where the kernels of a solve write: `dev` is the caller's batch itself on DEVICE arrays, the slots of the staging `block`
// on HOST arrays, which is handed out on the host afterwards -- small (one pinned block) or large (ragged).
struct solve_outputs {
  enum where_t { kDevice, kSmallHost, kLargeHost } where = kDevice;
  solve_out_layout lay;
  cilqr_solution_batch dev{};
  solve_outputs() = default;
  solve_outputs(const solve_out_layout& l, const cilqr_solution_batch& out, void* block)
      : where(!l.on_host ? kDevice : l.is_big() ? kLargeHost : kSmallHost), lay(l), dev(out) {
    if (where == kDevice) return;
    dev.memory = CILQR_MEM_DEVICE;
    dev.traj = l.traj.in<double>(block);
    dev.cost_hist = l.cost_hist.in<double>(block);
    dev.n_cost = l.n_cost.in<int32_t>(block);
    dev.status = l.status.in<int32_t>(block);
    dev.n_iter = l.n_iter.in<int32_t>(block);
    dev.n_iter_trajs = l.n_iter_trajs.in<int32_t>(block);
    dev.alpha_trace = l.alpha_trace.bytes ? l.alpha_trace.in<int8_t>(block) : nullptr;
    dev.iter_trajs = l.iter_trajs.bytes ? l.iter_trajs.in<double>(block) : nullptr;
  }
};

// ---- the hand-out on the host.  Live rows of a problem: n_cost clamped to what the array holds.
inline size_t live_cost_rows(int32_t n_cost, int max_iter) { return (size_t)std::min(std::max(n_cost, 0), max_iter + 1); }

// The live Cost rows of every problem into the caller's dense cost_hist; nothing behind them is touched.  src_block: bytes
// from one problem's rows to the next at the source, 0 = packed (a problem's live rows follow those of the one before).
inline void scatter_cost_rows(double* cost_hist, const void* src, size_t src_block, const int32_t* n_cost, int batch, int max_iter) {
  const size_t row = CILQR_COST_FIELDS * 8, block = ((size_t)max_iter + 1) * row;
  const char* s = static_cast<const char*>(src);
  for (int b = 0; b < batch; ++b) {
    const size_t live = live_cost_rows(n_cost[b], max_iter) * row;
    std::memcpy(reinterpret_cast<char*>(cost_hist) + (size_t)b * block, s, live);
    s += src_block ? src_block : live;
  }
}

// n_cost | status | n_iter | n_iter_trajs, back to back at `counts`, and the alpha trace (NULL: it travels on its own)
inline void hand_out_counts(const cilqr_solution_batch& out, const solve_out_layout& l, const void* counts, const void* alpha) {
  const auto give = [&](int32_t* dst, const slot& s) { std::memcpy(dst, static_cast<const char*>(counts) + (s.off - l.n_cost.off), s.bytes); };
  give(out.n_cost, l.n_cost);
  give(out.status, l.status);
  if (out.n_iter) give(out.n_iter, l.n_iter);
  if (out.iter_trajs) give(out.n_iter_trajs, l.n_iter_trajs);
  if (out.alpha_trace && alpha) std::memcpy(out.alpha_trace, alpha, l.alpha_trace.bytes);
}

}  // namespace cilqr
