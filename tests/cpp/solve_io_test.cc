// Stand-alone host test of cilqr_amd/csrc/solve_io.hpp: the two staging layouts of a solve against byte counts worked out
// here from the array shapes of include/cilqr.h, problems [b0, b1) of a batch, and the hand-out of a block that has come
// back.  Built with -fsanitize=address,undefined and run as a child process by tests/test_solve_io.py: every array below
// is a heap block of exactly its size, so a width that is one too large reads or writes past its end.
// Prints "<n> checks, <f> failures"; the exit status is 0 only without failures.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "solve_io.hpp"

using namespace cilqr;

static int g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failures;                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

// rows per problem and doubles per row of the three warm layouts (include/cilqr.h: cilqr_warm_start)
static size_t warm_doubles(int layout, size_t K) {
  return layout == CILQR_ROWS_TRAJ ? K * 10 : layout == CILQR_ROWS_PLAN ? K * 11 : (K - 1) * 2;
}

// ------------------------------------------------------------------------------------------------------------------
// layouts
// ------------------------------------------------------------------------------------------------------------------
struct InCase { int B, K, cmax; bool tracker, station; int warm_layout /* -1: none */; bool shift; };

static void check_in_layout(const InCase& c, size_t payload_by_hand /* 0: not given */) {
  const size_t B = c.B, K = c.K;
  cilqr_config cfg{};
  cfg.n_steps = c.K - 1;
  cfg.init_guess = c.tracker ? CILQR_INIT_TRACKER : CILQR_INIT_IQR;
  // (the layout looks at pointers only to tell given from not given: one object serves for all)
  static double some_doubles[1];
  static int32_t some_ints[1];
  cilqr_problem_batch in{};
  in.batch = c.B; in.n_knots = c.K; in.cmax = c.cmax; in.memory = CILQR_MEM_HOST;
  in.start = some_doubles; in.coarse = some_doubles + 0; in.corridor = some_doubles; in.corridor_count = some_ints;
  in.coarse_station = c.station ? some_doubles : nullptr;
  cilqr_warm_start warm{};
  warm.memory = CILQR_MEM_HOST; warm.layout = c.warm_layout; warm.rows = some_doubles; warm.shift = c.shift ? some_ints : nullptr;
  const bool has_warm = c.warm_layout >= 0;
  // bytes of the seven arrays in the order they travel: [B][4], [B][K][6], [B][K][cmax][3] doubles, [B][K] stations (the
  // tracker init guess alone reads them), the warm rows, [B][K] int32 counts, [B] int32 shifts
  const size_t want[7] = {B * 4 * 8, B * K * 6 * 8, B * K * c.cmax * 3 * 8, (c.tracker && c.station) ? B * K * 8 : 0,
                          has_warm ? B * warm_doubles(c.warm_layout, K) * 8 : 0, B * K * 4, (has_warm && c.shift) ? B * 4 : 0};
  const void* src[7] = {in.start, in.coarse, in.corridor, in.coarse_station, has_warm ? warm.rows : nullptr, in.corridor_count,
                        has_warm ? warm.shift : nullptr};
  const solve_in_layout lay(cfg, in, has_warm ? &warm : nullptr);
  CHECK(solve_in_layout::kArrays == 7);
  size_t off = 0;
  for (int i = 0; i < 7; ++i) {
    CHECK(lay.a[i].s.bytes == want[i]);
    CHECK(lay.a[i].s.off == off);
    if (want[i]) CHECK(lay.a[i].host == src[i]);
    off += want[i];
  }
  CHECK(lay.payload_bytes() == off);
  if (payload_by_hand) CHECK(lay.payload_bytes() == payload_by_hand);
  CHECK(lay.is_small() == (off <= ((size_t)4 << 20)));
}

struct OutCase { int B, K, M, cap; bool iters, alpha, host; };

static void check_out_layout(const OutCase& c, size_t pad_by_hand, size_t head_by_hand, size_t total_by_hand) {
  const size_t B = c.B, K = c.K, M = c.M;
  cilqr_config cfg{};
  cfg.n_steps = c.K - 1; cfg.max_iter = c.M;
  std::vector<char> block(16);   // (its address alone is used)
  static double d[1];
  static int32_t n[1];
  static int8_t a8[1];
  cilqr_solution_batch out{};
  out.memory = c.host ? CILQR_MEM_HOST : CILQR_MEM_DEVICE;
  out.max_iter_trajs = c.cap;
  out.traj = d; out.cost_hist = d; out.n_cost = n; out.status = n; out.n_iter = n;
  out.iter_trajs = c.iters ? d : nullptr; out.n_iter_trajs = c.iters ? n : nullptr; out.alpha_trace = c.alpha ? a8 : nullptr;
  const solve_out_layout lay(cfg, c.B, out);
  // [B][K][10] and [B][M+1][5] doubles, four [B] int32 arrays, [B][M] int8, up to the next multiple of 8, [B][cap][K][10] doubles
  const size_t n_traj = B * K * 10 * 8, n_hist = B * (M + 1) * 5 * 8, n_alpha = c.alpha ? B * M : 0;
  const size_t unpadded = n_traj + n_hist + 4 * B * 4 + n_alpha, pad = (8 - unpadded % 8) % 8;
  const size_t n_iters = c.iters ? B * (size_t)c.cap * K * 10 * 8 : 0;
  CHECK(pad == pad_by_hand);
  CHECK(lay.traj.off == 0 && lay.traj.bytes == n_traj);
  CHECK(lay.cost_hist.off == n_traj && lay.cost_hist.bytes == n_hist);
  CHECK(lay.n_cost.off == n_traj + n_hist && lay.n_cost.bytes == B * 4);
  CHECK(lay.status.off == n_traj + n_hist + B * 4 && lay.status.bytes == B * 4);
  CHECK(lay.n_iter.off == n_traj + n_hist + 2 * B * 4 && lay.n_iter.bytes == B * 4);
  CHECK(lay.n_iter_trajs.off == n_traj + n_hist + 3 * B * 4 && lay.n_iter_trajs.bytes == B * 4);
  CHECK(lay.alpha_trace.off == n_traj + n_hist + 4 * B * 4 && lay.alpha_trace.bytes == n_alpha);
  CHECK(lay.iter_trajs.off == unpadded + pad && lay.iter_trajs.bytes == n_iters);
  CHECK(lay.counts_bytes() == 4 * B * 4);
  CHECK(lay.head_bytes() == unpadded + pad && lay.head_bytes() == head_by_hand);
  CHECK(lay.total_bytes() == unpadded + pad + n_iters && lay.total_bytes() == total_by_hand);
  CHECK(lay.is_big() == (c.host && total_by_hand > ((size_t)4 << 20)));
  // the pointers the kernels get: the block's slots on HOST arrays, the caller's own on DEVICE arrays
  const solve_outputs res(lay, out, block.data());
  const cilqr_solution_batch& r = res.dev;
  char* p = block.data();
  if (c.host) {
    CHECK(res.where == (lay.is_big() ? solve_outputs::kLargeHost : solve_outputs::kSmallHost));
    CHECK(r.memory == CILQR_MEM_DEVICE && r.max_iter_trajs == c.cap);
    CHECK((char*)r.traj == p && (char*)r.cost_hist == p + n_traj && (char*)r.n_cost == p + n_traj + n_hist);
    CHECK((char*)r.status == (char*)r.n_cost + B * 4 && (char*)r.n_iter == (char*)r.n_cost + 2 * B * 4);
    CHECK((char*)r.n_iter_trajs == (char*)r.n_cost + 3 * B * 4);
    CHECK(c.alpha ? (char*)r.alpha_trace == (char*)r.n_cost + 4 * B * 4 : r.alpha_trace == nullptr);
    CHECK(c.iters ? (char*)r.iter_trajs == p + head_by_hand : r.iter_trajs == nullptr);
  } else {
    CHECK(res.where == solve_outputs::kDevice);
    CHECK(r.traj == out.traj && r.cost_hist == out.cost_hist && r.n_cost == out.n_cost && r.status == out.status);
    CHECK(r.n_iter == out.n_iter && r.n_iter_trajs == out.n_iter_trajs && r.iter_trajs == out.iter_trajs);
    CHECK(r.alpha_trace == out.alpha_trace && r.memory == CILQR_MEM_DEVICE && r.max_iter_trajs == c.cap);
  }
}

static void test_layouts() {
  // B = 1, K = 51, cmax = 16: 32 + 2448 + 19584 doubles' bytes, 204 of counts
  check_in_layout({1, 51, 16, false, false, -1, false}, 22268);
  check_in_layout({1, 51, 16, false, true, -1, false}, 22268);            // a station column the IQR init guess does not read
  check_in_layout({1, 51, 16, true, true, -1, false}, 22268 + 408);
  check_in_layout({1, 51, 16, true, false, -1, false}, 22268);
  check_in_layout({1, 51, 16, false, false, CILQR_ROWS_TRAJ, false}, 22268 + 4080);
  check_in_layout({1, 51, 16, false, false, CILQR_ROWS_TRAJ, true}, 22268 + 4080 + 4);
  check_in_layout({1, 51, 16, false, false, CILQR_ROWS_PLAN, false}, 22268 + 4488);
  check_in_layout({1, 51, 16, false, false, CILQR_ROWS_PLAN, true}, 22268 + 4488 + 4);
  check_in_layout({1, 51, 16, false, false, CILQR_ROWS_CONTROLS, false}, 22268 + 800);
  check_in_layout({1, 51, 16, true, true, CILQR_ROWS_CONTROLS, true}, 22268 + 408 + 800 + 4);
  // odd B and K: the counts end at an odd multiple of 4, and the shifts follow them there
  check_in_layout({3, 7, 5, true, true, CILQR_ROWS_PLAN, true}, 3 * (32 + 336 + 840 + 56 + 616 + 28 + 4));
  // either side of the 4 MiB block: 188 * 22268 = 4186384 <= 4194304 < 189 * 22268 = 4208652
  check_in_layout({188, 51, 16, false, false, -1, false}, 4186384);
  check_in_layout({189, 51, 16, false, false, -1, false}, 4208652);
  {
    cilqr_config cfg{};
    cfg.n_steps = 50;
    cilqr_problem_batch in{};
    static double d[1];
    static int32_t n[1];
    in.n_knots = 51; in.cmax = 16; in.memory = CILQR_MEM_HOST; in.start = d; in.coarse = d; in.corridor = d; in.corridor_count = n;
    in.batch = 188;
    CHECK(solve_in_layout(cfg, in, nullptr).is_small());
    in.batch = 189;
    CHECK(!solve_in_layout(cfg, in, nullptr).is_small());
  }

  // B = 1, K = 51, M = 200: 4080 + 8040 + 16 (+ 200 of alpha trace), no pad; 201 iterates of 4080 bytes
  check_out_layout({1, 51, 200, 201, true, true, true}, 0, 12336, 12336 + 820080);
  check_out_layout({1, 51, 200, 201, false, true, true}, 0, 12336, 12336);
  check_out_layout({1, 51, 200, 201, true, false, true}, 0, 12136, 12136 + 820080);
  check_out_layout({1, 51, 200, 0, false, false, true}, 0, 12136, 12136);
  check_out_layout({1, 51, 200, 201, true, true, false}, 0, 12336, 12336 + 820080);   // DEVICE arrays: never "big"
  // odd B and M: 3 * 7 = 21 bytes of alpha trace behind 48 of counts -> 3 bytes of pad
  check_out_layout({3, 7, 7, 2, true, true, true}, 3, 1680 + 960 + 48 + 21 + 3, 2712 + 3360);
  check_out_layout({3, 7, 7, 2, false, true, true}, 3, 2712, 2712);
  check_out_layout({3, 7, 7, 2, true, false, true}, 0, 2688, 2688 + 3360);
  check_out_layout({5, 4, 3, 1, true, true, true}, 1, 1600 + 800 + 80 + 15 + 1, 2496 + 1600);
  // 64 problems with 48 iterates each: 12.5 MB behind a head of 261120 + 514560 + 1024 + 12800 -> large
  check_out_layout({64, 51, 200, 48, true, true, true}, 0, 789504, 789504 + 12533760);
  check_out_layout({64, 51, 200, 48, true, true, false}, 0, 789504, 789504 + 12533760);
}

// ------------------------------------------------------------------------------------------------------------------
// slices: element i of problem b of array `id` holds id * 1e6 + b * 1e3 + i
// ------------------------------------------------------------------------------------------------------------------
template <class T>
static T code(int id, int b, size_t i) { return (T)(id * 1000000 + b * 1000 + (int)i); }
template <>
int8_t code<int8_t>(int id, int b, size_t i) { return (int8_t)((id + b * 11 + (int)i) % 100); }

template <class T>
static std::vector<T> filled(int id, int B, size_t width) {
  std::vector<T> v((size_t)B * width);
  for (int b = 0; b < B; ++b)
    for (size_t i = 0; i < width; ++i) v[(size_t)b * width + i] = code<T>(id, b, i);
  return v;
}
// first and last element of problems [b0, b1) of array `id`
template <class T>
static void check_range(const T* s, int id, int b0, int b1, size_t width) {
  CHECK(s != nullptr);
  if (s == nullptr) return;
  CHECK(s[0] == code<T>(id, b0, 0));
  CHECK(s[(size_t)(b1 - b0) * width - 1] == code<T>(id, b1 - 1, width - 1));
}

static void test_slices() {
  const int B = 5, K = 4, cmax = 3, M = 3, cap = 2;
  const auto start = filled<double>(1, B, 4), coarse = filled<double>(2, B, K * 6), cor = filled<double>(3, B, K * cmax * 3);
  const auto station = filled<double>(4, B, K);
  const auto ccount = filled<int32_t>(5, B, K);
  auto traj = filled<double>(6, B, K * 10), hist = filled<double>(7, B, (M + 1) * 5), iters = filled<double>(8, B, cap * K * 10);
  auto n_cost = filled<int32_t>(9, B, 1), status = filled<int32_t>(10, B, 1), n_iter = filled<int32_t>(11, B, 1);
  auto n_its = filled<int32_t>(12, B, 1);
  auto alpha = filled<int8_t>(13, B, M);
  const auto shift = filled<int32_t>(14, B, 1);
  const int ranges[][2] = {{0, 5}, {0, 1}, {4, 5}, {2, 3}, {1, 4}, {0, 4}, {1, 5}};
  for (const auto& r : ranges) {
    const int b0 = r[0], b1 = r[1];
    for (int nulls = 0; nulls < 2; ++nulls) {   // every optional array given, then none of them
      cilqr_problem_batch in{};
      in.batch = B; in.n_knots = K; in.cmax = cmax; in.memory = CILQR_MEM_HOST; in.n_left = 3; in.n_right = 2;
      in.start = start.data(); in.coarse = coarse.data(); in.corridor = cor.data(); in.corridor_count = ccount.data();
      in.coarse_station = nulls ? nullptr : station.data();
      const cilqr_problem_batch s = slice(in, b0, b1);
      CHECK(s.batch == b1 - b0 && s.n_knots == K && s.cmax == cmax && s.memory == CILQR_MEM_HOST && s.n_left == 3 && s.n_right == 2);
      check_range(s.start, 1, b0, b1, 4);
      check_range(s.coarse, 2, b0, b1, K * 6);
      check_range(s.corridor, 3, b0, b1, K * cmax * 3);
      check_range(s.corridor_count, 5, b0, b1, K);
      if (nulls) CHECK(s.coarse_station == nullptr);
      else check_range(s.coarse_station, 4, b0, b1, K);

      cilqr_solution_batch out{};
      out.memory = CILQR_MEM_HOST; out.max_iter_trajs = cap;
      out.traj = traj.data(); out.cost_hist = hist.data(); out.n_cost = n_cost.data(); out.status = status.data();
      out.n_iter = nulls ? nullptr : n_iter.data();
      out.iter_trajs = nulls ? nullptr : iters.data();
      out.n_iter_trajs = nulls ? nullptr : n_its.data();
      out.alpha_trace = nulls ? nullptr : alpha.data();
      const cilqr_solution_batch o = slice(out, b0, b1, K, M);
      CHECK(o.memory == CILQR_MEM_HOST && o.max_iter_trajs == cap);
      check_range(o.traj, 6, b0, b1, K * 10);
      check_range(o.cost_hist, 7, b0, b1, (M + 1) * 5);
      check_range(o.n_cost, 9, b0, b1, 1);
      check_range(o.status, 10, b0, b1, 1);
      if (nulls) {
        CHECK(o.n_iter == nullptr && o.iter_trajs == nullptr && o.n_iter_trajs == nullptr && o.alpha_trace == nullptr);
      } else {
        check_range(o.n_iter, 11, b0, b1, 1);
        check_range(o.iter_trajs, 8, b0, b1, cap * K * 10);
        check_range(o.n_iter_trajs, 12, b0, b1, 1);
        check_range(o.alpha_trace, 13, b0, b1, M);
      }

      for (int layout : {CILQR_ROWS_TRAJ, CILQR_ROWS_PLAN, CILQR_ROWS_CONTROLS}) {
        const size_t width = warm_doubles(layout, K);
        const auto rows = filled<double>(15 + layout, B, width);
        cilqr_warm_start warm{};
        warm.memory = CILQR_MEM_HOST; warm.layout = layout; warm.rows = rows.data(); warm.shift = nulls ? nullptr : shift.data();
        const cilqr_warm_start w = slice(warm, b0, K);
        CHECK(w.memory == CILQR_MEM_HOST && w.layout == layout);
        check_range(w.rows, 15 + layout, b0, b1, width);
        if (nulls) CHECK(w.shift == nullptr);
        else check_range(w.shift, 14, b0, b1, 1);
      }
    }
  }
  // a batch whose required arrays are missing too: nothing is invented
  cilqr_problem_batch none{};
  none.batch = B; none.n_knots = K; none.cmax = cmax;
  const cilqr_problem_batch s = slice(none, 2, 4);
  CHECK(s.start == nullptr && s.coarse == nullptr && s.corridor == nullptr && s.corridor_count == nullptr && s.coarse_station == nullptr);
  cilqr_solution_batch no_out{};
  const cilqr_solution_batch o = slice(no_out, 2, 4, K, M);
  CHECK(o.traj == nullptr && o.cost_hist == nullptr && o.n_cost == nullptr && o.status == nullptr);
  cilqr_warm_start no_warm{};
  no_warm.layout = CILQR_ROWS_TRAJ;
  CHECK(slice(no_warm, 2, K).rows == nullptr && slice(no_warm, 2, K).shift == nullptr);
}

// ------------------------------------------------------------------------------------------------------------------
// the hand-out
// ------------------------------------------------------------------------------------------------------------------
static void test_hand_out() {
  const int B = 5, M = 4, rows_cap = M + 1;
  const double kUntouched = -777.0;
  const int32_t n_cost[B] = {0, 1, M + 1, -3, M + 6};   // the last two are clamped: none, all
  const size_t live[B] = {0, 1, 5, 0, 5};
  for (int b = 0; b < B; ++b) CHECK(live_cost_rows(n_cost[b], M) == live[b]);
  const auto dense = filled<double>(1, B, rows_cap * 5);
  std::vector<double> packed;   // the live rows back to back, and not a byte more
  for (int b = 0; b < B; ++b)
    packed.insert(packed.end(), dense.begin() + (size_t)b * rows_cap * 5, dense.begin() + (size_t)b * rows_cap * 5 + live[b] * 5);
  CHECK(packed.size() == 11 * 5);
  for (int from_packed = 0; from_packed < 2; ++from_packed) {
    std::vector<double> dst((size_t)B * rows_cap * 5, kUntouched);
    if (from_packed) scatter_cost_rows(dst.data(), packed.data(), 0, n_cost, B, M);
    else scatter_cost_rows(dst.data(), dense.data(), (size_t)rows_cap * 5 * 8, n_cost, B, M);
    for (int b = 0; b < B; ++b)
      for (size_t i = 0; i < (size_t)rows_cap * 5; ++i) {
        const double got = dst[(size_t)b * rows_cap * 5 + i];
        CHECK(got == (i < live[b] * 5 ? code<double>(1, b, i) : kUntouched));
      }
  }

  // the four count arrays and the alpha trace, as they lie in the block: with and without the optional arrays
  cilqr_config cfg{};
  cfg.n_steps = 3; cfg.max_iter = M;
  const auto counts = filled<int32_t>(2, 4, B);   // "problem" q of this array = count array q
  const auto alpha = filled<int8_t>(3, B, M);
  for (int optional = 0; optional < 2; ++optional)
    for (int alpha_with_counts = 0; alpha_with_counts < 2; ++alpha_with_counts) {
      std::vector<int32_t> nc(B, -5), st(B, -5), ni(B, -5), nit(B, -5);
      std::vector<int8_t> at((size_t)B * M, -5);
      std::vector<double> its(1);
      cilqr_solution_batch out{};
      out.memory = CILQR_MEM_HOST; out.max_iter_trajs = 1;
      out.n_cost = nc.data(); out.status = st.data();
      out.n_iter = optional ? ni.data() : nullptr;
      out.iter_trajs = optional ? its.data() : nullptr;
      out.n_iter_trajs = nit.data();   // (given, but only read back together with iter_trajs)
      out.alpha_trace = optional ? at.data() : nullptr;
      const solve_out_layout lay(cfg, B, out);
      hand_out_counts(out, lay, counts.data(), alpha_with_counts ? alpha.data() : nullptr);
      for (int b = 0; b < B; ++b) {
        CHECK(nc[b] == code<int32_t>(2, 0, b) && st[b] == code<int32_t>(2, 1, b));
        CHECK(ni[b] == (optional ? code<int32_t>(2, 2, b) : -5));
        CHECK(nit[b] == (optional ? code<int32_t>(2, 3, b) : -5));
        for (int i = 0; i < M; ++i) CHECK(at[(size_t)b * M + i] == (optional && alpha_with_counts ? code<int8_t>(3, b, i) : -5));
      }
    }
}

int main() {
  test_layouts();
  test_slices();
  test_hand_out();
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
