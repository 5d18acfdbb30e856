// Stand-alone host test of include/cilqr/row_math.hpp, the one statement of the arithmetic that the host statements and
// the kernels share: NormalizeAngle, slerp, the bracket, hypot_ref and the pair step.  Both sides run these very functions,
// so a wrong one agrees with itself: here every rule is written out a second time, in its plain form -- fmod for the angle,
// std::lower_bound for the bracket, sqrtl for the hypotenuse, the rule of include/cilqr.h ("resample") with the column
// numbers as literals for the pair step.  Built with g++ alone (-fsanitize=address,undefined) and run as a child process by
// tests/test_row_math.py.  Prints "<n> checks, <f> failures"; the exit status is 0 only without failures.
#include "cilqr/row_math.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "cilqr/trajectory_queries.hpp"

using namespace cilqr;
namespace tq = cilqr::trajectory_queries;

static int g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failures;                                                        \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}
static double of_bits(uint64_t b) {
  double v;
  std::memcpy(&v, &b, sizeof(v));
  return v;
}
static bool same(double a, double b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }
static const double kInf = std::numeric_limits<double>::infinity();
static const double kNan = std::numeric_limits<double>::quiet_NaN();

// ---- the plain forms
static double plain_normalize(double angle) {   // math_utils.cpp:53-59
  double a = std::fmod(angle + M_PI, 2.0 * M_PI);
  if (a < 0.0) a += 2.0 * M_PI;
  return a - M_PI;
}
static double plain_slerp(double a0, double t0, double a1, double t1, double t) {   // math_utils.h:208-225
  if (std::fabs(t1 - t0) <= 1e-10) return plain_normalize(a0);
  const double a0_n = plain_normalize(a0), a1_n = plain_normalize(a1);
  double d = a1_n - a0_n;
  if (d > M_PI) d = d - 2 * M_PI;
  else if (d < -M_PI) d = d + 2 * M_PI;
  const double r = (t - t0) / (t1 - t0);
  return plain_normalize(a0_n + d * r);
}

static void check_normalize_angle() {
  // the boundaries of the short paths, t = angle + pi at 0, 2 pi, 4 pi, -2 pi: the angle that lands there and its
  // neighbours, one representable value after the other on either side
  const double at[4] = {-M_PI, M_PI, 3.0 * M_PI, -3.0 * M_PI};
  const double edge[4] = {0.0, 2.0 * M_PI, 4.0 * M_PI, -2.0 * M_PI};
  for (int b = 0; b < 4; ++b) {
    bool below = false, on = false, above = false;
    double lo = at[b], hi = at[b];
    for (int step = 0; step <= 8; ++step) {
      for (double a : {lo, hi}) {
        CHECK(same(normalize_angle(a), plain_normalize(a)));
        const double t = a + M_PI;
        below = below || t < edge[b];
        on = on || t == edge[b];
        above = above || t > edge[b];
      }
      lo = std::nextafter(lo, -kInf);
      hi = std::nextafter(hi, kInf);
    }
    CHECK(below && on && above);
  }
  for (double a : {M_PI, 3.0 * M_PI, 1e5, 1e300, 0.0, 7.5 * M_PI, 9.25 * M_PI, 1.0, 6.0, 12.0, 13.0}) {
    CHECK(same(normalize_angle(a), plain_normalize(a)));
    CHECK(same(normalize_angle(-a), plain_normalize(-a)));
  }
  CHECK(bits(normalize_angle(0.0)) == bits(0.0) && bits(normalize_angle(-0.0)) == bits(0.0));
  CHECK(normalize_angle(M_PI) == -M_PI && normalize_angle(-M_PI) == -M_PI);
  CHECK(std::isnan(normalize_angle(kInf)) && std::isnan(plain_normalize(kInf)));
  CHECK(std::isnan(normalize_angle(-kInf)) && std::isnan(plain_normalize(-kInf)));
  CHECK(std::isnan(normalize_angle(kNan)) && std::isnan(plain_normalize(kNan)));
  uint64_t seed = 12345;
  for (int i = 0; i < 20000; ++i) {   // a seeded sweep over (-40, 40): every path, the library call included
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    const double a = ((double)(seed >> 11) / 9007199254740992.0 - 0.5) * 80.0;
    CHECK(same(normalize_angle(a), plain_normalize(a)));
  }
  CHECK(kMathEps == 1e-10 && bits(kPi) == bits(M_PI) && bits(kTwoPi) == bits(2.0 * M_PI));
}

static void check_slerp() {
  const double above = std::nextafter(1e-10, 1.0);
  // |t1 - t0| below, exactly at and above 1e-10: `<=`, so exactly at is degenerate -- the heading of p0, wrapped
  for (double t0 : {0.0, -1e-10}) {
    for (double dt : {0.0, 0.5e-10, 1e-10}) {
      for (double sign : {1.0, -1.0}) {
        const double t1 = t0 + sign * dt;
        if (std::fabs(t1 - t0) > 1e-10) continue;   // (t0 + dt - t0 can round above)
        CHECK(same(slerp(7.5 * M_PI, t0, 1.0, t1, t1), plain_normalize(7.5 * M_PI)));
      }
    }
  }
  CHECK(std::fabs(1e-10 - 0.0) <= 1e-10 && !(std::fabs(above - 0.0) <= 1e-10));
  CHECK(same(slerp(0.25, 0.0, 1.0, 1e-10, 1e-10), plain_normalize(0.25)));
  CHECK(same(slerp(0.25, 0.0, 1.0, above, above), plain_slerp(0.25, 0.0, 1.0, above, above)));
  CHECK(std::fabs(slerp(0.25, 0.0, 1.0, above, above) - 1.0) < 1e-12);
  // across the +-pi wrap, both directions: the short way round, and a result back in [-pi, pi)
  for (double t : {-0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5}) {
    const double fwd = slerp(3.0, 0.0, -3.0, 1.0, t), back = slerp(-3.0, 0.0, 3.0, 1.0, t);
    CHECK(same(fwd, plain_slerp(3.0, 0.0, -3.0, 1.0, t)) && same(back, plain_slerp(-3.0, 0.0, 3.0, 1.0, t)));
    CHECK(fwd >= -M_PI && fwd < M_PI && back >= -M_PI && back < M_PI);
    if (t >= 0.0 && t <= 1.0) CHECK(std::fabs(fwd) >= 3.0 - 1e-12 && std::fabs(back) >= 3.0 - 1e-12);
  }
  CHECK(slerp(3.0, 0.0, -3.0, 1.0, 0.25) > 3.0 && slerp(3.0, 0.0, -3.0, 1.0, 0.75) < -3.0);
  CHECK(slerp(-3.0, 0.0, 3.0, 1.0, 0.25) < -3.0 && slerp(-3.0, 0.0, 3.0, 1.0, 0.75) > 3.0);
  // headings far outside [-pi, pi)
  for (double t : {0.0, 0.3, 1.0, 2.0})
    CHECK(same(slerp(7.5 * M_PI, 1.0, -9.25 * M_PI, 3.0, t), plain_slerp(7.5 * M_PI, 1.0, -9.25 * M_PI, 3.0, t)));
}

// ---- the bracket
static int halving(const std::vector<double>& key, double q) {   // std::lower_bound's loop, for keys in any order
  int first = 0, len = (int)key.size();
  while (len > 0) {
    const int half = len >> 1;
    if (key[first + half] < q) {
      first += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return first;
}
static void check_bracket_on(const std::vector<double>& key, const std::vector<double>& queries, bool sorted) {
  const int n = (int)key.size();
  for (double q : queries) {
    int want;
    if (q >= key[n - 1]) want = n - 1;
    else if (q < key[0]) want = 0;
    else want = sorted ? (int)(std::lower_bound(key.begin(), key.end(), q) - key.begin()) : halving(key, q);
    const int got = bracket(n, q, [&](int i) { return key[i]; });
    const int pair = bracket_pair(n, q, [&](int i) { return key[i]; });
    CHECK(got == want);
    CHECK(pair == (want == 0 ? 1 : want > n - 1 ? n - 1 : want) && pair >= 1 && pair <= n - 1);
    const int rows1 = tq::bracket(key.data(), 1, 0, n, q);
    CHECK(rows1 == pair);
  }
}
static void check_bracket() {
  for (int n : {2, 3, 256}) {
    std::vector<double> key(n), queries;
    for (int i = 0; i < n; ++i) key[i] = 0.5 * (i / 2) - 3.0;   // sorted, every key twice (but for an odd last one)
    for (int i = 0; i < n; ++i) {
      queries.push_back(key[i]);
      queries.push_back(std::nextafter(key[i], -kInf));
      queries.push_back(std::nextafter(key[i], kInf));
      queries.push_back(key[i] + 0.25);
    }
    for (double q : {-1e9, -3.5, key[n - 1] + 1e9, -kInf, kInf}) queries.push_back(q);
    check_bracket_on(key, queries, true);
    for (int i = 0; i < n; ++i) key[i] = 0.125 * i;   // strictly increasing
    check_bracket_on(key, queries, true);
    // the end rules: below the first key row 0 (the pair: row 1), at or above the last key row n - 1
    CHECK(bracket(n, -1.0, [&](int i) { return key[i]; }) == 0 && bracket_pair(n, -1.0, [&](int i) { return key[i]; }) == 1);
    CHECK(bracket(n, key[n - 1], [&](int i) { return key[i]; }) == n - 1);
    CHECK(bracket(n, key[0], [&](int i) { return key[i]; }) == 0 && bracket_pair(n, key[0], [&](int i) { return key[i]; }) == 1);
    // unsorted and NaN keys, a NaN query: the halving written out, and a pair inside the rows whatever comes
    uint64_t seed = 99 + n;
    for (int i = 0; i < n; ++i) {
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      key[i] = (seed >> 60) == 0 ? kNan : (double)((seed >> 33) % 64) * 0.125;
    }
    queries.push_back(kNan);
    check_bracket_on(key, queries, false);
    key[0] = kNan;
    key[n - 1] = kNan;
    check_bracket_on(key, queries, false);
  }
}

static void check_hypot_ref() {
  for (int e = -60; e <= 60; ++e) {   // representable triples: exact
    const double s = std::ldexp(1.0, e);
    CHECK(hypot_ref(3.0 * s, 4.0 * s) == 5.0 * s && hypot_ref(-4.0 * s, 3.0 * s) == 5.0 * s);
    CHECK(hypot_ref(5.0 * s, -12.0 * s) == 13.0 * s && hypot_ref(s, 0.0) == s && hypot_ref(0.0, -s) == s);
  }
  CHECK(bits(hypot_ref(0.0, 0.0)) == bits(0.0));
  // beyond the 2^54 ratio: ax + ay
  CHECK(same(hypot_ref(0x1p54, 1.0), 0x1p54 + 1.0) && same(hypot_ref(1.0, -0x1p54), 0x1p54 + 1.0));
  CHECK(same(hypot_ref(3.0, std::ldexp(1.0, -53)), 3.0 + std::ldexp(1.0, -53)) && same(hypot_ref(std::ldexp(1.0, -60), 7.0), 7.0 + std::ldexp(1.0, -60)));
  CHECK(same(hypot_ref(0x1.8p54, 1.5), 0x1.8p54 + 1.5));
  // lengths in metres: within one ulp of the long-double square root
  uint64_t seed = 2024;
  int worst = 0;
  for (int i = 0; i < 20000; ++i) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    const double x = std::ldexp((double)(seed >> 11) / 9007199254740992.0 - 0.5, (int)(seed % 21) - 10);
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    const double y = std::ldexp((double)(seed >> 11) / 9007199254740992.0 - 0.5, (int)(seed % 21) - 10);
    if (x == 0.0 && y == 0.0) continue;
    const double want = (double)sqrtl((long double)x * x + (long double)y * y), got = hypot_ref(x, y);
    const int64_t off = (int64_t)bits(got) - (int64_t)bits(want);
    worst = std::max(worst, (int)(off < 0 ? -off : off));
  }
  CHECK(worst <= 1);
}

// ---- the pair step.  The layouts as include/cilqr.h documents them: fields, time, station, theta, first control (-1: none)
static const int kLayout[3][5] = {{10, 0, -1, 3, 8}, {11, 0, 1, 4, 9}, {9, 0, 1, 4, -1}};
static void plain_row(int layout, int kc, const double* p0, const double* p1, double q, double* out) {
  const int F = kLayout[layout][0], theta = kLayout[layout][3], ctrl = kLayout[layout][4];
  const double k0 = p0[kc], k1 = p1[kc];
  if (std::fabs(k1 - k0) < 1e-10) {
    std::memcpy(out, p0, sizeof(double) * F);
    return;
  }
  const double w = (q - k0) / (k1 - k0);
  for (int f = 0; f < F; ++f) {
    if (f == kc) out[f] = q;
    else if (f == theta) out[f] = plain_slerp(p0[f], k0, p1[f], k1, q);
    else if (ctrl >= 0 && f >= ctrl) std::memcpy(out + f, p0 + f, sizeof(double));
    else out[f] = (1 - w) * p0[f] + w * p1[f];
  }
}

static void check_pair_step() {
  const double held = of_bits(0x7ff8000000000123ull);   // a NaN with a payload: a held column carries bits
  const int carry_from[3][7] = {{1, 2, 3, 7, 4, 5, 6}, {2, 3, 4, 5, 6, 7, 8}, {2, 3, 4, 5, 6, 7, 8}};   // x y theta kappa v a delta
  const int stop_from[3][5] = {{1, 2, 3, 7, 6}, {2, 3, 4, 5, 8}, {2, 3, 4, 5, 8}};                     // x y theta kappa delta
  const int stop_to[5] = {2, 3, 4, 5, 8};                                                              // ... of a plan row
  const double theta_pair[3][2] = {{0.5, 0.75}, {7.5 * M_PI, -9.25 * M_PI}, {3.0, -3.0}};
  for (int layout = 0; layout < 3; ++layout) {
    const int F = kLayout[layout][0], th = kLayout[layout][3], ctrl = kLayout[layout][4];
    for (int key = 0; key < 2; ++key) {
      const int kc = kLayout[layout][1 + key];
      if (kc < 0) {
        CHECK(tq::key_column(layout, key) == -1);
        continue;
      }
      CHECK(tq::key_column(layout, key) == kc);
      for (int tp = 0; tp < 3; ++tp) {
        // gap: an ordinary pair, one exactly 1e-10 apart (NOT degenerate here, degenerate in slerp), a degenerate one, equal keys
        for (double gap : {2.0, 1e-10, 0.5e-10, 0.0}) {
          double rows[2 * 11];
          for (int f = 0; f < F; ++f) {
            rows[f] = 0.375 * f - 1.0;
            rows[F + f] = 1.0 / (f + 3.0) + f;
          }
          rows[th] = theta_pair[tp][0];
          rows[F + th] = theta_pair[tp][1];
          rows[kc] = 0.0;
          rows[F + kc] = gap;
          if (ctrl >= 0) rows[ctrl + 1] = held;
          const bool degenerate = gap < 1e-10;
          for (double q : {0.0, gap, 0.5 * gap, 0.3, -1.5, gap + 0.7, 4.0}) {   // on a key, inside, before the first, beyond the last
            double want[11], got[11], all[11];
            plain_row(layout, kc, rows, rows + F, q, want);
            tq::resample_rows(layout, rows, 2, key, &q, 1, got);   // K = 2: the bracket gives the one pair
            pair_step(pair_all(tq::columns_of(layout)), kc, rows[kc], rows[F + kc], q, rows, rows + F, all);
            for (int f = 0; f < F; ++f) CHECK(bits(got[f]) == bits(want[f]) && bits(all[f]) == bits(want[f]));
            if (degenerate) {
              for (int f = 0; f < F; ++f) CHECK(bits(got[f]) == bits(rows[f]));   // p0's bits, the key column included
            } else {
              CHECK(bits(got[kc]) == bits(q));
              if (ctrl >= 0) CHECK(bits(got[ctrl]) == bits(rows[ctrl]) && bits(got[ctrl + 1]) == bits(held));
            }
            if (gap == 1e-10) {   // interpolated, with the heading of p0: at q = k1 everything else is p1's
              CHECK(same(got[th], plain_normalize(rows[th])));
              if (q == gap) CHECK(got[th == 3 ? 1 : 2] == rows[F + (th == 3 ? 1 : 2)]);
            }
            // the instances against the same values picked from the all-columns row
            double seven[7], five[11] = {0}, ctr[7], ctr_tq[7];
            pair_step(tq::pair_carry(tq::columns_of(layout)), kc, rows[kc], rows[F + kc], q, rows, rows + F, seven);
            for (int e = 0; e < 7; ++e) CHECK(bits(seven[e]) == bits(want[carry_from[layout][e]]));
            pair_step(tq::pair_stop(tq::columns_of(layout), row_columns(1)), -1, rows[kc], rows[F + kc], q, rows, rows + F, five);
            for (int e = 0; e < 5; ++e) CHECK(bits(five[stop_to[e]]) == bits(want[stop_from[layout][e]]));
            for (int f : {0, 1, 6, 7, 9, 10}) CHECK(bits(five[f]) == bits(0.0));   // nothing else is written
            if (layout == 2 && key == 1) {   // a centre row s x y theta kappa left right: columns 1 ... 7 of a coarse row keyed by s
              pair_step(pair_center(), 0, rows[1], rows[F + 1], q, rows + 1, rows + F + 1, ctr);
              tq::interpolate_center(rows + 1, rows + F + 1, q, ctr_tq);
              for (int e = 0; e < 7; ++e) CHECK(bits(ctr[e]) == bits(want[1 + e]) && bits(ctr_tq[e]) == bits(want[1 + e]));
            }
          }
        }
      }
    }
  }
  // the lists themselves, as literals
  const PairColumns c = pair_center();
  CHECK(c.n == 7);
  for (int e = 0; e < 7; ++e) CHECK(c.from[e] == e && c.to[e] == e && c.kind[e] == (e == 0 ? kPairKey : e == 3 ? kPairSlerp : kPairLerp));
  for (int layout = 0; layout < 3; ++layout) {
    const PairColumns a = pair_all(row_columns(layout));
    CHECK(a.n == kLayout[layout][0]);
    for (int f = 0; f < a.n; ++f) {
      const int ctrl = kLayout[layout][4];
      const int want = (f == kLayout[layout][1] || f == kLayout[layout][2]) ? kPairKey : f == kLayout[layout][3] ? kPairSlerp
                       : (ctrl >= 0 && f >= ctrl) ? kPairHold : kPairLerp;
      CHECK(a.from[f] == f && a.to[f] == f && a.kind[f] == want);
    }
  }
}

int main() {
  check_normalize_angle();
  check_slerp();
  check_bracket();
  check_hypot_ref();
  check_pair_step();
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
