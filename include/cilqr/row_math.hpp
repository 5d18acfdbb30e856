// include/cilqr/row_math.hpp -- the arithmetic every query on rows shares (include/cilqr.h, "resample"), stated ONCE for
// host and device: the geometry epsilon, NormalizeAngle, slerp, the bracket of a key, hypot as the reference's libm
// evaluates it, and the pair step of EvaluateTime / EvaluateStation.  The host statements (trajectory_queries.hpp,
// dp_planner.hpp, tracker.hpp, constraint_margins.hpp) and the kernels of cilqr_amd/csrc call these very functions, so
// the two sides cannot drift apart; what holds them to an independent statement is tests/cpp/row_math_test.cc, the
// NumPy statements of cilqr_amd/ and the device-math cases ("row layouts").
// C++14, header-only, no HIP header.  Every product and sum is meant to be rounded once: build with -ffp-contract=off.
#ifndef CILQR_ROW_MATH_HPP_
#define CILQR_ROW_MATH_HPP_

#include <math.h>

#include "row_layouts.hpp"

// what marks a function of this file: both sides under hipcc, and inlined into every kernel as __forceinline__ would
#if defined(__HIPCC__)
#define CILQR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CILQR_HD inline
#endif
// (in device code the loops over a column list are asked to unroll; a host compiler is left to itself)
#if defined(__HIP_DEVICE_COMPILE__)
#define CILQR_HD_UNROLL _Pragma("unroll")
#else
#define CILQR_HD_UNROLL
#endif

namespace cilqr {

constexpr double kMathEps = 1e-10;   // math::kMathEpsilon, algorithm/math/vec2d.h:33
constexpr double kPi = 3.14159265358979323846;   // M_PI
constexpr double kTwoPi = 2.0 * kPi;

// NormalizeAngle (algorithm/math/math_utils.cpp:53-59): fmod(a + pi, 2 pi), plus 2 pi where negative, minus pi.  fmod is
// always exact in IEEE arithmetic, so the short branches return bit-identical values to the library call -- on the
// device they save the call, and the host may take them too.  (-2 pi itself goes to fmod: its -0.0 is not below 0.)
CILQR_HD double normalize_angle(double angle) {
  const double t = angle + kPi;
  double r;
  if (t >= 0.0 && t < kTwoPi) {
    r = t;
  } else if (t >= kTwoPi && t < 2.0 * kTwoPi) {
    r = t - kTwoPi;  // exact (Sterbenz)
  } else if (t < 0.0 && t > -kTwoPi) {
    r = t;
  } else {
    r = fmod(t, kTwoPi);
  }
  if (r < 0.0) r += kTwoPi;
  return r - kPi;
}

// math::slerp (math_utils.h:208-225).  Its degenerate test is `<=`; the pair step's (below) is a strict `<`: a pair
// exactly 1e-10 apart is interpolated, with its heading that of p0.
CILQR_HD double slerp(double a0, double t0, double a1, double t1, double t) {
  if (fabs(t1 - t0) <= kMathEps) return normalize_angle(a0);
  const double a0_n = normalize_angle(a0), a1_n = normalize_angle(a1);
  double d = a1_n - a0_n;
  if (d > kPi) d = d - kTwoPi;
  else if (d < -kPi) d = d + kTwoPi;
  const double r = (t - t0) / (t1 - t0);
  const double a = a0_n + d * r;
  return normalize_angle(a);
}

// bracket: n - 1 for q >= key(n - 1), 0 for q < key(0), else std::lower_bound's halving written out -- the first row whose
// key is not below q; defined and terminating for any keys.  key: int -> double, n >= 2
template <class Key>
CILQR_HD int bracket(int n, double q, Key key) {
  if (q >= key(n - 1)) return n - 1;
  if (q < key(0)) return 0;
  int first = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    if (key(first + half) < q) {
      first += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return first;
}
// ... as the row i of p1 (1 <= i <= n - 1) of the pair a query is evaluated on; p0 is row i - 1
template <class Key>
CILQR_HD int bracket_pair(int n, double q, Key key) {
  int i = bracket(n, q, key);
  if (i == 0) i = 1;
  if (i > n - 1) i = n - 1;   // not reached for sorted keys: q < key(n - 1) here, so the halving stops at or before n - 1
  return i;
}

// hypot as the reference's libm evaluates it.  glibc 2.35 (sysdeps/ieee754/dbl-64/e_hypot.c, the build without FMA
// that x86-64 -O2 binaries get): h = sqrt(ax^2 + ay^2) with ax >= ay, corrected by one Newton step whose residual is
// evaluated in two exact-ish parts.  Written out so that the value depends neither on the C library a caller links nor
// on the device library, whose hypot differs in the last bit on ~0.6 % of arguments (measured against numpy on 200 000
// pairs; this routine on none).  Arguments are lengths in metres: the scaling branches for huge / tiny values are left out.
CILQR_HD double hypot_ref(double x, double y) {
  x = fabs(x);
  y = fabs(y);
  const double ax = x < y ? y : x, ay = x < y ? x : y;
  if (ax >= ay * 0x1p54) return ax + ay;
  double h = sqrt(ax * ax + ay * ay);
  double t1, t2;
  if (h <= 2.0 * ay) {
    const double delta = h - ay;
    t1 = ax * (2.0 * delta - ax);
    t2 = (delta - 2.0 * (ax - ay)) * delta;
  } else {
    const double delta = h - ax;
    t1 = 2.0 * delta * (ax - 2.0 * ay);
    t2 = (4.0 * delta - ay) * ay + delta * delta;
  }
  h -= (t1 + t2) / (2.0 * h);
  return h;
}

// ---- the pair step: one output row from the pair (p0, p1) whose keys k0, k1 bracket the query q
// (LinearInterpolateTrajectory, algorithm/utils/discretized_trajectory.cpp:66-89).  Which columns are produced, where
// each goes and what it is are a list; a kernel passes a constexpr one, and the loops below unroll to constant columns.
enum PairKind {
  kPairLerp,    // (1 - w) a + w b
  kPairKey,     // q where the column is the key column, linear otherwise (the time and station columns)
  kPairSlerp,   // the heading
  kPairHold     // a control holds over its step: p0's bits
};
struct PairColumns {
  int n;
  int from[kMaxRowFields], to[kMaxRowFields], kind[kMaxRowFields];
};
constexpr PairColumns pair_with(PairColumns L, int from, int to, int kind) {
  L.from[L.n] = from;
  L.to[L.n] = to;
  L.kind[L.n] = kind;
  ++L.n;
  return L;
}
// the same columns to out[0 ... n - 1]: for a kernel that holds them in registers before it places them
constexpr PairColumns pair_packed(PairColumns L) {
  for (int e = 0; e < L.n; ++e) L.to[e] = e;
  return L;
}
// every column of a trajectory layout, in place (cilqr_resample_rows)
constexpr PairColumns pair_all(const RowColumns& c) {
  PairColumns L{};
  for (int f = 0; f < c.fields; ++f)
    L = pair_with(L, f, f, (f == c.time || f == c.station) ? kPairKey : f == c.theta ? kPairSlerp
                           : (f == c.jerk || f == c.rate) ? kPairHold : kPairLerp);
  return L;
}
// a centre row, in place: s x y theta kappa left_bound right_bound with the station as its key (key_col = 0)
constexpr PairColumns pair_center() {
  PairColumns L{};
  for (int f = 0; f < 7; ++f) L = pair_with(L, f, f, f == 0 ? kPairKey : f == 3 ? kPairSlerp : kPairLerp);
  return L;
}

// out[to] for every column of L.  A degenerate pair (|k1 - k0| < 1e-10, STRICT -- slerp's own test is `<=`) gives p0 as
// bits, its key column included.  key_col: the column of p0 / p1 that holds the key; -1 where the keys are kept elsewhere.
CILQR_HD void pair_step(const PairColumns& L, int key_col, double k0, double k1, double q, const double* p0, const double* p1,
                        double* out) {
  if (fabs(k1 - k0) < kMathEps) {
    CILQR_HD_UNROLL
    for (int e = 0; e < L.n; ++e) out[L.to[e]] = p0[L.from[e]];   // loads and stores: the bits travel untouched
    return;
  }
  const double w = (q - k0) / (k1 - k0);
  const double w1 = 1 - w;
  CILQR_HD_UNROLL
  for (int e = 0; e < L.n; ++e) {
    const int f = L.from[e];
    const double a = p0[f];
    double v;
    if (L.kind[e] == kPairSlerp) {
      v = slerp(a, k0, p1[f], k1, q);
    } else if (L.kind[e] == kPairHold) {
      v = a;
    } else {
      v = w1 * a + w * p1[f];
      if (L.kind[e] == kPairKey) v = (f == key_col) ? q : v;
    }
    out[L.to[e]] = v;
  }
}

}  // namespace cilqr

#endif  // CILQR_ROW_MATH_HPP_
