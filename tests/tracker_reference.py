"""An independent statement of the closed-loop tracker init guess, in numpy.longdouble, for tests/test_tracker.py.
A helper module: nothing here is collected.

Written from the behaviour SURVEY.md, DESIGN.md (section (f)-4) and the header of cilqr_amd/csrc/kernels_tracker.hip describe,
not from oracle/tracker_oracle.cc, and in another shape on purpose (numpy matrices, one function per idea):

  * a clock t = 0, h, 2h, ... (h = sumulation_dt) runs while t < t_end + 1e-10.  Every round the vehicle is advanced one RK4
    step of length h under the controls computed from its state BEFORE the step; the state is kept as knot i when the clock
    t of that round is past knot time i * knot_dt - 1e-10, and knot i - 1 receives the controls of that round.  The run fails
    when the clock leaves knots unvisited.  The clock is the time GRID: it is summed in plain doubles (clock_passes()), since
    its comparisons are decisions; everything the state depends on continuously is long double.
  * controls: a point previewed preview_time ahead along the heading is projected on the followed path: nearest knot
    (first minimum of the squared distance), then the point at station s0 + (w . d) / |d| between that knot's two
    neighbours p0, p1 (d = p1 - p0, w = preview - p0), interpolated linearly in station, the heading along the shorter
    arc; two neighbours with (nearly) the same station give p0 itself.  Lateral state: signed offset of the VEHICLE from
    that point's tangent, heading error, steering angle.  Longitudinal state: station of the path at the clock's time
    (linear between the knots around it) minus the projected station, speed error there, acceleration.
  * u = -K state for both, K = (R + B'PB)^-1 B'PA with P from the value iteration P <- A'PA - A'PB (R + B'PB)^-1 B'PA + Q
    started at Q, run while fewer than max_num_iteration rounds are done and |max coefficient of (P_next - P)| > tolerance.
    Lateral model: A = I + [[0, v 0.1, 0], [0, 0, -v / L 0.1], 0] with v = max(2, speed) -- the 0.1 is a literal --, B = (0, 0,
    dt), Q = diag(weight_l, weight_theta, weight_delta), R = weight_delta_rate.  Longitudinal: A = I + [[0, dt, 0], [0, 0,
    -dt], 0], B = (0, 0, dt), Q = diag(weight_s, weight_v, weight_a), R = weight_j.
  * delta_rate and jerk are clamped; after the RK4 step of (x, y, theta, v, delta, a)' = (v cos, v sin, v tan(delta) / L, a,
    delta_rate, jerk) the heading is wrapped, v is held at >= 0, delta is clamped then wrapped, a is clamped.

Angles wrap with the DOUBLE constants pi and 2 pi (the operation is defined with M_PI), evaluated in long double.

track() also counts how often each branch was taken (the census of tests/test_tracker.py).
"""
import math

import numpy as np

LD = np.longdouble
PI = LD(math.pi)
TWO_PI = LD(2.0 * math.pi)
EPS = 1e-10
CENSUS = ("v_below_2", "v_clamped_at_0", "delta_saturated", "acceleration_saturated", "jerk_saturated", "delta_rate_saturated",
          "duplicate_station", "nearest_is_first_knot", "nearest_is_last_knot", "heading_wraps")


def wrap(a):
    r = np.fmod(a + PI, TWO_PI)
    if r < 0:
        r = r + TWO_PI
    return r - PI


def clock_passes(K, knot_dt, h):
    """The time grid in plain doubles: (rounds of the clock, knots passed beyond knot 0)."""
    t, end, i, rounds = knot_dt * 0, knot_dt * (K - 1), 1, 0
    while t < end + EPS:
        rounds += 1
        if i < K and t > knot_dt * i - EPS:
            i += 1
        t += h
    return rounds, i - 1


def riccati_step(A, B, Q, R, P):
    BtP = B @ P
    return A.T @ P @ A - np.outer(A.T @ P @ B, BtP @ A) / (R + BtP @ B) + Q


def gain(A, B, R, P):
    BtP = B @ P
    return (BtP @ A) / (R + BtP @ B)


def dare_gain(A, B, Q, R, tolerance, max_num_iteration):
    """(K, rounds, smallest relative distance of a stopping test to the tolerance)"""
    A, B, Q, R = np.asarray(A, LD), np.asarray(B, LD), np.asarray(Q, LD), LD(R)
    P, rounds, diff, margin = Q.copy(), 0, LD(np.inf), np.inf
    while rounds < max_num_iteration and diff > tolerance:
        Pn = riccati_step(A, B, Q, R, P)
        diff = abs((Pn - P).max())
        if tolerance > 0:
            margin = min(margin, float(abs(diff - LD(tolerance)) / LD(tolerance)))
        P = Pn
        rounds += 1
    return gain(A, B, R, P), rounds, margin


def lateral_model(cfg, speed):
    v = max(LD(2.0), speed)
    A = np.eye(3, dtype=LD)
    A[0, 1] = v * LD(0.1)
    A[1, 2] = -v / LD(cfg["wheel_base"]) * LD(0.1)
    B = np.array([0, 0, cfg["dt"]], LD)
    Q = np.diag(np.array([cfg["weight_l"], cfg["weight_theta"], cfg["weight_delta"]], LD))
    return A, B, Q, LD(cfg["weight_delta_rate"])


def longitudinal_model(cfg):
    dt = LD(cfg["dt"])
    A = np.eye(3, dtype=LD)
    A[0, 1], A[1, 2] = dt, -dt
    B = np.array([0, 0, cfg["dt"]], LD)
    Q = np.diag(np.array([cfg["weight_s"], cfg["weight_v"], cfg["weight_a"]], LD))
    return A, B, Q, LD(cfg["weight_j"])


class Path:
    def __init__(self, coarse, station, knot_dt, census):
        c = np.asarray(coarse, LD)
        self.x, self.y, self.th, self.v = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
        self.s = np.asarray(station, LD)
        self.K, self.knot_dt, self.census = len(self.s), knot_dt, census
        self.times = [knot_dt * i for i in range(self.K)]          # doubles: the knots' times as the caller's dt gives them

    def heading_between(self, a0, s0, a1, s1, s):
        if abs(s1 - s0) <= EPS:
            return wrap(a0)
        a0, a1 = wrap(a0), wrap(a1)
        d = a1 - a0
        if d > PI:
            d, self.census["heading_wraps"] = d - TWO_PI, self.census["heading_wraps"] + 1
        elif d < -PI:
            d, self.census["heading_wraps"] = d + TWO_PI, self.census["heading_wraps"] + 1
        return wrap(a0 + d * (s - s0) / (s1 - s0))

    def project(self, px, py):
        """(station, x, y, heading) of the projection of (px, py)"""
        dx, dy = self.x - px, self.y - py
        near = int(np.argmin(dx * dx + dy * dy))                   # argmin: the first of equal minima
        self.census["nearest_is_first_knot"] += near == 0
        self.census["nearest_is_last_knot"] += near == self.K - 1
        i0, i1 = max(0, near - 1), min(self.K - 1, near + 1)
        if not i0 < i1:
            return self.s[near], self.x[near], self.y[near], self.th[near]
        ex, ey = self.x[i1] - self.x[i0], self.y[i1] - self.y[i0]
        if abs(self.s[i1] - self.s[i0]) < EPS:
            self.census["duplicate_station"] += 1
            return self.s[i0], self.x[i0], self.y[i0], self.th[i0]
        s = self.s[i0] + ((px - self.x[i0]) * ex + (py - self.y[i0]) * ey) / np.sqrt(ex * ex + ey * ey)
        w = (s - self.s[i0]) / (self.s[i1] - self.s[i0])
        return (s, (1 - w) * self.x[i0] + w * self.x[i1], (1 - w) * self.y[i0] + w * self.y[i1],
                self.heading_between(self.th[i0], self.s[i0], self.th[i1], self.s[i1], s))

    def at_time(self, t):
        """(station, speed) at clock time t (a double)"""
        if t >= self.times[-1]:
            j = self.K - 1
        else:
            j = next(i for i, ti in enumerate(self.times) if ti >= t)   # the first knot whose time is not below t
        j = max(j, 1)
        t0, t1 = self.times[j - 1], self.times[j]
        if abs(t1 - t0) < EPS:
            return self.s[j - 1], self.v[j - 1]
        w = (LD(t) - LD(t0)) / (LD(t1) - LD(t0))
        return (1 - w) * self.s[j - 1] + w * self.s[j], (1 - w) * self.v[j - 1] + w * self.v[j]


def clamp(x, lo, hi, census, key):
    y = min(LD(hi), max(LD(lo), x))
    census[key] += int(y != x)
    return y


def track(start4, coarse, station, knot_dt, cfg):
    """cfg: the 22 fields of oracle.TRACKER_CFG_FIELDS by name.  Returns dict(ok, X [K,6] = x y theta v a delta, U [K-1,2] =
    jerk delta_rate, margin, census)."""
    census = dict.fromkeys(CENSUS, 0)
    path = Path(coarse, station, knot_dt, census)
    K, h, L = path.K, cfg["sumulation_dt"], LD(cfg["wheel_base"])
    cap, tol = int(cfg["max_num_iteration"]), cfg["tolerance"]
    k_lon, _, margin = dare_gain(*longitudinal_model(cfg), tol, cap)
    x, y, th, v = (LD(q) for q in start4)
    dl, a = LD(0), LD(0)
    X, U = np.zeros((K, 6), LD), np.zeros((K - 1, 2), LD)
    X[0] = x, y, th, v, a, dl
    lat_cache = {}
    t, end, i = knot_dt * 0, knot_dt * (K - 1), 1
    clock = t
    while t < end + EPS:
        # ---- controls from the state before the step ----
        look = v * LD(cfg["preview_time"])
        ps, px, py, pth = path.project(x + np.cos(th) * look, y + np.sin(th) * look)
        lat = np.array([np.sin(pth) * (x - px) - np.cos(pth) * (y - py), wrap(pth - th), dl], LD)
        ms, mv = path.at_time(clock)
        lon = np.array([ms - ps, mv - v, a], LD)
        census["v_below_2"] += int(v < 2)
        key = max(LD(2.0), v)
        if key not in lat_cache:
            lat_cache = {key: dare_gain(*lateral_model(cfg, v), tol, cap)}     # (a stopped or slow vehicle repeats it)
        k_lat, _, m_lat = lat_cache[key]
        margin = min(margin, m_lat)
        rate = clamp(-(k_lat @ lat), cfg["delta_rate_min"], cfg["delta_rate_max"], census, "delta_rate_saturated")
        jerk = clamp(-(k_lon @ lon), cfg["jerk_min"], cfg["jerk_max"], census, "jerk_saturated")

        # ---- one RK4 step of length h ----
        def f(q):
            return np.array([q[3] * np.cos(q[2]), q[3] * np.sin(q[2]), q[3] * np.tan(q[4]) / L, q[5], rate, jerk], LD)
        q = np.array([x, y, th, v, dl, a], LD)
        hh = LD(h)
        k1 = f(q)
        k2 = f(q + k1 * (hh / 2))
        k3 = f(q + k2 * (hh / 2))
        k4 = f(q + k3 * hh)
        q = q + (k1 + 2 * k2 + 2 * k3 + k4) / 6 * hh
        x, y = q[0], q[1]
        th = wrap(q[2])
        census["heading_wraps"] += int(abs(th - q[2]) > 1)
        census["v_clamped_at_0"] += int(q[3] < 0)
        v = max(LD(0), q[3])
        dl = wrap(clamp(q[4], cfg["delta_min"], cfg["delta_max"], census, "delta_saturated"))
        a = clamp(q[5], cfg["min_acceleration"], cfg["max_acceleration"], census, "acceleration_saturated")
        clock = t
        if i < K and clock > knot_dt * i - EPS:
            X[i] = x, y, th, v, a, dl
            U[i - 1] = jerk, rate
            i += 1
        t += h
    return dict(ok=i == K, X=X, U=U, margin=margin, census=census)
