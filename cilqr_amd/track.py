"""The track rule (include/cilqr.h, "track") in plain Python doubles: the closed-loop Tracker of the reference
(Tracker::Plan, algorithm/ilqr/tracker.cc) driving a vehicle along rows in the ROWS_TRAJ / ROWS_PLAN / ROWS_COARSE
layouts.  Independent of the C++ statement (include/cilqr/tracker.hpp), which it is compared against bit for bit: a
Python float is an IEEE double and every operation below rounds once; sin / cos (one sincos call) and tan are the C
library's, called through ctypes where the host call calls them.  One trajectory at a time.

The vehicle is simulated at sumulation_dt with RK4.  Every step a point previewed along the heading is projected on
the followed rows (nearest row, then along the chord between its neighbours, linear in station), the followed
trajectory is evaluated at the clock's time, and two 3-state LQR controllers -- the lateral one re-solved every step,
the longitudinal one once -- give delta_rate and jerk, both clamped.  The state is recorded whenever the clock passes
a row's time; the row before it receives the controls of that step.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import math

import numpy as np

ROWS_TRAJ, ROWS_PLAN, ROWS_COARSE = 0, 1, 2
MATH_EPSILON = 1e-10
DBL_MAX = 1.7976931348623157e308
MAX_SIM_STEPS = 32768   # CILQR_TRACKER_MAX_SIM_STEPS
DRIVEN_FIELDS = 10      # CILQR_TRAJ_FIELDS
# layout -> (doubles per row, time, station or None, x (y follows), theta, v, a, delta)
COLUMNS = {ROWS_TRAJ: (10, 0, None, 1, 3, 4, 5, 6), ROWS_PLAN: (11, 0, 1, 2, 4, 6, 7, 8), ROWS_COARSE: (9, 0, 1, 2, 4, 6, 7, 8)}
TRACKER_FIELDS = ("weight_l", "weight_theta", "weight_delta", "weight_delta_rate", "preview_time", "weight_s", "weight_v",
                  "weight_a", "weight_j", "sumulation_dt", "dt", "tolerance", "max_num_iteration")
VEHICLE_FIELDS = ("wheel_base", "delta_min", "delta_max", "delta_rate_min", "delta_rate_max", "jerk_min", "jerk_max",
                  "min_acceleration", "max_acceleration")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tan.restype = ctypes.c_double
_libm.tan.argtypes = [ctypes.c_double]
_libm.sin.restype = _libm.cos.restype = ctypes.c_double
_libm.sin.argtypes = _libm.cos.argtypes = [ctypes.c_double]
_HAVE_SINCOS = hasattr(_libm, "sincos")
if _HAVE_SINCOS:
    _libm.sincos.restype = None
    _libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]


def sin_cos(angle: float):
    if _HAVE_SINCOS:
        s, c = ctypes.c_double(), ctypes.c_double()
        _libm.sincos(angle, ctypes.byref(s), ctypes.byref(c))
        return s.value, c.value
    return _libm.sin(angle), _libm.cos(angle)


def tan(angle: float) -> float:
    return _libm.tan(angle)


def fmax(a: float, b: float) -> float:
    """fmax written out as the host statement has it: a NaN loses, of equal arguments the first wins"""
    return a if (a >= b or b != b) else b


def fmin(a: float, b: float) -> float:
    return a if (a <= b or b != b) else b


def div(a: float, b: float) -> float:
    """IEEE division (Python raises where C returns an infinity or a NaN)"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def fmod(a: float, b: float) -> float:
    try:
        return math.fmod(a, b)
    except ValueError:
        return math.nan


def sqrt(a: float) -> float:
    try:
        return math.sqrt(a)
    except ValueError:
        return math.nan


def normalize_angle(angle: float) -> float:
    a = fmod(angle + math.pi, 2.0 * math.pi)
    if a < 0.0:
        a += 2.0 * math.pi
    return a - math.pi


def slerp(a0: float, t0: float, a1: float, t1: float, t: float) -> float:
    if abs(t1 - t0) <= MATH_EPSILON:
        return normalize_angle(a0)
    a0_n, a1_n = normalize_angle(a0), normalize_angle(a1)
    d = a1_n - a0_n
    if d > math.pi:
        d = d - 2 * math.pi
    elif d < -math.pi:
        d = d + 2 * math.pi
    r = div(t - t0, t1 - t0)
    return normalize_angle(a0_n + d * r)


def hypot_ref(x: float, y: float) -> float:
    """hypot as glibc 2.35 evaluates it without fused multiply-add"""
    x, y = abs(x), abs(y)
    ax, ay = (y, x) if x < y else (x, y)
    if ax >= ay * 2.0 ** 54:
        return ax + ay
    h = sqrt(ax * ax + ay * ay)
    if h <= 2.0 * ay:
        delta = h - ay
        t1 = ax * (2.0 * delta - ax)
        t2 = (delta - 2.0 * (ax - ay)) * delta
    else:
        delta = h - ax
        t1 = 2.0 * delta * (ax - 2.0 * ay)
        t2 = (4.0 * delta - ay) * ay + delta * delta
    return h - div(t1 + t2, 2.0 * h)


def bracket(keys, q: float) -> int:
    """the row index i (1 <= i <= K - 1) of the pair (i - 1, i) around q ("resample")"""
    K = len(keys)
    if q >= keys[K - 1]:
        i = K - 1
    elif q < keys[0]:
        i = 0
    else:
        first, length = 0, K
        while length > 0:
            half = length >> 1
            if keys[first + half] < q:
                first += half + 1
                length -= half + 1
            else:
                length = half
        i = first
    if i == 0:
        i = 1
    return min(i, K - 1)


def _dot3(a, b) -> float:
    s = a[0] * b[0]
    s += a[1] * b[1]
    s += a[2] * b[2]
    return s


def _mul33(a, b):
    return [[_dot3(a[i], (b[0][j], b[1][j], b[2][j])) for j in range(3)] for i in range(3)]


def _row33(v, m):
    return [_dot3(v, (m[0][j], m[1][j], m[2][j])) for j in range(3)]


def solve_lqr(A, B, Q, R: float, tolerance: float, max_iter: int):
    """K [3] of the rule's value iteration"""
    AT = [[A[j][i] for j in range(3)] for i in range(3)]
    P = [row[:] for row in Q]
    rounds, diff = 0, DBL_MAX
    while rounds < max_iter and diff > tolerance:
        rounds += 1
        ATP = _mul33(AT, P)
        ATPA = _mul33(ATP, A)
        ATPB = [_dot3(ATP[i], B) + 0.0 for i in range(3)]
        BTP = _row33(B, P)
        inv = div(1.0, R + _dot3(BTP, B))
        BTPA = _row33(BTP, A)
        maxc = -DBL_MAX
        Pn = [[0.0] * 3 for _ in range(3)]
        for i in range(3):
            left = ATPB[i] * inv
            for j in range(3):
                pn = (ATPA[i][j] - left * (BTPA[j] + 0.0)) + Q[i][j]
                maxc = fmax(maxc, pn - P[i][j])
                Pn[i][j] = pn
        diff = abs(maxc)
        P = Pn
    BTP = _row33(B, P)
    inv = div(1.0, R + _dot3(BTP, B))
    BTPA = _row33(BTP, A)
    return [inv * (BTPA[j] + 0.0) for j in range(3)]


def _field(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def track_rows(cfg, tcfg, rows, layout: int, start6=None, n_drive: int | None = None, max_steps: int = MAX_SIM_STEPS):
    """cfg: the vehicle (an api.Config, or a dict with VEHICLE_FIELDS); tcfg: the tracker's configuration (an
    api.TrackerConfig, or a dict with TRACKER_FIELDS); rows [K,F] in `layout`; start6 = x y theta v a delta (None: row 0);
    n_drive (None: K).  Returns (driven [n_drive,10] in ROWS_TRAJ layout, ok); ok False: the rows are zero."""
    if layout not in COLUMNS:
        raise ValueError(f"no row layout {layout}")
    F, c_t, c_s, c_x, c_th, c_v, c_a, c_d = COLUMNS[layout]
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != F or rows.shape[0] < 2:
        raise ValueError(f"rows must be [K >= 2, {F}]")
    K = rows.shape[0]
    D = K if n_drive is None else int(n_drive)
    if not 1 <= D <= K:
        raise ValueError("n_drive must be 1 ... K")
    T = {k: float(_field(tcfg, k)) for k in TRACKER_FIELDS[:-1]}
    max_iter = int(_field(tcfg, "max_num_iteration"))
    V = {k: float(_field(cfg, k)) for k in VEHICLE_FIELDS}
    L = V["wheel_base"]
    ft, fx, fy = rows[:, c_t].tolist(), rows[:, c_x].tolist(), rows[:, c_x + 1].tolist()
    fth, fv = rows[:, c_th].tolist(), rows[:, c_v].tolist()
    if c_s is not None:
        fs = rows[:, c_s].tolist()
    else:
        fs, acc = [0.0] * K, 0.0
        for k in range(1, K):
            acc = acc + hypot_ref(fx[k] - fx[k - 1], fy[k] - fy[k - 1])
            fs[k] = acc
    dt = T["dt"]
    latA = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    latB = [0.0, 0.0, 1.0 * dt]
    latQ = [[T["weight_l"], 0.0, 0.0], [0.0, T["weight_theta"], 0.0], [0.0, 0.0, T["weight_delta"]]]
    lonA = [[1.0, dt, 0.0], [0.0, 1.0, -dt], [0.0, 0.0, 1.0]]
    lonB = [0.0, 0.0, 1.0 * dt]
    lonQ = [[T["weight_s"], 0.0, 0.0], [0.0, T["weight_v"], 0.0], [0.0, 0.0, T["weight_a"]]]
    k_lon = solve_lqr(lonA, lonB, lonQ, T["weight_j"], T["tolerance"], max_iter)

    if start6 is not None:
        cx, cy, cth, cv, ca, cdl = (float(q) for q in np.asarray(start6, dtype=np.float64).ravel())
    else:
        cx, cy, cth, cv, ca, cdl = (float(rows[0, c]) for c in (c_x, c_x + 1, c_th, c_v, c_a, c_d))
    driven = np.zeros((D, DRIVEN_FIELDS))

    def record(i, time):
        driven[i] = time, cx, cy, cth, cv, ca, cdl, div(tan(cdl), L), 0.0, 0.0

    start_time, end_time = ft[0], ft[K - 1]
    record(0, start_time)
    ctime, i, steps, t = start_time, 1, 0, start_time
    h, preview = T["sumulation_dt"], T["preview_time"]
    h2 = h / 2.0
    while t < end_time + MATH_EPSILON and i < D and steps < max_steps:
        # ---- preview and projection
        sn, cs = sin_cos(cth)
        pvx = cx + cs * cv * preview
        pvy = cy + sn * cv * preview
        at, nearest = 0, DBL_MAX
        for k in range(K):
            dx, dy = fx[k] - pvx, fy[k] - pvy
            d = dx * dx + dy * dy
            if d < nearest:
                nearest, at = d, k
        ps, px, py, pth = fs[at], fx[at], fy[at], fth[at]
        i0, i1 = max(0, at - 1), min(K - 1, at + 1)
        if i0 < i1:
            v0x, v0y = pvx - fx[i0], pvy - fy[i0]
            v1x, v1y = fx[i1] - fx[i0], fy[i1] - fy[i0]
            v1_norm = sqrt(v1x * v1x + v1y * v1y)
            dot = v0x * v1x + v0y * v1y
            st = fs[i0] + div(dot, v1_norm)
            if abs(fs[i1] - fs[i0]) < MATH_EPSILON:
                ps, px, py, pth = fs[i0], fx[i0], fy[i0], fth[i0]
            else:
                w = div(st - fs[i0], fs[i1] - fs[i0])
                ps = st
                px = (1 - w) * fx[i0] + w * fx[i1]
                py = (1 - w) * fy[i0] + w * fy[i1]
                pth = slerp(fth[i0], fs[i0], fth[i1], fs[i1], st)
        psn, pcs = sin_cos(pth)
        ddx, ddy = cx - px, cy - py
        lat = (psn * ddx - pcs * ddy, normalize_angle(pth - cth), cdl)
        # ---- the followed trajectory at the clock's time
        time = ctime + 0.0
        it = bracket(ft, time)
        t0, t1 = ft[it - 1], ft[it]
        if abs(t1 - t0) < MATH_EPSILON:
            match_s, match_v = fs[it - 1], fv[it - 1]
        else:
            w = div(time - t0, t1 - t0)
            match_s = (1 - w) * fs[it - 1] + w * fs[it]
            match_v = (1 - w) * fv[it - 1] + w * fv[it]
        lon = (match_s - ps, match_v - cv, ca)
        # ---- controls
        v_amend = fmax(2.0, cv)
        latA[0][1] = v_amend * 0.1
        latA[1][2] = div(-v_amend, L) * 0.1
        k_lat = solve_lqr(latA, latB, latQ, T["weight_delta_rate"], T["tolerance"], max_iter)
        delta_rate = -_dot3(k_lat, lat)
        jerk = -_dot3(k_lon, lon)
        delta_rate = fmax(V["delta_rate_min"], fmin(V["delta_rate_max"], delta_rate))
        jerk = fmax(V["jerk_min"], fmin(V["jerk_max"], jerk))

        # ---- RK4
        def mode(th, v, dl):
            s_, c_ = sin_cos(th)
            return v * c_, v * s_, div(v * tan(dl), L)

        k1 = mode(cth, cv, cdl)
        a1, a2, a3, a4 = ca, ca + jerk * h2, ca + jerk * h2, ca + jerk * h
        k2 = mode(cth + k1[2] * h2, cv + a1 * h2, cdl + delta_rate * h2)
        k3 = mode(cth + k2[2] * h2, cv + a2 * h2, cdl + delta_rate * h2)
        k4 = mode(cth + k3[2] * h, cv + a3 * h, cdl + delta_rate * h)
        nx = cx + (k1[0] + k2[0] * 2.0 + k3[0] * 2.0 + k4[0]) / 6.0 * h
        ny = cy + (k1[1] + k2[1] * 2.0 + k3[1] * 2.0 + k4[1]) / 6.0 * h
        nth = normalize_angle(cth + (k1[2] + k2[2] * 2.0 + k3[2] * 2.0 + k4[2]) / 6.0 * h)
        nv = fmax(0.0, cv + (a1 + a2 * 2.0 + a3 * 2.0 + a4) / 6.0 * h)
        ndl = normalize_angle(fmin(V["delta_max"], fmax(V["delta_min"], cdl + (delta_rate + delta_rate * 2.0 + delta_rate * 2.0
                                                                               + delta_rate) / 6.0 * h)))
        na = fmin(V["max_acceleration"], fmax(V["min_acceleration"], ca + (jerk + jerk * 2.0 + jerk * 2.0 + jerk) / 6.0 * h))
        cx, cy, cth, cv, cdl, ca = nx, ny, nth, nv, ndl, na
        ctime = t
        if i < K and ctime > ft[i] - MATH_EPSILON:
            driven[i - 1, 8] = jerk
            driven[i - 1, 9] = delta_rate
            record(i, ctime)
            i += 1
        t += h
        steps += 1
    if i == D:
        return driven, True
    driven[:] = 0.0
    return driven, False
