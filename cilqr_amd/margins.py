"""The constraint margins of include/cilqr.h ("constraint margins"), stated a second time in plain NumPy doubles.

How far every knot of a trajectory stays inside the constraints of its own solve: the corridor half-planes, the nearest
segment of the left and of the right lane table, the state and control bounds.  Every value is a margin in physical units,
>= 0 satisfied, < 0 violated.  Written from the rule in the header, independently of include/cilqr/constraint_margins.hpp:
that file walks one knot at a time, this one works on all knots of all problems at once, as arrays.  Every operation is one
NumPy ufunc, so every product and sum is rounded once; cos, sin and the one hypot of the disc radius are the C library's
(called through ctypes, as the host call calls them), every other hypot is `hypot_ref`, the evaluation written out.

tests/test_margins.py holds cilqr_constraint_margins to constraint_margins() bit for bit.
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

FIELDS = 8          # corridor, left lane, right lane, velocity, acceleration, steering, jerk, steering rate
WHICH_FIELDS = 6    # corridor disc, corridor plane, left disc, left segment, right disc, right segment
SEG_EPS = 1e-10     # algorithm/math/vec2d.h:33
# per layout (ROWS_TRAJ 0, ROWS_PLAN 1, ROWS_COARSE 2): doubles per row, then the columns of x y theta v a delta jerk rate
COLUMNS = {0: (10, 1, 2, 3, 4, 5, 6, 8, 9), 1: (11, 2, 3, 4, 6, 7, 8, 9, 10), 2: (9, 2, 3, 4, 6, 7, 8, None, None)}

_LIBM = None


def _libm():
    global _LIBM
    if _LIBM is None:
        m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for name, n in (("cos", 1), ("sin", 1), ("hypot", 2)):
            f = getattr(m, name)
            f.restype = ctypes.c_double
            f.argtypes = [ctypes.c_double] * n
        _LIBM = m
    return _LIBM


def _elementwise(name, a):
    f = getattr(_libm(), name)
    a = np.asarray(a, np.float64)
    return np.array([f(float(v)) for v in a.ravel()], np.float64).reshape(a.shape)


def hypot_ref(x, y):
    """hypot as the reference's C library evaluates it for lengths in metres: sqrt of the sum of squares and one Newton step."""
    with np.errstate(all="ignore"):
        x, y = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(y, np.float64))
        swap = x < y
        ax, ay = np.where(swap, y, x), np.where(swap, x, y)
        h = np.sqrt(ax * ax + ay * ay)
        near = h <= 2.0 * ay
        dn, df = h - ay, h - ax
        t1 = np.where(near, ax * (2.0 * dn - ax), 2.0 * df * (ax - 2.0 * ay))
        t2 = np.where(near, (dn - 2.0 * (ax - ay)) * dn, (4.0 * df - ay) * ay + df * df)
        return np.where(ax >= ay * 2.0 ** 54, ax + ay, h - (t1 + t2) / (2.0 * h))


def vehicle(cfg) -> dict:
    """Disc offsets and the two shrink distances, by the expressions the solver fills its parameters with."""
    D = int(cfg.num_of_disc)
    length = cfg.front_hang + cfg.wheel_base + cfg.rear_hang
    radius = _libm().hypot(cfg.width / 2.0, length / 2.0 / D)
    L = (cfg.rear_hang + cfg.wheel_base + cfg.front_hang) / D
    return dict(off=np.array([L * (j - 0.5) - cfg.rear_hang for j in range(D)], np.float64),
                shrink_corridor=radius + cfg.safe_margin, shrink_lane=radius)


def shrink_normalise(a, b, c, shrink, guard):
    """(a, b, c) moved inwards by `shrink` and divided by its 3-norm; guard: a non-finite result becomes (0, 0, -inf)."""
    with np.errstate(all="ignore"):
        c = c - shrink * (a * a + b * b) / hypot_ref(a, b)
        nrm = hypot_ref(hypot_ref(a, b), c)
        pa, pb, pc = a / nrm, b / nrm, c / nrm
        if guard:
            bad = ~(np.isfinite(pa) & np.isfinite(pb) & np.isfinite(pc))
            pa, pb, pc = np.where(bad, 0.0, pa), np.where(bad, 0.0, pb), np.where(bad, -np.inf, pc)
    return pa, pb, pc


def plane_margin(pa, pb, pc, px, py):
    with np.errstate(all="ignore"):
        g = pa * px + pb * py - pc
        m = -g / hypot_ref(pa, pb)
    return np.where(np.isnan(m), -np.inf, m)


def prepare_lane(rows7, shrink) -> dict:
    r = np.asarray(rows7, np.float64).reshape(-1, 7)
    pa, pb, pc = shrink_normalise(r[:, 0], r[:, 1], r[:, 2], shrink, False)
    sx, sy, ex, ey = r[:, 3], r[:, 4], r[:, 5], r[:, 6]
    with np.errstate(all="ignore"):
        dx, dy = ex - sx, ey - sy
        ln = hypot_ref(dx, dy)
        point = ln <= SEG_EPS
        ux, uy = np.where(point, 0.0, dx / ln), np.where(point, 0.0, dy / ln)
    return dict(pa=pa, pb=pb, pc=pc, sx=sx, sy=sy, ex=ex, ey=ey, ux=ux, uy=uy, ln=ln, point=point)


def nearest_segment(tab, px, py, exact_ties):
    """FindNeastLaneSegment for points [...]: the index of the first smallest distance under a strict `<` from DBL_MAX (0 when
    no distance is below it).  exact_ties: the reference's distances; otherwise the same cases on squares alone."""
    P, Q = np.asarray(px, np.float64)[..., None], np.asarray(py, np.float64)[..., None]
    with np.errstate(all="ignore"):
        x0, y0 = P - tab["sx"], Q - tab["sy"]
        x1, y1 = P - tab["ex"], Q - tab["ey"]
        proj = x0 * tab["ux"] + y0 * tab["uy"]
        cross = x0 * tab["uy"] - y0 * tab["ux"]
        at_start = tab["point"] | (proj <= 0.0)
        at_end = proj >= tab["ln"]
        if exact_ties:
            d = np.where(at_start, hypot_ref(x0, y0), np.where(at_end, hypot_ref(x1, y1), np.abs(cross)))
        else:
            d = np.where(at_start, x0 * x0 + y0 * y0, np.where(at_end, x1 * x1 + y1 * y1, cross * cross))
    d = np.where(d < np.finfo(np.float64).max, d, np.inf)      # a NaN or +inf is never taken
    return np.argmin(d, axis=-1)


def nearest_segment_gap(tab, px, py):
    """How far the choice of nearest_segment is from being another: the distance (metres, the reference's values) to the
    nearest segment that is measured to ANOTHER point, minus the distance to the nearest.  Two segments measured to the same
    end point (bitwise equal coordinates: the wedge outside a joint) tie in any arithmetic and the first wins everywhere, so
    they do not count against each other.  +inf with one segment, or where nothing else is finite."""
    n = tab["sx"].size
    ids = {}
    start = np.array([ids.setdefault((float(tab["sx"][k]).hex(), float(tab["sy"][k]).hex()), len(ids)) for k in range(n)])
    end = np.array([ids.setdefault((float(tab["ex"][k]).hex(), float(tab["ey"][k]).hex()), len(ids)) for k in range(n)])
    P, Q = np.asarray(px, np.float64)[..., None], np.asarray(py, np.float64)[..., None]
    with np.errstate(all="ignore"):
        x0, y0 = P - tab["sx"], Q - tab["sy"]
        x1, y1 = P - tab["ex"], Q - tab["ey"]
        proj = x0 * tab["ux"] + y0 * tab["uy"]
        at_start = tab["point"] | (proj <= 0.0)
        at_end = proj >= tab["ln"]
        d = np.where(at_start, hypot_ref(x0, y0), np.where(at_end, hypot_ref(x1, y1), np.abs(x0 * tab["uy"] - y0 * tab["ux"])))
    code = np.where(at_start, start, np.where(at_end, end, 2 * n + np.arange(n)))
    d = np.where(d < np.finfo(np.float64).max, d, np.inf)
    at = np.argmin(d, axis=-1)[..., None]
    best, best_code = np.take_along_axis(d, at, axis=-1), np.take_along_axis(code, at, axis=-1)
    with np.errstate(all="ignore"):
        other = np.where(code != best_code, d, np.inf).min(axis=-1)
        gap = other - best[..., 0]
    return np.where(np.isnan(gap), np.inf, gap)


def _pair(g1, g2):
    with np.errstate(all="ignore"):
        m1, m2 = -g1, -g2
    m1, m2 = np.where(np.isnan(m1), -np.inf, m1), np.where(np.isnan(m2), -np.inf, m2)
    return np.where(m2 < m1, m2, m1)


def constraint_margins(cfg, rows, layout, corridor, count, left, right, exact_ties=True, candidates=False) -> dict:
    """rows [B, K, F] (or [K, F]) in `layout`, corridor [B, K, cmax, 3] raw planes, count [B, K], left / right [n, 7] raw lane
    rows (one lane group).  Returns margins [B, K, 8], which [B, K, 6] int32, min_margin [B, 8], min_knot [B, 8] int32.
    candidates=True adds what the minima were taken over, for tests that ask how close a decision was: corridor_candidates
    [B, K, D * cmax] (disc-major; +inf beyond the count), lane_candidates [2, B, K, D], lane_segments [2, B, K, D] and
    lane_gaps [2, B, K, D] (nearest_segment_gap)."""
    rows = np.asarray(rows, np.float64)
    single = rows.ndim == 2
    if single:
        rows = rows[None]
    F, cx, cy, ct, cv, ca, cd, cj, cr = COLUMNS[layout]
    B, K = rows.shape[:2]
    assert rows.shape[2] == F
    corridor = np.asarray(corridor, np.float64).reshape(B, K, -1, 3)
    cmax = corridor.shape[2]
    count = np.asarray(count).reshape(B, K).astype(np.int64)
    veh = vehicle(cfg)
    off = veh["off"]
    D = off.size
    x, y, theta = rows[..., cx], rows[..., cy], rows[..., ct]
    cs, sn = _elementwise("cos", theta), _elementwise("sin", theta)
    with np.errstate(all="ignore"):
        px = x[..., None] + off * cs[..., None]                # [B, K, D]
        py = y[..., None] + off * sn[..., None]
    margins = np.full((B, K, FIELDS), np.inf)
    which = np.full((B, K, WHICH_FIELDS), -1, np.int32)
    extra = dict(lane_candidates=[], lane_segments=[], lane_gaps=[])

    # corridor: discs outside, planes inside
    n = np.clip(count, 0, cmax)
    live = np.arange(cmax)[None, None, :] < n[..., None]       # [B, K, cmax]
    pa, pb, pc = shrink_normalise(corridor[..., 0], corridor[..., 1], corridor[..., 2], veh["shrink_corridor"], True)
    m = plane_margin(pa[:, :, None, :], pb[:, :, None, :], pc[:, :, None, :], px[..., None], py[..., None])   # [B, K, D, cmax]
    m = np.where(live[:, :, None, :], m, np.inf).reshape(B, K, D * cmax)
    extra["corridor_candidates"] = m
    at = np.argmin(m, axis=-1)                                 # the first of equals
    best = np.take_along_axis(m, at[..., None], axis=-1)[..., 0]
    margins[..., 0] = best
    taken = best < np.inf
    which[..., 0] = np.where(taken, at // cmax, -1)
    which[..., 1] = np.where(taken, at % cmax, -1)

    # lanes: every disc against the plane of its nearest segment
    for side, raw in enumerate((left, right)):
        tab = prepare_lane(raw, veh["shrink_lane"])
        seg = nearest_segment(tab, px, py, exact_ties)         # [B, K, D]
        m = plane_margin(tab["pa"][seg], tab["pb"][seg], tab["pc"][seg], px, py)
        extra["lane_candidates"].append(m)
        extra["lane_segments"].append(seg)
        if candidates:
            extra["lane_gaps"].append(nearest_segment_gap(tab, px, py))
        at = np.argmin(m, axis=-1)
        best = np.take_along_axis(m, at[..., None], axis=-1)[..., 0]
        margins[..., 1 + side] = best
        taken = best < np.inf
        which[..., 2 + 2 * side] = np.where(taken, at, -1)
        which[..., 3 + 2 * side] = np.where(taken, np.take_along_axis(seg, at[..., None], axis=-1)[..., 0], -1)

    # bounds, as DynamicsCost writes its g
    v, a, delta = rows[..., cv], rows[..., ca], rows[..., cd]
    margins[..., 3] = _pair(-v, v - cfg.max_velocity)
    margins[..., 4] = _pair(a - cfg.max_acceleration, cfg.min_acceleration - a)
    margins[..., 5] = _pair(delta - cfg.delta_max, cfg.delta_min - delta)
    if cj is not None and K > 1:
        jerk, rate = rows[:, :K - 1, cj], rows[:, :K - 1, cr]
        margins[:, :K - 1, 6] = _pair(jerk - cfg.jerk_max, cfg.jerk_min - jerk)
        margins[:, :K - 1, 7] = _pair(rate - cfg.delta_rate_max, cfg.delta_rate_min - rate)

    knot = np.argmin(margins, axis=1)                          # [B, 8], the first knot of equals
    min_margin = np.take_along_axis(margins, knot[:, None, :], axis=1)[:, 0, :]
    min_knot = np.where(min_margin < np.inf, knot, -1).astype(np.int32)
    out = dict(margins=margins, which=which, min_margin=min_margin, min_knot=min_knot)
    if candidates and not single:
        out.update(corridor_candidates=extra["corridor_candidates"], **{k: np.stack(extra[k]) for k in
                                                                        ("lane_candidates", "lane_segments", "lane_gaps")})
    return {k: v[0] for k, v in out.items()} if single else out


def violated(min_margin, tol=None):
    """The bit mask of a problem: bit f set when min_margin[..., f] < -tol[f]."""
    tol = np.zeros(FIELDS) if tol is None else np.asarray(tol, np.float64)
    bits = (np.asarray(min_margin, np.float64) < -tol).astype(np.uint32) << np.arange(FIELDS, dtype=np.uint32)
    return bits.sum(axis=-1).astype(np.uint32)
