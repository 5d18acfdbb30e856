"""The Frenet rule (include/cilqr.h, "frenet") in NumPy: DiscretizedTrajectory::GetProjection / GetCartesian of the
reference on a centre line [n][7] = s x y theta kappa left_bound right_bound.  Written from the rule, independent of the
C++ statement (include/cilqr/trajectory_queries.hpp), which it is compared against bit for bit; the nearest point and the
bracket are found one query at a time, the arithmetic runs over all queries at once.

Projection of (px, py): `at` = the first centre point with the smallest dx*dx + dy*dy; the pair (max(0, at-1),
min(n-1, at+1)); delta_s = (v0 . v1) / sqrt(v1 . v1) along that pair; the projected point is the pair interpolated at
s_i0 + delta_s (row i0 as it is when the pair's stations are less than 1e-10 apart; extrapolated outside the pair);
lateral = copysign(hypot(nr), nr_y cos(theta) - nr_x sin(theta)) with nr = p - projected point.
Inverse of (station, lateral): the line evaluated at the station by the bracket of the resample rule, shifted by lateral
along its normal.
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

from .resample import MATH_EPSILON, bracket, slerp

CENTER_FIELDS, FRENET_FIELDS = 7, 8
DBL_MAX = np.finfo(np.float64).max

# sincos and hypot are the C library's own, element by element: NumPy may vectorise its own, and the rule names sincos
# (glibc's is not its sin / cos in the last bit for every angle)
_LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_LIBM.hypot.restype = ctypes.c_double
_LIBM.hypot.argtypes = [ctypes.c_double] * 2
_LIBM.sincos.restype = None
_LIBM.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]


def _each(fn, *arrays):
    return np.array([fn(*v) for v in zip(*(np.asarray(a, dtype=np.float64).ravel().tolist() for a in arrays))],
                    dtype=np.float64)


def _center(center):
    center = np.ascontiguousarray(center, dtype=np.float64)
    if center.ndim != 2 or center.shape[0] < 2 or center.shape[1] != CENTER_FIELDS:
        raise ValueError(f"center of shape {center.shape} is not two or more rows of {CENTER_FIELDS}")
    return center


def nearest_index(center, px: float, py: float) -> int:
    """QueryNearestPoint: np.argmin would put a NaN first; the rule's strict `<` from DBL_MAX skips it"""
    with np.errstate(all="ignore"):
        dx, dy = center[:, 1] - px, center[:, 2] - py
        d = dx * dx + dy * dy
    ok = d < DBL_MAX
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (d == d[ok].min()))[0])


def interpolate_center(p0, p1, s):
    """LinearInterpolateTrajectory on centre rows, row by row: p0, p1 [M][7], s [M] -> [M][7]"""
    s0, s1 = p0[:, 0], p1[:, 0]
    with np.errstate(all="ignore"):
        w = ((s - s0) / (s1 - s0))[:, None]
        out = (1 - w) * p0 + w * p1
        out[:, 0] = s
        out[:, 3] = slerp(p0[:, 3], s0, p1[:, 3], s1, s)
        degenerate = np.abs(s1 - s0) < MATH_EPSILON
    out.view(np.uint64)[degenerate] = p0.view(np.uint64)[degenerate]      # as bits
    return out


def frenet_rows(center, xy):
    """center [n][7], xy [M][2] -> (frenet [M][8], cross [M], distance [M]): the rows of the rule, the cross product the
    sign of lateral was taken from, and |nr|"""
    center = _center(center)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    n = center.shape[0]
    at = np.array([nearest_index(center, px, py) for px, py in xy.tolist()], dtype=np.int64)
    i0, i1 = np.maximum(0, at - 1), np.minimum(n - 1, at + 1)      # i0 < i1 for n >= 2
    c0, c1 = center[i0], center[i1]
    with np.errstate(all="ignore"):
        v0x, v0y = xy[:, 0] - c0[:, 1], xy[:, 1] - c0[:, 2]
        v1x, v1y = c1[:, 1] - c0[:, 1], c1[:, 2] - c0[:, 2]
        v1_norm = np.sqrt(v1x * v1x + v1y * v1y)
        dot = v0x * v1x + v0y * v1y
        delta_s = dot / v1_norm
        pp = interpolate_center(c0, c1, c0[:, 0] + delta_s)
        nr_x, nr_y = xy[:, 0] - pp[:, 1], xy[:, 1] - pp[:, 2]
        sn, cs = _libm_trig(pp[:, 3])
        cross = nr_y * cs - nr_x * sn
        distance = _each(_LIBM.hypot, nr_x, nr_y)
    out = np.empty((len(xy), FRENET_FIELDS))
    out[:, 0] = pp[:, 0]
    out[:, 1] = np.copysign(distance, cross)
    out.view(np.uint64)[:, 2:] = pp.view(np.uint64)[:, 1:]
    return out, cross, distance


def branch_of(center, px: float, py: float) -> set:
    """which parts of the rule answer (px, py) -- for the census of tests/frenet_cases.py"""
    center = _center(center)
    n = center.shape[0]
    with np.errstate(all="ignore"):
        d = (center[:, 1] - px) ** 2 + (center[:, 2] - py) ** 2
    at = nearest_index(center, px, py)
    i0, i1 = max(0, at - 1), min(n - 1, at + 1)
    seen = set()
    seen.add("clamp_low" if at == 0 else "clamp_high" if at == n - 1 else "interior")
    if not (d < DBL_MAX).any():
        seen.add("no_distance")
    elif np.count_nonzero(d == d[at]) > 1:
        seen.add("tie")
    s0, s1 = center[i0, 0], center[i1, 0]
    if abs(s1 - s0) < MATH_EPSILON:
        seen.add("degenerate")
    else:
        row, _, dist = frenet_rows(center, [[px, py]])
        with np.errstate(all="ignore"):
            w = (row[0, 0] - s0) / (s1 - s0)
        seen.add("w_below_0" if w < 0 else "w_above_1" if w > 1 else "w_inside" if 0 <= w <= 1 else "w_nan")
        if dist[0] == 0.0:
            seen.add("on_line")
    return seen


def _libm_trig(theta):
    """(sin, cos) by the C library's sincos"""
    theta = np.asarray(theta, dtype=np.float64).ravel()
    sn, cs = ctypes.c_double(), ctypes.c_double()
    out = np.empty((2, len(theta)))
    for i, a in enumerate(theta.tolist()):
        _LIBM.sincos(a, ctypes.byref(sn), ctypes.byref(cs))
        out[0, i], out[1, i] = sn.value, cs.value
    return out[0], out[1]


def cartesian_points(center, sl, trig=None) -> np.ndarray:
    """center [n][7], sl [M][2] station, lateral -> [M][3] x, y, theta.  trig(theta [M]) -> (sin, cos): the C library's
    by default; a test hands in another implementation's"""
    center = _center(center)
    sl = np.ascontiguousarray(sl, dtype=np.float64).reshape(-1, 2)
    stations = center[:, 0].tolist()
    i1 = np.array([bracket(stations, q) for q in sl[:, 0].tolist()], dtype=np.int64)
    ref = interpolate_center(center[i1 - 1], center[i1], sl[:, 0])
    sn, cs = (trig or _libm_trig)(ref[:, 3])
    out = np.empty((len(sl), 3))
    with np.errstate(all="ignore"):
        out[:, 0] = ref[:, 1] - sl[:, 1] * sn
        out[:, 1] = ref[:, 2] + sl[:, 1] * cs
    out.view(np.uint64)[:, 2] = ref.view(np.uint64)[:, 3]
    return out
