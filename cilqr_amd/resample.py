"""The resample rule (include/cilqr.h, "resample") in NumPy: DiscretizedTrajectory::EvaluateTime / EvaluateStation of
the reference on rows in the ROWS_TRAJ / ROWS_PLAN / ROWS_COARSE layouts.  Independent of the C++ statement
(include/cilqr/trajectory_queries.hpp), which it is compared against bit for bit; the bracket is found one query at a time, the arithmetic
runs over all queries at once.

For a query q on the key column (time, or station where the layout has one): the pair of rows (p0, p1) around q by the
reference's lower bound -- the last pair past the end, the first before the start, so the result extrapolates there --
then, if the keys of the pair are less than 1e-10 apart, p0 as it is; otherwise w = (q - key0) / (key1 - key0), the key
column = q, theta by the shorter arc, jerk / delta_rate = p0's (a control holds over its step), every other column
(1 - w) p0 + w p1.
"""
from __future__ import annotations

import math

import numpy as np

ROWS_TRAJ, ROWS_PLAN, ROWS_COARSE = 0, 1, 2
KEY_TIME, KEY_STATION = 0, 1
MATH_EPSILON = 1e-10
# layout -> (doubles per row, time column, station column or None, theta column, first of the two control columns or None)
COLUMNS = {ROWS_TRAJ: (10, 0, None, 3, 8), ROWS_PLAN: (11, 0, 1, 4, 9), ROWS_COARSE: (9, 0, 1, 4, None)}


def key_column(layout: int, key: int) -> int:
    if layout not in COLUMNS:
        raise ValueError(f"no row layout {layout}")
    if key not in (KEY_TIME, KEY_STATION):
        raise ValueError(f"no key {key}")
    col = COLUMNS[layout][1 if key == KEY_TIME else 2]
    if col is None:
        raise ValueError(f"layout {layout} has no station column")
    return col


def normalize_angle(angle):
    """NormalizeAngle (math_utils.cpp:53-59), element by element; np.fmod is the C library's fmod, which is exact"""
    with np.errstate(all="ignore"):
        a = np.fmod(np.asarray(angle, dtype=np.float64) + np.float64(math.pi), np.float64(2.0 * math.pi))
        a = np.where(a < 0.0, a + np.float64(2.0 * math.pi), a)
        return a - np.float64(math.pi)


def slerp(a0, t0, a1, t1, t):
    """math::slerp (math_utils.h:208-225), element by element"""
    with np.errstate(all="ignore"):
        a0_n, a1_n = normalize_angle(a0), normalize_angle(a1)
        d = a1_n - a0_n
        d = np.where(d > math.pi, d - np.float64(2 * math.pi), np.where(d < -math.pi, d + np.float64(2 * math.pi), d))
        r = (t - t0) / (t1 - t0)
        return np.where(np.abs(t1 - t0) <= MATH_EPSILON, a0_n, normalize_angle(a0_n + d * r))


def bracket(keys, q) -> int:
    """index of p1 (p0 is the row before it); keys [K], K >= 2"""
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
    return max(1, min(i, K - 1))


def branch_of(rows, layout: int, q, key: int = KEY_TIME) -> str:
    """which part of the rule answers q: 'degenerate', or where the bracket came from -- 'past_end' (q >= the last key),
    'before_start', 'first_pair' (the lower bound was row 0), 'search' -- for the census of tests/resample_cases.py"""
    rows = np.asarray(rows, dtype=np.float64)
    keys = rows[:, key_column(layout, key)]
    i = bracket(keys, q)
    if abs(keys[i] - keys[i - 1]) < MATH_EPSILON:
        return "degenerate"
    if q >= keys[-1]:
        return "past_end"
    if q < keys[0]:
        return "before_start"
    return "first_pair" if not (keys[0] < q) else "search"


def resample_rows(rows, layout: int, queries, key: int = KEY_TIME) -> np.ndarray:
    """rows [K][F] in `layout`, queries [M] -> [M][F] float64"""
    fields, _, _, c_theta, c_ctrl = COLUMNS[layout] if layout in COLUMNS else (0,) * 5
    kc = key_column(layout, key)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    queries = np.ascontiguousarray(queries, dtype=np.float64).ravel()
    if rows.ndim != 2 or rows.shape[0] < 2 or rows.shape[1] != fields:
        raise ValueError(f"rows of shape {rows.shape} are not two or more rows of layout {layout}")
    bits = rows.view(np.uint64)      # copies go as 64-bit integers: the bits of a NaN survive whatever float copies do
    keys = rows[:, kc]
    key_list = keys.tolist()
    i1 = np.array([bracket(key_list, q) for q in queries.tolist()], dtype=np.int64)
    p0, p1 = rows[i1 - 1], rows[i1]
    k0, k1 = keys[i1 - 1], keys[i1]
    with np.errstate(all="ignore"):
        w = ((queries - k0) / (k1 - k0))[:, None]
        out = (1 - w) * p0 + w * p1
        out[:, kc] = queries
        out[:, c_theta] = slerp(p0[:, c_theta], k0, p1[:, c_theta], k1, queries)
        degenerate = np.abs(k1 - k0) < MATH_EPSILON
    out_bits = out.view(np.uint64)
    if c_ctrl is not None:
        out_bits[:, c_ctrl:c_ctrl + 2] = bits[i1 - 1, c_ctrl:c_ctrl + 2]     # a control holds over its step
    out_bits[degenerate] = bits[i1 - 1][degenerate]
    return out
