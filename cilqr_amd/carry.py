"""The carry rule (include/cilqr.h, "carry") in NumPy: a trajectory of the previous planning cycle as the coarse
trajectory of the next, on top of the resample rule (cilqr_amd/resample.py).  Independent of the C++ statement
(include/cilqr/trajectory_queries.hpp: carry_rows), which it is compared against bit for bit.

For rows of one trajectory, an `advance` in seconds and n_knots knots delta_t apart: state 1 (not asked) for a negative
advance; state 2 (refused) for an advance that is a NaN or above max_advance, for rows whose last time is not after their
first, and for a result with a non-finite x, y, theta, velocity, a or delta; otherwise state 0 (kept) and the rows
EvaluateTime gives at (time[0] + advance) + k delta_t, with the time column delta_t k and the station column the running
sum of the chord lengths.  Every row of a trajectory that is not kept is zero.
"""
from __future__ import annotations

import numpy as np

from . import resample

KEPT, NOT_ASKED, REFUSED, OFF_START, HIT = 0, 1, 2, 3, 4
STATE_NAMES = {KEPT: "kept", NOT_ASKED: "not asked", REFUSED: "refused", OFF_START: "off start", HIT: "hit"}
# layout -> the columns of x y theta kappa velocity a delta: the columns 2 ... 8 of a coarse row
COLUMNS = {resample.ROWS_TRAJ: (1, 2, 3, 7, 4, 5, 6), resample.ROWS_PLAN: (2, 3, 4, 5, 6, 7, 8),
           resample.ROWS_COARSE: (2, 3, 4, 5, 6, 7, 8)}
COARSE6 = (2, 3, 4, 6, 7, 8)    # x y theta velocity a delta of a coarse row
KNOTS3 = (2, 3, 4)


def carry_rows(rows, layout: int, advance: float, max_advance: float, n_knots: int, delta_t: float) -> dict:
    """rows [R][F] in `layout` -> dict(state, coarse9 [n_knots,9], coarse6 [n_knots,6], knots3 [n_knots,3],
    station [n_knots])"""
    if layout not in COLUMNS:
        raise ValueError(f"no row layout {layout}")
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[0] < 2 or rows.shape[1] != resample.COLUMNS[layout][0]:
        raise ValueError(f"rows of shape {rows.shape} are not two or more rows of layout {layout}")
    if n_knots < 1 or not delta_t > 0.0:
        raise ValueError("n_knots >= 1 and delta_t > 0")
    advance, delta_t = np.float64(advance), np.float64(delta_t)
    nine = np.zeros((n_knots, 9))
    state = KEPT
    with np.errstate(all="ignore"):
        if advance < 0.0:
            state = NOT_ASKED
        elif not advance <= max_advance or not rows[-1, 0] - rows[0, 0] > 0.0:
            state = REFUSED
        else:
            k = np.arange(n_knots, dtype=np.float64)
            r = resample.resample_rows(rows, layout, (rows[0, 0] + advance) + k * delta_t, resample.KEY_TIME)
            nine[:, 0] = delta_t * k
            nine.view(np.uint64)[:, 2:] = r.view(np.uint64)[:, list(COLUMNS[layout])]
            s = np.float64(0.0)
            for i in range(1, n_knots):     # the running sum is serial by rule
                s = s + np.hypot(nine[i, 2] - nine[i - 1, 2], nine[i, 3] - nine[i - 1, 3])
                nine[i, 1] = s
            if not np.isfinite(nine[:, list(COARSE6)]).all():
                state, nine = REFUSED, np.zeros((n_knots, 9))
    return dict(state=state, coarse9=nine, coarse6=nine[:, list(COARSE6)].copy(), knots3=nine[:, list(KNOTS3)].copy(),
                station=nine[:, 1].copy())


def source_of(state: int, start_xy, row0_xy, first_hit: int, max_start_offset: float) -> int:
    """the selection rule of cilqr_plan_scenes_batch_carry for one scene, first match wins"""
    if state == NOT_ASKED:
        return NOT_ASKED
    if state != KEPT:
        return REFUSED
    with np.errstate(all="ignore"):
        off = np.hypot(np.float64(start_xy[0]) - np.float64(row0_xy[0]), np.float64(start_xy[1]) - np.float64(row0_xy[1]))
    if not off <= max_start_offset:
        return OFF_START
    return HIT if first_hit != -1 else KEPT
