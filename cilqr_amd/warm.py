"""The gather rule of a warm start (cilqr_warm_start, include/cilqr.h) in NumPy: what the GPU kernels are held against.

For problem b with s = shift[b] (shift None: 0 for every problem) and every step i < N, with r = i + s:
U[b, i] = the two control columns of row r of the problem's warm rows if 0 <= s and r < N -- the bits are copied, neither
clamped nor angle-wrapped -- and (0, 0) if r >= N.  A problem with s < 0 is not warm-started: its rows of the result are
zero and mean nothing (the solver gives it the configured init guess).
"""
from __future__ import annotations

import numpy as np

ROWS_TRAJ, ROWS_PLAN, ROWS_COARSE, ROWS_CONTROLS = 0, 1, 2, 3
# layout -> (doubles per row, first control column); ROWS_COARSE carries no controls
CONTROL_COLUMNS = {ROWS_TRAJ: (10, 8), ROWS_PLAN: (11, 9), ROWS_CONTROLS: (2, 0)}


def rows_per_problem(layout: int, n_steps: int) -> int:
    """rows the layout stores per problem: the N steps for ROWS_CONTROLS, the N + 1 knots otherwise"""
    if layout not in CONTROL_COLUMNS:
        raise ValueError(f"layout {layout} carries no controls")
    return n_steps if layout == ROWS_CONTROLS else n_steps + 1


def warm_controls(rows, shift, layout: int, n_steps: int) -> np.ndarray:
    """rows [B][K][10] | [B][K][11] | [B][N][2], shift [B] ints or None -> U [B][N][2] float64, bit for bit"""
    if layout not in CONTROL_COLUMNS:
        raise ValueError(f"layout {layout} carries no controls")
    stride, col = CONTROL_COLUMNS[layout]
    rows = np.asarray(rows, dtype=np.float64)
    N = int(n_steps)
    if rows.ndim != 3 or rows.shape[1] < rows_per_problem(layout, N) or rows.shape[2] != stride:
        raise ValueError(f"rows of shape {rows.shape} do not fit layout {layout} with {N} steps")
    B = rows.shape[0]
    s = np.zeros(B, np.int64) if shift is None else np.asarray(shift).astype(np.int64).reshape(B)
    # moved as 64-bit integers: the bits of a NaN payload survive whatever the host's float copies do
    src = np.ascontiguousarray(rows[:, :N, col:col + 2]).view(np.uint64)
    U = np.zeros((B, N, 2), np.uint64)
    for b in range(B):
        sb = int(s[b])
        if sb < 0 or sb >= N:     # compared before anything is added: 2**31 - 1 is a shift like any other
            continue
        U[b, :N - sb] = src[b, sb:]
    return U.view(np.float64)
