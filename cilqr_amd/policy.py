"""The rule of cilqr_policy_rollout_batch (include/cilqr.h, "policy"), stated in plain NumPy: Forward (cc:392-415) from a
start the caller chooses -- control law, clamp, row assembly, summaries.  The dynamics step is an ARGUMENT, so that a test
plugs in a statement of its own (or a recorded rollout); nothing here calls the library, and nothing in the library calls this.

Arrays carry a leading axis of chains (any shape [..., 6] of states): `rollout` runs S samples of B problems as [S, B].
Arithmetic is in `dtype` (float64: the kernel's operations in the kernel's order, one rounding each; numpy.longdouble for a
comparison with a long-double statement).
"""
from __future__ import annotations

import math

import numpy as np

ROWS_TRAJ, ROWS_PLAN = 0, 1
TRAJ_FIELDS = 10
# column of x, y, theta, v, a, delta | jerk, rate in the two layouts that carry states AND controls (row_layouts.hpp)
COLUMNS = {ROWS_TRAJ: ((1, 2, 3, 4, 5, 6), (8, 9), 10), ROWS_PLAN: ((2, 3, 4, 6, 7, 8), (9, 10), 11)}


def normalize_angle(a):
    """NormalizeAngle with the double constants: fmod(a + pi, 2 pi), + 2 pi where negative, - pi"""
    a = np.asarray(a)
    pi, two_pi = a.dtype.type(math.pi), a.dtype.type(2.0 * math.pi)
    r = np.fmod(a + pi, two_pi)
    r = np.where(r < 0, r + two_pi, r)
    return r - pi


def control_law(u_nom, K, dx, k=None, alpha=0.0):
    """u_r = (u*_r + acc) + alpha k_r with acc = K[r][0] dx_0, then += K[r][e] dx_e for e = 1 .. 5; k None: u_r = u*_r + acc.
    u_nom [..., 2], K [..., 2, 6], dx [..., 6], k [..., 2]"""
    acc = K[..., :, 0] * dx[..., None, 0]
    for e in range(1, 6):
        acc = acc + K[..., :, e] * dx[..., None, e]
    u = u_nom + acc
    if k is not None:
        u = u + dx.dtype.type(alpha) * k
    return u


def clamp(u, lo, hi):
    """u < lo ? lo : (u > hi ? hi : u) -- a NaN passes; returns (clamped, a limit was applied)"""
    below, above = u < lo, u > hi
    return np.where(below, lo, np.where(above, hi, u)), below | above


def rollout(rows, layout, Kfb, start6, step, dt, wheel_base, kff=None, alpha=0.0, bounds=None, n_out=None, dtype=np.float64):
    """rows [B, K, F] nominal (ROWS_TRAJ / ROWS_PLAN), Kfb [B, K-1, 2, 6], kff [B, K-1, 2] or None, start6 [S, B, 6].
    step(i, x [S, B, 6], u [S, B, 2]) -> x_next [S, B, 6]: Dynamics(x, u) of step i; u arrives clamped and with u_1 wrapped.
    bounds: None (no clamp) or (jerk_min, jerk_max, delta_rate_min, delta_rate_max).  n_out (None: K) rows are recorded.
    Returns dict(rows [S, B, n_out, 10], max_dev [S, B], end_dev [S, B], n_clamped [S, B] int32)."""
    xc, uc, F = COLUMNS[layout]
    rows = np.asarray(rows).astype(dtype)
    assert rows.ndim == 3 and rows.shape[2] == F
    Kfb = np.asarray(Kfb).astype(dtype)
    kff = None if kff is None else np.asarray(kff).astype(dtype)
    x = np.asarray(start6).astype(dtype)
    S, B = x.shape[:2]
    K = rows.shape[1]
    n_out = K if n_out is None else int(n_out)
    assert 1 <= n_out <= K
    X, U = rows[:, :, xc], rows[:, :, uc]
    out = np.zeros((S, B, n_out, TRAJ_FIELDS), dtype)
    n_clamped = np.zeros((S, B), np.int32)
    dev2_max = None
    for i in range(n_out):
        dx = x - X[None, :, i]
        d2 = dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]
        dev2_max = d2 if dev2_max is None else np.where((d2 > dev2_max) | (d2 != d2), d2, dev2_max)
        dev2_end = d2
        u = np.zeros((S, B, 2), dtype)
        xn = x
        if i < n_out - 1:
            u = control_law(U[None, :, i], Kfb[None, :, i], dx, None if kff is None else kff[None, :, i], alpha)
            if bounds is not None:
                u0, hit0 = clamp(u[..., 0], dtype(bounds[0]), dtype(bounds[1]))
                u1, hit1 = clamp(u[..., 1], dtype(bounds[2]), dtype(bounds[3]))
                u = np.stack([u0, u1], axis=-1)
                n_clamped += (hit0 | hit1).astype(np.int32)
            u = np.stack([u[..., 0], normalize_angle(u[..., 1])], axis=-1)
            xn = np.asarray(step(i, x, u)).astype(dtype)
        out[..., i, 0] = dtype(i) * dtype(dt)
        out[..., i, 1:7] = x
        out[..., i, 7] = np.tan(x[..., 5]) / dtype(wheel_base)
        out[..., i, 8:10] = u
        x = xn
    return dict(rows=out, max_dev=np.sqrt(dev2_max), end_dev=np.sqrt(dev2_end), n_clamped=n_clamped)
