"""Inputs shared by tests/test_gpu_policy.py and the CPU count its docstrings quote: the perturbed starts of the closed-loop
rollouts that are held against the oracle and against the long-double statement.  A helper module: nothing here is collected.

The set is fixed by reasoning, not by what the kernel gives: offsets of the size a tracking error has after one planning cycle
(at most 0.3 m, 0.05 rad, 0.5 m/s, 0.2 m/s^2, 0.02 rad), both signs of every component, gains at lambda = 1 -- the
regularised law, which keeps the feedback bounded where Quu is nearly singular -- on solved trajectories."""
import numpy as np

REF_B = 32               # scenes of the reference comparison: the first REF_B of the batch whose NOMINAL trajectory is tame
REF_SEED = 1404          # rc.HORIZON_SEED + 1000 + N50_SEED_OFFSET of tests/test_gpu_riccati.py
REF_LAMBDA = 1.0
REF_ALPHAS = (1.0, 0.0)  # with the feed-forward term of the last iterate, and the feedback alone

_OFFSETS = np.array([
    #  x      y     theta    v      a     delta
    [0.30, 0.00, 0.00, 0.0, 0.0, 0.00],
    [0.00, -0.30, 0.00, 0.0, 0.0, 0.00],
    [0.10, 0.20, 0.05, 0.5, 0.0, 0.00],
    [-0.20, 0.10, -0.05, -0.5, 0.0, 0.00],
    [0.00, 0.00, 0.00, 0.0, 0.2, 0.02],
    [0.00, 0.00, 0.00, 0.0, -0.2, -0.02],
    [0.30, -0.30, 0.05, -0.5, 0.2, -0.02],
    [-0.30, 0.30, -0.05, 0.5, -0.2, 0.02],
])


def reference_scenes(X, n=REF_B):
    """indices of the first n trajectories of X [B, K, 6] that are tame themselves (riccati_cases.tame): a plan that steers
    beyond 0.7 rad is not tame from any start, which says nothing about the rollout"""
    import riccati_cases as rc
    idx = [b for b in range(X.shape[0]) if rc.tame(X[b])][:n]
    assert len(idx) == n
    return np.array(idx)


def offsets():
    """[8, 6]: the first four move x, y, theta, v only (what the oracle's set_problem can be given), the last four all six"""
    return _OFFSETS.copy()


def rows_of(X, U, layout, fill=np.nan):
    """trajectory rows in `layout` (0 TRAJ, 1 PLAN) from X [B, K, 6] and U [B, K-1, 2]; every column the policy calls do not
    read -- time, station, kappa, the last row's controls -- holds `fill`"""
    from cilqr_amd import policy
    xc, uc, F = policy.COLUMNS[layout]
    rows = np.full((X.shape[0], X.shape[1], F), fill)
    rows[:, :, xc] = X
    rows[:, :-1, uc] = U
    return rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
