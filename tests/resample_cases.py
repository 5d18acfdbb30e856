"""Crafted trajectories and queries for the resample rule (include/cilqr.h, "resample"), shared by tests/test_resample.py
(host call, NumPy statement, reference, sanitizer program) and tests/test_gpu_resample.py (kernel).

A case is written once in the 11 columns of ROWS_PLAN (time s x y theta kappa velocity a delta jerk delta_rate); the
crafted key values go into BOTH the time and the station column, so the same case serves either key, and
rows_in_layout() gives it in any layout.  Every case names the branches of the rule its queries must reach
(resample.branch_of): the census of the test asserts that each is hit at least once over the table.
"""
import struct
from collections import namedtuple

import numpy as np

from cilqr_amd import api, resample

# generic (plan) column -> column in the layout
PLAN_TO_TRAJ = (0, 2, 3, 4, 6, 7, 8, 5, 9, 10)     # time x y theta v a delta kappa jerk delta_rate
LAYOUTS = (api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE)
KEYS_OF = {api.ROWS_TRAJ: (api.KEY_TIME,), api.ROWS_PLAN: (api.KEY_TIME, api.KEY_STATION),
           api.ROWS_COARSE: (api.KEY_TIME, api.KEY_STATION)}
BRANCHES = ("degenerate", "past_end", "before_start", "first_pair", "search")

# monotone = False: compared host against NumPy only (the reference's std::lower_bound is not defined there)
Case = namedtuple("Case", "name plan queries branches monotone")


def rows_in_layout(layout, plan):
    plan = np.asarray(plan, dtype=np.float64)
    if layout == api.ROWS_PLAN:
        return np.ascontiguousarray(plan)
    if layout == api.ROWS_COARSE:
        return np.ascontiguousarray(plan[..., :9])
    return np.ascontiguousarray(plan[..., PLAN_TO_TRAJ])


def smooth_plan(rng, keys, theta=None):
    """a plausible trajectory on the given key values (in both key columns); headings as given or a slow turn"""
    keys = np.asarray(keys, dtype=np.float64)
    K = len(keys)
    plan = np.zeros((K, 11))
    plan[:, 0] = plan[:, 1] = keys
    th = np.cumsum(rng.uniform(-0.08, 0.08, K)) + rng.uniform(-3.0, 3.0) if theta is None else np.asarray(theta, float)
    plan[:, 4] = th
    step = rng.uniform(0.3, 1.2, K)
    plan[:, 2], plan[:, 3] = np.cumsum(step * np.cos(th)), np.cumsum(step * np.sin(th))
    plan[:, 5] = rng.uniform(-0.2, 0.2, K)
    plan[:, 6] = rng.uniform(0.0, 12.0, K)
    plan[:, 7], plan[:, 8] = rng.uniform(-2.0, 2.0, K), rng.uniform(-0.5, 0.5, K)
    plan[:, 9], plan[:, 10] = rng.uniform(-3.0, 3.0, K), rng.uniform(-0.4, 0.4, K)
    return plan


def crafted_cases():
    rng = np.random.default_rng(811)
    grid = np.arange(11) * 0.1 + 2.0
    cases = []

    def add(name, keys, queries, branches, theta=None, monotone=True, edit=None):
        plan = smooth_plan(rng, keys, theta)
        if edit is not None:
            edit(plan)
        cases.append(Case(name, plan, np.asarray(queries, dtype=np.float64), tuple(branches), monotone))

    add("query equal to a key", grid, [grid[3], grid[7], np.nextafter(grid[3], 9.0), np.nextafter(grid[3], 0.0)], ["search"])
    add("query equal to the first key", grid, [grid[0]], ["first_pair"])        # i = 0 -> 1, w = 0
    add("query equal to the last key", grid, [grid[-1]], ["past_end"])          # the last pair, w = 1
    add("before the first and past the last key", grid, [grid[0] - 0.25, grid[0] - 1e-13, grid[-1] + 1e-13, grid[-1] + 3.0],
        ["before_start", "past_end"])
    dup = np.array([0.0, 0.1, 0.2, 0.2, 0.2, 0.3, 0.4])
    add("duplicate keys", dup, [0.2, 0.15, 0.25, np.nextafter(0.2, 1.0)], ["search"])     # the lower bound
    # of a run of equal keys is its first row, p0 the row before the run: only a run at either END pairs two equal keys
    add("duplicate keys at both ends", [1.0, 1.0, 1.5, 2.0, 2.0], [0.5, 1.0, 2.0, 2.5], ["degenerate"])
    near = np.array([0.0, 0.5, 0.5 + 5e-11, 1.0])
    add("keys 5e-11 apart", near, [0.5 + 2e-11, 0.5 + 5e-11, 0.5], ["degenerate", "search"])
    exact = np.array([-1.0, 0.0, 1e-10, 1.0])          # 1e-10 - 0.0 is 1e-10 exactly: `<` is false, slerp's `<=` is true
    add("keys exactly 1e-10 apart", exact, [5e-11, 1e-10, 2.5e-11], ["search"])
    assert not abs(exact[2] - exact[1]) < 1e-10 and abs(exact[2] - exact[1]) <= 1e-10
    add("headings either side of pi", grid[:6], grid[0] + np.array([0.02, 0.05, 0.11, 0.18, 0.27, 0.33, 0.42, 0.49]), ["search"],
        theta=[3.10, -3.12, 3.13, 3.14159, -3.14159, -3.0])
    add("headings either side of -pi", grid[:5], grid[0] + np.array([0.03, 0.12, 0.2, 0.26, 0.39]), ["search"],
        theta=[-3.05, 3.08, -3.14, 3.11, -3.10])
    add("unwrapped headings near 3 pi", grid[:6], grid[0] + np.array([0.01, 0.07, 0.15, 0.22, 0.38, 0.5, 0.61]), ["search", "past_end"],
        theta=3 * np.pi + np.array([-0.06, -0.01, 0.02, 0.05, -0.03, 0.04]))
    add("two knots", [4.0, 4.5], [3.0, 4.0, 4.2, 4.5, 7.0], ["before_start", "first_pair", "past_end"])
    add("NaN query", grid, [np.nan, grid[2] + 0.03], ["first_pair", "search"])
    add("infinite queries", grid, [np.inf, -np.inf], ["past_end", "before_start"])

    def nan_row(plan):
        plan[4, :] = np.nan
    add("NaN row", grid, [grid[2] + 0.05, grid[3] + 0.05, grid[4] + 0.05, grid[5] + 0.05, grid[4]], ["search"],
        edit=nan_row)

    def nan_values(plan):
        plan[3, 2], plan[6, 4], plan[2, 9] = np.nan, np.inf, np.nan      # x, theta, jerk: the keys stay finite
    add("NaN values under finite keys", grid, grid[0] + np.array([0.15, 0.25, 0.35, 0.55, 0.65]), ["search"], edit=nan_values)
    add("non-monotone keys", [0.0, 0.4, 0.2, 0.6, 0.5, 0.1, 0.9], [0.05, 0.2, 0.3, 0.45, 0.55, 0.7, 0.9, -1.0, 2.0],
        ["search", "past_end", "before_start"], monotone=False)
    # (added last: the cases above keep their draws)  more than 2 pi outside [-pi, pi): the library call of NormalizeAngle
    add("headings far outside [-pi, pi)", grid[:5], grid[0] + np.array([-0.2, 0.0, 0.04, 0.1, 0.17, 0.25, 0.31, 0.4, 0.6]),
        ["before_start", "first_pair", "search", "past_end"], theta=np.pi * np.array([7.5, -9.25, 7.75, -9.0, 40.5]))
    return cases


def random_cases(n=300, seed=812):
    """trajectories with 2 ... 60 knots on irregular, strictly increasing keys; queries inside, on and around the range"""
    rng = np.random.default_rng(seed)
    cases = []
    for j in range(n):
        K = int(rng.integers(2, 61))
        keys = np.cumsum(rng.uniform(0.01, 0.5, K)) + rng.uniform(-5.0, 5.0)
        theta = np.cumsum(rng.uniform(-0.6, 0.6, K)) + rng.uniform(-8.0, 8.0) if j % 3 == 0 else None
        plan = smooth_plan(rng, keys, theta)
        q = np.concatenate([rng.uniform(keys[0] - 0.3, keys[-1] + 0.3, 12), keys[rng.integers(0, K, 3)]])
        cases.append(Case(f"random {j}", plan, q, (), True))
    return cases


def census(cases):
    """branch -> how many (case, key, query) triples of the table reach it"""
    seen = dict.fromkeys(BRANCHES, 0)
    for c in cases:
        for q in c.queries:
            seen[resample.branch_of(c.plan, api.ROWS_PLAN, q, api.KEY_TIME)] += 1
    return seen


def same_rows(a, b):
    """bit for bit -- except that a NaN matches any NaN: which NaN an operation returns is the processor's choice, not the
    rule's (a copied NaN keeps its bits in every implementation, and the tests of the copied columns ask for them)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | both_nan))


def write_cases(path, cases, layout, key):
    """The cases as tests/cpp/trajectory_queries_test.cc reads them (little-endian): "RCASES01", i32 n; per case i32
    layout, i32 key, i32 K, i32 M, rows [K][F], queries [M], expected [M][F] (the NumPy statement's rows)."""
    with open(path, "wb") as o:
        o.write(b"RCASES01" + struct.pack("<i", len(cases)))
        for c in cases:
            rows = rows_in_layout(layout, c.plan)
            want = resample.resample_rows(rows, layout, c.queries, key)
            o.write(struct.pack("<iiii", layout, key, len(rows), len(c.queries)))
            o.write(rows.astype("<f8").tobytes() + c.queries.astype("<f8").tobytes() + want.astype("<f8").tobytes())
