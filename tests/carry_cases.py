"""Crafted trajectories for the carry rule (include/cilqr.h, "carry"): one case per branch of the rule, each with the
state it must end in and the branches of the resample rule its knots must reach.  Shared by tests/test_carry.py (host
call against the NumPy statement and an independent composition) and tests/test_gpu_carry.py (kernel against host call)."""
from collections import namedtuple

import numpy as np

import resample_cases as rc
from cilqr_amd import api, carry, resample

LAYOUTS = rc.LAYOUTS
DT = 0.1
# plan: [R,11] rows in ROWS_PLAN layout (rc.rows_in_layout gives the other two); branches: resample branches some knot reaches
Case = namedtuple("Case", "name plan advance max_advance n_knots delta_t state branches")
NEEDED = ("advance 0", "advance on a knot", "advance between knots", "advance past the last row", "advance equal to max_advance",
          "advance just above max_advance", "negative advance", "NaN advance", "two rows", "duplicated time", "all-zero rows",
          "NaN in one column of one row", "NaN time in the last row", "heading across pi", "heading across -pi",
          "NaN kappa is carried", "one knot", "infinite velocity past the end")


def crafted_cases():
    rng = np.random.default_rng(1711)
    grid = np.arange(11) * DT + 2.0          # eleven rows, 2.0 ... 3.0
    cases = []

    def add(name, keys, advance, state, branches=(), max_advance=1.0, n_knots=6, delta_t=DT, theta=None, edit=None):
        plan = rc.smooth_plan(rng, keys, theta)
        if edit is not None:
            edit(plan)
        cases.append(Case(name, plan, float(advance), float(max_advance), int(n_knots), float(delta_t), state, tuple(branches)))

    add("advance 0", grid, 0.0, carry.KEPT, ("first_pair", "search"))
    add("advance on a knot", grid, grid[3] - grid[0], carry.KEPT, ("search",))
    add("advance between knots", grid, 0.234, carry.KEPT, ("search",))
    add("advance past the last row", grid, 0.55, carry.KEPT, ("search", "past_end"), n_knots=10)     # knots 5 ... 9 extrapolate
    add("advance equal to max_advance", grid, 0.5, carry.KEPT, ("search",), max_advance=0.5)
    add("advance just above max_advance", grid, np.nextafter(0.5, 1.0), carry.REFUSED, max_advance=0.5)
    add("infinite advance", grid, np.inf, carry.REFUSED)
    add("negative advance", grid, -1.0, carry.NOT_ASKED)
    add("negative zero advance", grid, -0.0, carry.KEPT, ("first_pair",))
    add("tiny negative advance", grid, -5e-324, carry.NOT_ASKED)
    add("NaN advance", grid, np.nan, carry.REFUSED)
    add("two rows", [4.0, 4.5], 0.2, carry.KEPT, ("search", "past_end"), n_knots=6)
    # a degenerate pair answers a knot only at the ends: inside, the lower bound is the first of the equal rows
    add("duplicated time", [0.0, 0.0, 0.1, 0.2, 0.3], 0.0, carry.KEPT, ("degenerate", "search"), n_knots=4)
    add("duplicated time in the middle", [0.0, 0.1, 0.2, 0.2, 0.2, 0.3, 0.4], 0.05, carry.KEPT, ("search",), n_knots=4)
    add("duplicated time at the end", [0.0, 0.1, 0.2, 0.2], 0.1, carry.KEPT, ("degenerate",), n_knots=4)
    add("all-zero rows", grid, 0.1, carry.REFUSED, edit=lambda p: p.fill(0.0))
    add("equal first and last time", [1.0, 1.1, 1.0], 0.05, carry.REFUSED)
    add("times running backwards", grid[::-1].copy(), 0.1, carry.REFUSED)

    def nan_x(p):
        p[4, 2] = np.nan
    add("NaN in one column of one row", grid, 0.05, carry.REFUSED, edit=nan_x)

    def nan_x_out_of_reach(p):
        p[9, 2] = np.nan
    add("NaN in a row no knot reaches", grid, 0.05, carry.KEPT, ("search",), edit=nan_x_out_of_reach, n_knots=6)

    def nan_last_time(p):
        p[-1, 0] = np.nan
    add("NaN time in the last row", grid, 0.05, carry.REFUSED, edit=nan_last_time)

    def nan_kappa(p):
        p[:, 5] = np.nan
    add("NaN kappa is carried", grid, 0.05, carry.KEPT, ("search",), edit=nan_kappa)

    def inf_v(p):
        p[-1, 6] = np.inf
    add("infinite velocity past the end", grid, 0.95, carry.REFUSED, edit=inf_v, n_knots=3)
    near_pi = np.pi - 0.05 + 0.02 * np.arange(11)            # crosses +pi between rows 2 and 3
    add("heading across pi", grid, 0.13, carry.KEPT, ("search",), theta=near_pi)
    add("heading across -pi", grid, 0.13, carry.KEPT, ("search",), theta=-near_pi)
    add("unwrapped headings near 3 pi", grid, 0.13, carry.KEPT, ("search",), theta=3 * np.pi - 0.06 + 0.012 * np.arange(11))
    add("one knot", grid, 0.31, carry.KEPT, ("search",), n_knots=1)
    add("fifty-one knots over fifty-one rows", np.arange(51) * DT, 0.5, carry.KEPT, ("search", "past_end"), n_knots=51, max_advance=2.0)
    add("the limit of rows and knots", np.arange(256) * 0.02 + 1.0, 0.011, carry.KEPT, ("search", "past_end"), n_knots=256,
        delta_t=0.03, max_advance=2.0)
    # (added last: the cases above keep their draws)  1e-10 - 0.0 is 1e-10 exactly: the pair is interpolated (`<`), its
    # heading that of its first row (slerp's own `<=`); the first knot lies inside the pair, or on its second key
    add("times exactly 1e-10 apart, a knot inside", [0.0, 1e-10, 1.0], 5e-11, carry.KEPT, ("search",), n_knots=3,
        delta_t=0.25, theta=[1.0, 2.5, 2.75])
    add("times exactly 1e-10 apart, a knot on the second", [0.0, 1e-10, 1.0], 1e-10, carry.KEPT, ("search",), n_knots=3,
        delta_t=0.25, theta=[1.0, 2.5, 2.75])
    # more than 2 pi outside [-pi, pi): the library call of NormalizeAngle
    add("headings far outside [-pi, pi)", grid, 0.13, carry.KEPT, ("search",),
        theta=np.pi * np.array([7.5, -9.25, 7.75, -9.0, 40.5, 7.5, 7.6, -9.25, -9.3, 7.5, -7.5]))
    return cases


def knot_branches(case):
    """the resample branches the knots of a case reach (none unless the first two tests of the rule pass)"""
    t = case.plan[:, 0]
    if not (case.advance >= 0.0 and case.advance <= case.max_advance and t[-1] - t[0] > 0.0):
        return set()
    q = (t[0] + case.advance) + np.arange(case.n_knots) * case.delta_t
    return {resample.branch_of(case.plan, api.ROWS_PLAN, v) for v in q}


def census(cases):
    """state -> cases that end in it; branch -> kept cases with a knot in it"""
    states = {s: 0 for s in (carry.KEPT, carry.NOT_ASKED, carry.REFUSED)}
    branches = dict.fromkeys(rc.BRANCHES, 0)
    for c in cases:
        states[c.state] += 1
        if c.state == carry.KEPT:
            for b in knot_branches(c):
                branches[b] += 1
    return states, branches


def host_carry(case, layout):
    return api.carry_rows(rc.rows_in_layout(layout, case.plan), layout, case.advance, case.max_advance, case.n_knots, case.delta_t)


def same_result(a, b):
    """state equal; the four arrays bit for bit, a NaN matching a NaN (rc.same_rows)"""
    return int(a["state"]) == int(b["state"]) and all(rc.same_rows(a[k], b[k]) for k in ("coarse9", "coarse6", "knots3", "station"))


def random_cases(n=120, seed=1712):
    """trajectories of 2 ... 60 rows on irregular increasing times; advances inside, at and beyond the span and the limit"""
    rng = np.random.default_rng(seed)
    cases = []
    for j in range(n):
        R = int(rng.integers(2, 61))
        keys = np.cumsum(rng.uniform(0.01, 0.3, R)) + rng.uniform(-3.0, 3.0)
        theta = np.cumsum(rng.uniform(-0.5, 0.5, R)) + rng.uniform(-7.0, 7.0) if j % 2 else None
        plan = rc.smooth_plan(rng, keys, theta)
        span = keys[-1] - keys[0]
        advance = float(rng.choice([0.0, keys[int(rng.integers(0, R))] - keys[0], rng.uniform(0, span), rng.uniform(span, 2 * span), -0.3]))
        max_advance = float(rng.choice([advance, 1.5 * span, 0.5 * span])) if advance >= 0 else 1.0
        cases.append(Case(f"random {j}", plan, advance, max_advance, int(rng.integers(1, 70)), float(rng.uniform(0.02, 0.2)), None, ()))
    return cases


ADVANCE_KINDS = ("zero", "on a knot", "between knots", "past the end", "at the limit", "above the limit", "negative", "nan")
ROW_KINDS = ("plain", "duplicate first time", "duplicate last time", "all zero", "nan x", "across pi", "nan kappa", "irregular times")
BATCH_MAX_ADVANCE = 0.5


def make_batch(B, R, seed, delta=DT):
    """plans [B,R,11] on times delta apart and advance [B] for max_advance = BATCH_MAX_ADVANCE: trajectory b takes advance kind
    b % 8 and row kind (b // 8) % 8, so 64 trajectories hold every pair; returns (plans, advance, kinds [B] of pairs)"""
    rng = np.random.default_rng(seed)
    plans, advance, kinds = np.zeros((B, R, 11)), np.zeros(B), []
    for b in range(B):
        ak, rk = ADVANCE_KINDS[b % 8], ROW_KINDS[(b // 8) % 8]
        t = rng.uniform(-2.0, 5.0) + np.arange(R) * delta
        theta = None
        if rk == "irregular times":
            t = t[0] + np.cumsum(rng.uniform(0.3 * delta, 1.7 * delta, R))
        elif rk == "across pi":
            theta = (np.pi - 0.03 if b % 2 else -np.pi + 0.03) + 0.02 * np.arange(R) * (1 if b % 2 else -1)
        p = rc.smooth_plan(rng, t, theta)
        if rk == "duplicate first time":
            p[1, 0] = p[0, 0]
        elif rk == "duplicate last time" and R > 2:
            p[-1, 0] = p[-2, 0]
        elif rk == "all zero":
            p[:] = 0.0
        elif rk == "nan x":
            p[min(R - 1, 1 + b % 5), 2] = np.nan
        elif rk == "nan kappa":
            p[:, 5] = np.nan
        span = p[-1, 0] - p[0, 0]
        advance[b] = {"zero": 0.0, "on a knot": p[min(R - 1, 3), 0] - p[0, 0], "between knots": 0.234 * delta / DT,
                      "past the end": min(span + 0.05, 0.45), "at the limit": BATCH_MAX_ADVANCE,
                      "above the limit": np.nextafter(BATCH_MAX_ADVANCE, 1.0), "negative": -rng.uniform(1e-3, 2.0),
                      "nan": np.nan}[ak]
        plans[b] = p
        kinds.append((ak, rk))
    return plans, advance, kinds
