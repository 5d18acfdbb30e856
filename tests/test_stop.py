"""The stop rule (include/cilqr.h, "stop") on the host: the C-ABI call cilqr_stop_rows against the NumPy statement
cilqr_amd/stop.py bit for bit (a NaN matching a NaN) on the table of tests/stop_cases.py; the statement against an evaluation
in fractions where every step is exact; the geometry against the resample call at every row's station; the table's census;
every argument check.  No GPU involved: the kernel is held to the host call in tests/test_gpu_stop.py."""
from fractions import Fraction

import numpy as np
import pytest

import stop_cases as sc
from cilqr_amd import api, stop

CASES = sc.cases()


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def host(case, **over):
    a = dict(case, **over)
    return api.stop_rows(a["rows"], a["layout"], a["profiles"], a["delta_t"], a["n_out"], a["start_va"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_host_call_equals_the_numpy_statement_bit_for_bit(case):
    got, want = host(case), sc.reference(case)
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["stop_knot"], want["stop_knot"])
    assert sc.same_bits(got["travel"], want["travel"]), (got["travel"], want["travel"])
    assert sc.same_bits(got["rows"], want["rows"])
    if case["expect"] is not None:
        assert got["status"][0] == case["expect"]
    for m in range(len(case["profiles"])):
        if got["status"][m] == stop.REFUSED:
            assert not got["rows"][m].view(np.uint64).any() and got["stop_knot"][m] == -1 and got["travel"][m] == 0.0


def test_the_table_holds_every_status_and_branch():
    status = np.concatenate([sc.reference(c)["status"] for c in CASES])
    assert set(status.tolist()) == {stop.STOPPED, stop.MOVING, stop.OVERRUN, stop.REFUSED}
    assert {c["layout"] for c in CASES} == set(sc.LAYOUTS)
    assert any(c["start_va"] is not None for c in CASES) and any(c["start_va"] is None for c in CASES)
    assert {len(c["profiles"]) for c in CASES} >= {1, 2, 3, 8}
    assert {c["rows"].shape[0] for c in CASES} >= {2, 256} and {c["n_out"] for c in CASES} >= {1, 256}
    # a degenerate station pair is bracketed, a NaN is carried without reaching a row, and one reaches a row
    by_name = {c["name"]: c for c in CASES}
    plan = stop.plan_rows_of(by_name["standing_segment_layout0"]["rows"], api.ROWS_TRAJ)
    ref = sc.reference(by_name["standing_segment_layout0"])
    from cilqr_amd import resample
    branches = {resample.branch_of(plan, api.ROWS_PLAN, q, api.KEY_STATION) for q in ref["rows"][..., 1].ravel()}
    assert {"degenerate", "search", "first_pair"} <= branches, branches
    # ... and one is met only after two dozen finite rows: a kernel that works through the knots in chunks has let those go
    later = by_name["refused_nan_curvature_in_a_later_chunk"]
    keys = stop.plan_rows_of(later["rows"], later["layout"])[:, 1]
    s_k = [c[0] for c in stop.chain(keys[0], later["rows"][0, 4], later["rows"][0, 5], *later["profiles"][0], later["delta_t"], later["n_out"])]
    assert np.isnan(later["rows"][25, 7]) and min(k for k, s in enumerate(s_k) if s >= keys[24]) >= 24
    assert sc.reference(later)["status"].tolist() == [stop.REFUSED, stop.STOPPED]
    assert np.isnan(by_name["carried_nan_not_reached"]["rows"]).any()
    assert not np.isnan(sc.reference(by_name["carried_nan_not_reached"])["rows"]).any()


def exact_chain(v0, a0, a_target, jerk, delta_t, n_out):
    """the speed chain of the rule in fractions.Fraction from s = 0: the exact values, no rounding anywhere"""
    F = Fraction
    s, v, a, a_target, jerk, delta_t = F(0), F(v0), F(a0), F(a_target), F(jerk), F(delta_t)
    out = [(s, v, a)]
    for _ in range(1, n_out):
        if v == 0:
            a = F(0)
        else:
            if a > a_target:
                an = max(a + jerk * delta_t, a_target)
            elif a < a_target:
                an = min(a - jerk * delta_t, a_target)
            else:
                an = a_target
            vn = v + (F(1, 2) * delta_t) * (a + an)
            if not vn > 0:
                f = v / (v - vn)
                s, v, a = s + F(1, 2) * v * (f * delta_t), F(0), F(0)
            else:
                s, v, a = s + (F(1, 2) * delta_t) * (v + vn), vn, an
        out.append((s, v, a))
    return out


@pytest.mark.parametrize("name, travel, stop_knot", [("constant_braking", 16.0, 32), ("stop_inside_a_step", 14.0625, 8),
                                                     ("jerk_ramp", None, None), ("easing_off", None, None)])
def test_statement_is_exact_on_dyadic_inputs(name, travel, stop_knot):
    case = next(c for c in CASES if c["name"] == name)
    (a_target, jerk), v0, a0 = case["profiles"][0], case["rows"][0, 6], case["rows"][0, 7]
    want = exact_chain(v0, a0, a_target, jerk, case["delta_t"], case["n_out"])
    got = stop.stop_rows(case["rows"], case["layout"], case["profiles"][0], case["delta_t"], case["n_out"])
    for k, (s, v, a) in enumerate(want):     # float == Fraction compares exactly
        assert (got["rows"][k, 1], got["rows"][k, 6], got["rows"][k, 7]) == (s, v, a), (k, got["rows"][k], s, v, a)
        assert got["rows"][k, 2] == s and got["rows"][k, 3] == 0.0       # the straight path: x is the station
        assert got["rows"][k, 0] == Fraction(case["delta_t"]) * k
        if k + 1 < len(want):
            assert got["rows"][k, 9] == (want[k + 1][2] - a) / Fraction(case["delta_t"])
    assert got["travel"] == want[-1][0] and got["status"] == stop.STOPPED
    standing = [k for k, c in enumerate(want) if c[1] == 0]
    assert got["stop_knot"] == standing[0]
    if travel is not None:
        assert got["travel"] == travel and got["stop_knot"] == stop_knot
    assert host(case)["travel"][0] == got["travel"]
    # the ramp and the easing do change a before they hold it
    if name in ("jerk_ramp", "easing_off"):
        assert len({c[2] for c in want[:6]}) >= 5 and want[5][2] == a_target


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_geometry_is_the_resample_call_at_every_rows_station(case):
    got = host(case)
    plan = case["rows"] if case["layout"] == api.ROWS_PLAN else stop.plan_rows_of(case["rows"], case["layout"])
    for m in range(len(case["profiles"])):
        if got["status"][m] == stop.REFUSED:
            continue
        rows = got["rows"][m]
        if case["layout"] == api.ROWS_TRAJ:
            want = api.resample_rows(plan, api.ROWS_PLAN, rows[:, 1], api.KEY_STATION)
            cols = (2, 3, 4, 5, 8)
        else:
            want = api.resample_rows(case["rows"], case["layout"], rows[:, 1], api.KEY_STATION)
            cols = (2, 3, 4, 5, 8)       # x y theta kappa delta: the same columns in _PLAN and _COARSE
        assert sc.same_bits(rows[:, cols], want[:, cols]), (case["name"], m)
        # s is the chain's station clamped to the path, and after the stop the pose repeats with v = a = 0
        assert (rows[:, 1] <= plan[-1, 1]).all() and (np.diff(rows[:, 1]) >= 0).all()
        k = int(got["stop_knot"][m])
        if k >= 0:
            assert (rows[k:, 6] == 0.0).all() and (rows[k + 1:, 7] == 0.0).all()
            assert sc.same_bits(rows[k:, 1:6], np.broadcast_to(rows[k, 1:6], rows[k:, 1:6].shape))
            assert sc.same_bits(rows[k:, 8], np.broadcast_to(rows[k, 8], rows[k:, 8].shape))
            assert (rows[k + 1:, 9:11] == 0.0).all() and rows[k, 10] == 0.0
        assert (rows[-1, 9:11] == 0.0).all()
        assert got["status"][m] != stop.STOPPED or k >= 0


def test_v0_zero_repeats_row_zero():
    case = next(c for c in CASES if c["name"] == "stopped_v0_zero")
    got = host(case)
    assert got["status"][0] == stop.STOPPED and got["stop_knot"][0] == 0 and got["travel"][0] == 0.0
    assert sc.same_bits(got["rows"][0][:, 1:], np.broadcast_to(got["rows"][0][0, 1:], (case["n_out"], 10)))
    left = host(next(c for c in CASES if c["name"] == "stopped_v0_zero_a0_left"))
    assert left["rows"][0][0, 7] == -1.0 and (left["rows"][0][1:, 7] == 0.0).all() and left["rows"][0][0, 9] == 8.0


def test_start_va_replaces_row_zero_and_profiles_are_independent():
    case = next(c for c in CASES if c["name"] == "wrap_start_va_layout0")
    rows = case["rows"].copy()
    rows[0, 4:6] = case["start_va"]          # ROWS_TRAJ: v 4, a 5
    assert sc.same_bits(host(case)["rows"], host(case, rows=rows, start_va=None)["rows"])
    many = next(c for c in CASES if c["name"] == "eight_profiles")
    all_of = host(many)
    for m in (0, 3, 7):
        one = host(many, profiles=many["profiles"][m:m + 1])
        assert sc.same_bits(one["rows"][0], all_of["rows"][m]) and one["status"][0] == all_of["status"][m]
        assert one["stop_knot"][0] == all_of["stop_knot"][m] and sc.same_bits(one["travel"][0], all_of["travel"][m])


def test_every_argument_check_returns_its_code():
    case = CASES[0]
    rows, prof = case["rows"], case["profiles"]
    out = np.full((1, 4, 11), -7.0)
    status, knot, travel = np.full(1, -9, np.int32), np.full(1, -9, np.int32), np.full(1, -7.0)
    L = api.lib()

    def call(layout=api.ROWS_PLAN, rows=rows, n_knots=rows.shape[0], n_profiles=1, profiles=prof, dt=0.125, n_out=4,
             outputs=(out, status, knot, travel)):
        code = L.cilqr_stop_rows(layout, None if rows is None else rows.ctypes.data, n_knots, n_profiles,
                                 None if profiles is None else profiles.ctypes.data, None, api.C.c_double(dt), n_out,
                                 *[None if o is None else o.ctypes.data for o in outputs])
        if code != api.OK:
            assert (out == -7.0).all() and status[0] == -9 and knot[0] == -9 and travel[0] == -7.0
        return code

    assert call(rows=None) == api.ERR_NULL and call(profiles=None) == api.ERR_NULL
    assert call(layout=3) == api.ERR_ARG and call(layout=api.ROWS_POINTS) == api.ERR_ARG and call(layout=-1) == api.ERR_ARG
    assert call(n_knots=1) == api.ERR_ARG and call(n_out=0) == api.ERR_ARG
    assert call(n_profiles=0) == api.ERR_ARG and call(n_profiles=api.STOP_MAX_PROFILES + 1, profiles=np.tile(prof, (9, 1))) == api.ERR_ARG
    for bad in ((0.5, -1.0), (-1.0, 0.0), (-1.0, 1.0), (np.nan, -1.0), (-1.0, np.nan), (-np.inf, -1.0), (-1.0, -np.inf)):
        assert call(profiles=np.array([bad])) == api.ERR_ARG, bad
    for bad in (0.0, -0.1, np.nan):
        assert call(dt=bad) == api.ERR_ARG, bad
    assert call(outputs=(None, None, None, None)) == api.ERR_ARG
    big = np.zeros((api.DP_MAX_KNOTS + 1, 11))
    assert call(rows=big, n_knots=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    assert call(n_out=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    assert call(profiles=np.array([[0.0, -1.0]])) == api.OK          # a_target = 0 is inside the domain: coast at the jerk's end
    for keep in range(4):        # every output alone
        outs = [o if i == keep else None for i, o in enumerate((out, status, knot, travel))]
        assert call(outputs=outs) == api.OK
    want = api.stop_rows(rows, api.ROWS_PLAN, prof, 0.125, 4)
    assert sc.same_bits(out, want["rows"]) and status[0] == want["status"][0] and knot[0] == want["stop_knot"][0]
    assert travel[0] == want["travel"][0]
