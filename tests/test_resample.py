"""Resampling of trajectory rows on the host (cilqr_resample_rows, include/cilqr/trajectory_queries.hpp):
DiscretizedTrajectory::EvaluateTime / EvaluateStation of the reference.  Held against the reference's own class where it
builds (the seven columns it defines, bit for bit), against the NumPy statement cilqr_amd/resample.py on all columns, and
on crafted trajectories whose branches are counted (tests/resample_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_cases as rc
from cilqr_amd import api, resample
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def crafted():
    return rc.crafted_cases()


@pytest.fixture(scope="module")
def randoms():
    return rc.random_cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(orc.ref_lib() is None, reason="oracle/_ref/libcilqr_ref.so is not built (no reference tree here)")
def test_host_call_and_numpy_statement_equal_the_reference_class(crafted, randoms):
    """time, s, x, y, theta, kappa, velocity of DiscretizedTrajectory::EvaluateTime / EvaluateStation, bit for bit (a NaN
    matching a NaN), for the crafted table and 300 random trajectories; the rows go into the shim's nine columns with both
    bounds 0.  ROWS_COARSE carries exactly those seven columns first, ROWS_PLAN too."""
    REF = orc.ref_lib()
    checked = 0
    for case in crafted + randoms:
        if not case.monotone:
            continue
        nine = np.ascontiguousarray(np.concatenate([case.plan[:, :7], np.zeros((len(case.plan), 2))], axis=1))
        for key, fn in ((api.KEY_TIME, REF.ref_trajectory_evaluate_time), (api.KEY_STATION, REF.ref_trajectory_evaluate_station)):
            want = np.full((len(case.queries), 9), -7.0)
            for m, q in enumerate(case.queries):
                fn(nine.ctypes.data_as(C.c_void_p), len(nine), float(q), want[m].ctypes.data_as(C.c_void_p))
            for layout in (api.ROWS_PLAN, api.ROWS_COARSE):
                rows = rc.rows_in_layout(layout, case.plan)
                got = api.resample_rows(rows, layout, case.queries, key)
                stated = resample.resample_rows(rows, layout, case.queries, key)
                assert rc.same_rows(got[:, :7], want[:, :7]), (case.name, key, layout, got[:, :7], want[:, :7])
                assert rc.same_rows(stated[:, :7], want[:, :7]), (case.name, key, layout)
                checked += got.shape[0]
        # ROWS_TRAJ (time only): the same seven quantities in its own column order
        rows = rc.rows_in_layout(api.ROWS_TRAJ, case.plan)
        got = api.resample_rows(rows, api.ROWS_TRAJ, case.queries, api.KEY_TIME)
        want = np.full((len(case.queries), 9), -7.0)
        for m, q in enumerate(case.queries):
            REF.ref_trajectory_evaluate_time(nine.ctypes.data_as(C.c_void_p), len(nine), float(q), want[m].ctypes.data_as(C.c_void_p))
        # s is not a column of ROWS_TRAJ: time x y theta v kappa against plan columns 0 2 3 4 6 5
        assert rc.same_rows(got[:, [0, 1, 2, 3, 4, 7]], want[:, [0, 2, 3, 4, 6, 5]]), case.name
    assert checked > 10000


# ---------------------------------------------------------------------------------------------------------------------
# 2. the NumPy statement, all columns, every layout and key
# ---------------------------------------------------------------------------------------------------------------------
def test_host_call_equals_the_numpy_statement_in_every_layout_and_key(crafted, randoms):
    for case in crafted + randoms[:120]:
        for layout in rc.LAYOUTS:
            rows = rc.rows_in_layout(layout, case.plan)
            for key in rc.KEYS_OF[layout]:
                got = api.resample_rows(rows, layout, case.queries, key)
                want = resample.resample_rows(rows, layout, case.queries, key)
                assert rc.same_rows(got, want), (case.name, layout, key, got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the crafted table
# ---------------------------------------------------------------------------------------------------------------------
def test_crafted_table_reaches_every_branch(crafted):
    names = [c.name for c in crafted]
    for needed in ("query equal to a key", "query equal to the first key", "query equal to the last key",
                   "before the first and past the last key", "duplicate keys", "keys 5e-11 apart", "keys exactly 1e-10 apart",
                   "headings either side of pi", "unwrapped headings near 3 pi", "two knots", "NaN query", "NaN row",
                   "non-monotone keys"):
        assert needed in names, needed
    seen = rc.census(crafted)
    assert all(seen[b] >= 1 for b in rc.BRANCHES), seen
    for case in crafted:     # ... and every case reaches the branches it was written for
        mine = {resample.branch_of(case.plan, api.ROWS_PLAN, q) for q in case.queries}
        assert set(case.branches) <= mine, (case.name, case.branches, mine)


def test_crafted_values_follow_from_the_rule(crafted):
    by_name = {c.name: c for c in crafted}
    P = api.ROWS_PLAN
    for key in (api.KEY_TIME, api.KEY_STATION):
        kc = 0 if key == api.KEY_TIME else 1
        # a query on a key: w = 1 on the pair below it, so the linear columns are p1's values ((1 - 1) p0 + 1 p1)
        c = by_name["query equal to a key"]
        out = api.resample_rows(c.plan, P, c.queries[:2], key)
        for o, i in zip(out, (3, 7)):
            assert o[kc] == c.plan[i, kc] and np.array_equal(o[[2, 3, 5, 6, 7, 8]], 0.0 * c.plan[i - 1, [2, 3, 5, 6, 7, 8]] + c.plan[i, [2, 3, 5, 6, 7, 8]])
            assert np.array_equal(_bits(o[9:]), _bits(c.plan[i - 1, 9:]))         # the controls of the step that ends there
        # the first key: pair (0, 1), w = 0
        c = by_name["query equal to the first key"]
        o = api.resample_rows(c.plan, P, c.queries, key)[0]
        assert np.array_equal(o[[2, 3, 5, 6, 7, 8]], c.plan[0, [2, 3, 5, 6, 7, 8]] + 0.0 * c.plan[1, [2, 3, 5, 6, 7, 8]])
        assert np.array_equal(_bits(o[9:]), _bits(c.plan[0, 9:]))
        # the last key: pair (K-2, K-1), w = 1
        c = by_name["query equal to the last key"]
        o = api.resample_rows(c.plan, P, c.queries, key)[0]
        assert np.array_equal(o[[2, 3]], 0.0 * c.plan[-2, [2, 3]] + c.plan[-1, [2, 3]]) and np.array_equal(_bits(o[9:]), _bits(c.plan[-2, 9:]))
        # outside the range: extrapolation along the end pairs
        c = by_name["before the first and past the last key"]
        out = api.resample_rows(c.plan, P, c.queries, key)
        w = (c.queries[0] - c.plan[0, kc]) / (c.plan[1, kc] - c.plan[0, kc])
        assert w < 0 and out[0, 2] == (1 - w) * c.plan[0, 2] + w * c.plan[1, 2]
        w = (c.queries[3] - c.plan[-2, kc]) / (c.plan[-1, kc] - c.plan[-2, kc])
        assert w > 1 and out[3, 2] == (1 - w) * c.plan[-2, 2] + w * c.plan[-1, 2]
        # duplicates and keys 5e-11 apart: p0 as bits, key column included
        c = by_name["duplicate keys"]
        o = api.resample_rows(c.plan, P, c.queries[:1], key)[0]       # lower bound of 0.2 is row 2: pair (1, 2), not degenerate
        assert o[kc] == 0.2 and np.array_equal(_bits(o[9:]), _bits(c.plan[1, 9:]))
        o = api.resample_rows(c.plan, P, [np.nextafter(0.2, 1.0)], key)[0]     # lower bound is row 5: pair (4, 5)
        assert np.array_equal(_bits(o[9:]), _bits(c.plan[4, 9:]))
        c = by_name["duplicate keys at both ends"]
        out = api.resample_rows(c.plan, P, c.queries, key)
        assert np.array_equal(_bits(out[0]), _bits(c.plan[0])) and np.array_equal(_bits(out[1]), _bits(c.plan[0]))
        assert np.array_equal(_bits(out[2]), _bits(c.plan[3])) and np.array_equal(_bits(out[3]), _bits(c.plan[3]))
        c = by_name["keys 5e-11 apart"]
        out = api.resample_rows(c.plan, P, c.queries[:2], key)
        assert np.array_equal(_bits(out[0]), _bits(c.plan[1])) and np.array_equal(_bits(out[1]), _bits(c.plan[1]))
        # exactly 1e-10 apart: interpolated (the key column is the query), theta by slerp's own `<=`: NormalizeAngle(p0.theta)
        c = by_name["keys exactly 1e-10 apart"]
        out = api.resample_rows(c.plan, P, c.queries[:1], key)
        assert out[0, kc] == 5e-11 and out[0, 2] == (1 - 0.5) * c.plan[1, 2] + 0.5 * c.plan[2, 2]
        assert out[0, 4] == resample.normalize_angle(c.plan[1, 4])
        # headings: the short way round
        for name in ("headings either side of pi", "headings either side of -pi"):
            c = by_name[name]
            out = api.resample_rows(c.plan, P, c.queries, key)
            for o in out:
                i = resample.bracket(c.plan[:, kc], o[kc])
                a0, a1 = c.plan[i - 1, 4], c.plan[i, 4]
                short = abs(resample.normalize_angle(a1 - a0))
                assert -np.pi <= o[4] < np.pi and abs(resample.normalize_angle(o[4] - a0)) <= short + 1e-12
        c = by_name["unwrapped headings near 3 pi"]
        out = api.resample_rows(c.plan, P, c.queries, key)
        assert np.all(np.abs(np.abs(out[:, 4]) - np.pi) < 0.2)        # 3 pi +- 0.06 comes out next to +-pi
        # K = 2
        c = by_name["two knots"]
        out = api.resample_rows(c.plan, P, c.queries, key)
        assert np.array_equal(out[:, kc], c.queries) and out[2, 2] == (1 - (4.2 - 4.0) / (4.5 - 4.0)) * c.plan[0, 2] + ((4.2 - 4.0) / (4.5 - 4.0)) * c.plan[1, 2]
        # a NaN query: pair (0, 1); everything computed is NaN, the controls are p0's
        c = by_name["NaN query"]
        out = api.resample_rows(c.plan, P, c.queries, key)
        assert np.isnan(out[0, :9]).all() and np.array_equal(_bits(out[0, 9:]), _bits(c.plan[0, 9:])) and np.isfinite(out[1]).all()
        # a NaN row spoils the two steps it bounds and nothing else
        c = by_name["NaN row"]
        out = api.resample_rows(c.plan, P, c.queries[:4], key)
        assert np.isfinite(out[0]).all() and np.isfinite(out[3]).all()
        # a and delta follow the linear form, the controls never
        c = by_name["headings either side of pi"]
        out = api.resample_rows(c.plan, P, c.queries, key)
        for o in out:
            i = resample.bracket(c.plan[:, kc], o[kc])
            w = (o[kc] - c.plan[i - 1, kc]) / (c.plan[i, kc] - c.plan[i - 1, kc])
            assert o[7] == (1 - w) * c.plan[i - 1, 7] + w * c.plan[i, 7] and o[8] == (1 - w) * c.plan[i - 1, 8] + w * c.plan[i, 8]
            assert np.array_equal(_bits(o[9:]), _bits(c.plan[i - 1, 9:]))


def test_copied_values_keep_their_bits():
    """a NaN with a payload, a negative zero and a denormal in the controls and in a degenerate pair come out as they went in"""
    rng = np.random.default_rng(5)
    plan = rc.smooth_plan(rng, [0.0, 0.1, 0.1, 0.2])
    odd = np.array([0x7FF800000000BEEF, 0xFFF0000000000001, 0x8000000000000000, 0x0000000000000001], dtype=np.uint64).view(np.float64)
    plan[0, 9], plan[0, 10], plan[1, 9], plan[1, 10] = odd
    plan[1, 2], plan[1, 4] = odd[0], odd[1]
    for layout in (api.ROWS_PLAN, api.ROWS_TRAJ):
        rows = rc.rows_in_layout(layout, plan)
        for fn in (api.resample_rows, resample.resample_rows):
            out = fn(rows, layout, [0.05, 0.1], api.KEY_TIME)
            assert np.array_equal(_bits(out[0, -2:]), _bits(rows[0, -2:])), (layout, fn)
            out = fn(rows, layout, [0.15], api.KEY_TIME)       # lower bound of 0.15 is row 3: pair (2, 3)
            assert np.array_equal(_bits(out[0, -2:]), _bits(rows[2, -2:]))
            out = fn(rows, layout, [np.nextafter(0.1, 1.0)], api.KEY_TIME)
            assert np.array_equal(_bits(out[0, -2:]), _bits(rows[2, -2:]))
    plan3 = rc.smooth_plan(rng, [0.1, 0.1, 0.2])               # query below the range: pair (0, 1), degenerate: row 0 as bits
    plan3[0, 2:] = plan[1, 2:]
    for layout in rc.LAYOUTS:
        rows = rc.rows_in_layout(layout, plan3)
        for fn in (api.resample_rows, resample.resample_rows):
            out = fn(rows, layout, [-4.0, 0.1], api.KEY_TIME)
            assert np.array_equal(_bits(out[0]), _bits(rows[0])) and np.array_equal(_bits(out[1]), _bits(rows[0]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_host_call():
    L = api.lib()
    rng = np.random.default_rng(3)
    plan = rc.smooth_plan(rng, np.arange(api.DP_MAX_KNOTS + 1) * 0.1)
    q = np.array([0.05, 0.15])

    def call(layout=api.ROWS_PLAN, n_knots=5, key=api.KEY_TIME, n_queries=2, rows=True, queries=True, out=True, alias=False):
        r = rc.rows_in_layout(layout if layout in rc.LAYOUTS else api.ROWS_PLAN, plan)
        o = np.full((max(n_queries, 1), 11), -7.0)
        code = L.cilqr_resample_rows(layout, r.ctypes.data if rows else None, n_knots, key, q.ctypes.data if queries else None,
                                     n_queries, (r.ctypes.data if alias else o.ctypes.data) if out else None)
        if code != api.OK:      # nothing was written
            assert (o == -7.0).all()
        return code

    assert call() == api.OK
    for what in ("rows", "queries", "out"):
        assert call(**{what: False}) == api.ERR_NULL, what
    assert call(n_knots=1) == api.ERR_ARG and call(n_knots=0) == api.ERR_ARG and call(n_knots=-3) == api.ERR_ARG
    assert call(n_queries=0) == api.ERR_ARG and call(n_queries=-1) == api.ERR_ARG
    assert call(layout=3) == api.ERR_ARG and call(layout=-1) == api.ERR_ARG and call(layout=api.ROWS_CONTROLS) == api.ERR_ARG
    assert call(key=2) == api.ERR_ARG and call(key=-1) == api.ERR_ARG
    assert call(layout=api.ROWS_TRAJ, key=api.KEY_STATION) == api.ERR_ARG
    assert call(layout=api.ROWS_COARSE, key=api.KEY_STATION) == api.OK and call(layout=api.ROWS_TRAJ) == api.OK
    assert call(alias=True) == api.ERR_ARG
    assert call(n_knots=2) == api.OK
    assert call(n_knots=api.DP_MAX_KNOTS) == api.OK and call(n_knots=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    with pytest.raises(api.CilqrError) as e:
        api.resample_rows(plan[:1], api.ROWS_PLAN, q)
    assert e.value.code == api.ERR_ARG
    with pytest.raises(ValueError):
        resample.resample_rows(rc.rows_in_layout(api.ROWS_TRAJ, plan), api.ROWS_TRAJ, q, api.KEY_STATION)


# ---------------------------------------------------------------------------------------------------------------------
# 5. sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_crafted_cases_under_address_and_undefined_behaviour_sanitizers(crafted, randoms, tmp_path):
    """tests/cpp/trajectory_queries_test.cc -- a program of its own around include/cilqr/trajectory_queries.hpp -- built
    with -fsanitize=address,undefined and run as a child process on the crafted cases (and forty random ones) in every
    layout and key; what it compares against are the NumPy statement's rows."""
    exe = tmp_path / "trajectory_queries_test"
    # (the runtimes linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "trajectory_queries_test.cc"), "-o", str(exe)])
    cases = crafted + randoms[:40]
    n_rows = sum(len(c.queries) for c in cases)
    for layout in rc.LAYOUTS:
        for key in rc.KEYS_OF[layout]:
            path = tmp_path / f"cases_{layout}_{key}.bin"
            rc.write_cases(path, cases, layout, key)
            run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
            assert run.returncode == 0, run.stdout + run.stderr
            assert run.stdout.strip() == f"{len(cases)} cases, {n_rows} rows, 0 failures"
