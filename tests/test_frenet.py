"""The Frenet frame of a centre line on the host (cilqr_frenet_rows / cilqr_cartesian_points,
include/cilqr/trajectory_queries.hpp): DiscretizedTrajectory::GetProjection / GetCartesian of the reference.  Held against
the reference's own class where it builds (all eight and two outputs, bit for bit), against the NumPy statement
cilqr_amd/frenet.py in every layout, and on crafted centre lines whose branches are counted (tests/frenet_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frenet_cases as fc
from resample_cases import same_rows
from cilqr_amd import api, frenet, resample
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def crafted():
    return fc.crafted_cases()


@pytest.fixture(scope="module")
def randoms():
    return fc.random_cases()


@pytest.fixture(scope="module")
def inverses():
    return fc.inverse_cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference itself
# ---------------------------------------------------------------------------------------------------------------------
def _shim_rows(center):
    """centre rows in the shim's nine columns: time s x y theta kappa velocity left_bound right_bound, time = velocity = 0"""
    nine = np.zeros((len(center), 9))
    nine[:, 1:6] = center[:, 0:5]
    nine[:, 7:9] = center[:, 5:7]
    return np.ascontiguousarray(nine)


@pytest.mark.skipif(orc.ref_lib() is None, reason="oracle/_ref/libcilqr_ref.so is not built (no reference tree here)")
def test_host_calls_equal_the_reference_class(crafted, randoms, inverses):
    """station, lateral (its sign included) and the projected point's x, y, theta, kappa, left_bound, right_bound of
    DiscretizedTrajectory::GetProjection, and x, y of GetCartesian, bit for bit (a NaN matching a NaN) for the crafted
    table and 300 random lines of 2, 3, 10, 60 and 250 points with 50 points each."""
    REF = orc.ref_lib()
    checked = 0
    for case in crafted + randoms:
        nine = _shim_rows(case.center)
        want = np.full((len(case.points), 8), -7.0)
        for m, (px, py) in enumerate(case.points.tolist()):
            sl, pp = np.full(2, -7.0), np.full(9, -7.0)
            REF.ref_trajectory_projection(_p(nine), len(nine), px, py, _p(sl), _p(pp))
            assert same_rows(pp[[0, 6]], np.zeros(2)) or np.isnan(pp[[0, 6]]).any(), case.name      # time, velocity
            want[m, :2], want[m, 2:6], want[m, 6:] = sl, pp[2:6], pp[7:9]
            assert same_rows(sl[:1], pp[1:2]), case.name
        got = api.frenet_rows(case.center, case.points)
        _, cross, _ = frenet.frenet_rows(case.center, case.points)
        assert fc.same_frenet(got, want, cross), (case.name, got, want)
        checked += len(got)
    assert checked > 15000
    pairs = 0
    for v in inverses + [fc.Inverse(c.name, c.center, np.stack([np.linspace(-2.0, c.center[-1, 0] + 2.0, 9), np.linspace(-3, 3, 9)], 1))
                         for c in randoms[:100]]:
        nine = _shim_rows(v.center)
        want = np.full((len(v.sl), 2), -7.0)
        for m, (st, lat) in enumerate(v.sl.tolist()):
            REF.ref_trajectory_cartesian(_p(nine), len(nine), st, lat, _p(want[m]))
        got = api.cartesian_points(v.center, v.sl)
        assert same_rows(got[:, :2], want), (v.name, got, want)
        pairs += len(got)
    assert pairs > 1500


# ---------------------------------------------------------------------------------------------------------------------
# 2. the NumPy statement, every layout
# ---------------------------------------------------------------------------------------------------------------------
def test_host_calls_equal_the_numpy_statements_in_every_layout(crafted, randoms, inverses):
    rng = np.random.default_rng(4)
    for case in crafted + randoms[:120]:
        want, cross, _ = frenet.frenet_rows(case.center, case.points)
        for layout in fc.LAYOUTS:
            got = api.frenet_rows(case.center, fc.rows_in_layout(layout, case.points, rng), layout)
            assert fc.same_frenet(got, want, cross), (case.name, layout, got, want)
    for v in inverses:
        got, want = api.cartesian_points(v.center, v.sl), frenet.cartesian_points(v.center, v.sl)
        assert same_rows(got, want), (v.name, got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the crafted table
# ---------------------------------------------------------------------------------------------------------------------
def test_crafted_table_reaches_every_branch(crafted):
    names = [c.name for c in crafted]
    for needed in ("two centre points", "three centre points", "a line past one tile", "a line past two tiles",
                   "duplicated centre points", "degenerate pair", "stations exactly 1e-10 apart", "coincident pair",
                   "headings either side of pi", "unwrapped headings", "NaN row in the centre line"):
        assert needed in names, needed
    seen = fc.census(crafted)
    assert all(seen[b] >= 1 for b in fc.BRANCHES), seen
    for case in crafted:     # ... and every case reaches the branches it was written for
        mine = set().union(*(frenet.branch_of(case.center, px, py) for px, py in case.points.tolist()))
        assert set(case.branches) <= mine, (case.name, case.branches, mine)
        _, _, dist = frenet.frenet_rows(case.center, case.points)
        assert int(np.count_nonzero(dist == 0.0)) == case.on_line, (case.name, dist)


def test_the_tile_size_of_the_cases_is_the_kernels():
    hpp = open(os.path.join(ROOT, "cilqr_amd", "csrc", "frenet.hpp")).read()
    assert int(re.search(r"kFrTile = (\d+);", hpp).group(1)) == fc.TILE
    lanes, wide = (int(re.search(rf"{k} = (\d+);", hpp).group(1)) for k in ("kFrLanes", "kFrWide"))
    assert lanes * 4 * 64 * wide == fc.WIDE_FROM and "(size_t)256 * 4 * 64 * kFrWide" in hpp


def test_crafted_values_follow_from_the_rule(crafted):
    by_name = {c.name: c for c in crafted}
    # a straight dyadic line: station and offset are exact
    c = by_name["nine centre points"]
    q = {name: i for i, (name, *_rest) in enumerate(fc.line_queries(c.center))}
    out = api.frenet_rows(c.center, c.points)
    x0, y0, step, last = c.center[0, 1], c.center[0, 2], 0.5, c.center[-1]
    o = out[q["before the first point"]]          # pair (0, 1), w = -2.5: extrapolated
    assert o[0] == -2.5 * step and o[1] == 0.5 and o[2] == x0 - 2.5 * step and o[3] == y0
    assert o[6] == (1 - -2.5) * c.center[0, 5] + -2.5 * c.center[1, 5]
    o = out[q["beyond the last point"]]           # pair (n-2, n-1), w = 4.25
    assert o[0] == last[0] + 3.25 * step and o[1] == -0.75 and o[7] == (1 - 4.25) * c.center[-2, 6] + 4.25 * last[6]
    for name in ("on a centre point", "on a chord", "on the first point", "on the last point"):
        assert out[q[name], 1] == 0.0 and np.array_equal(out[q[name], 2:4], c.points[q[name]]), name
    # a tie: the FIRST of the two points is `at`, so the pair is (at-1, at+1) around it -- the bounds show which
    mid = len(c.center) // 2
    o = out[q["tie of two points"]]
    i0, i1 = mid - 2, mid
    w = (o[0] - c.center[i0, 0]) / (c.center[i1, 0] - c.center[i0, 0])
    assert w == 0.75 and o[1] == 0.75 and o[6] == (1 - w) * c.center[i0, 5] + w * c.center[i1, 5]
    assert o[6] != 0.25 * c.center[mid - 1, 5] + 0.75 * c.center[mid + 1, 5]      # what the second of the two would give
    o = out[q["tie of the first two points"]]     # at = 0: pair (0, 1)
    assert o[0] == 0.5 * step and o[1] == -0.25
    o = out[q["tie of the last two points"]]      # at = n-2: pair (n-3, n-1), w = 0.75
    assert o[6] == (1 - 0.75) * c.center[-3, 5] + 0.75 * last[5]
    # NaN and infinite queries: no distance is below DBL_MAX, at = 0, pair (0, 1); the arithmetic decides
    for name in ("NaN x", "NaN y", "infinite x", "infinite x and y", "infinite y"):
        assert not np.isfinite(out[q[name], :2]).any(), name
    assert np.isfinite(out[q["far away"]]).all()
    # the tie at a tile edge: at = TILE - 1
    c = by_name["a line past one tile"]
    q = {name: i for i, (name, *_rest) in enumerate(fc.line_queries(c.center))}
    o = api.frenet_rows(c.center, c.points)[q[f"tie across tile edge {fc.TILE}"]]
    assert o[0] == fc.TILE - 0.5 and o[6] == 0.25 * c.center[fc.TILE - 2, 5] + 0.75 * c.center[fc.TILE, 5]
    # duplicated points: the first of them is `at`
    c = by_name["duplicated centre points"]
    o = api.frenet_rows(c.center, c.points[:1])[0]               # at = 4: pair (3, 5), and row 5 is row 4
    assert o[0] == 4.0 and o[6] == 0.0 * c.center[3, 5] + 1.0 * c.center[5, 5]
    # a degenerate pair: row at-1 as bits, headings unwrapped and a negative zero included
    c = by_name["degenerate pair"]
    out = api.frenet_rows(c.center, c.points)
    for o in out:
        assert np.array_equal(_bits(o[[0, 2, 3, 4, 5, 6, 7]]), _bits(c.center[4])), o
    assert out[0, 1] == -np.hypot(1.0, 0.5) and out[2, 1] == 0.875      # theta = 3 pi + 0.01: row 4 says the line runs the other way
    # stations exactly 1e-10 apart: interpolated, theta by slerp's own `<=`
    c = by_name["stations exactly 1e-10 apart"]
    o = api.frenet_rows(c.center, c.points[:1])[0]
    assert o[0] == 0.0 + 1.0 and o[4] == resample.normalize_angle(c.center[1, 3]) and np.isfinite(o).all()
    # coincident pair: 0 / 0
    c = by_name["coincident pair"]
    assert np.isnan(api.frenet_rows(c.center, c.points)).all()
    # a NaN row: queries whose pair holds it are NaN, the others finite
    c = by_name["NaN row in the centre line"]
    out = api.frenet_rows(c.center, c.points)
    assert np.isnan(out[:3, 0]).all() and np.isfinite(out[-2:]).all()
    # headings: the projected heading lies between the pair's, the short way round
    for name in ("headings either side of pi", "unwrapped headings"):
        c = by_name[name]
        out = api.frenet_rows(c.center, c.points)
        assert (-np.pi <= out[:, 4]).all() and (out[:, 4] < np.pi).all() and (np.abs(np.abs(out[:, 4]) - np.pi) < 0.6).all(), name


def test_inverse_values_follow_from_the_rule(inverses):
    v = {i.name: i for i in inverses}["dyadic"]
    out = api.cartesian_points(v.center, v.sl)
    for (st, lat), o in zip(v.sl.tolist(), out):
        if np.isfinite(st) and np.isfinite(lat):      # heading 0: x = station, y = lateral, also outside the line
            assert o[0] == st and o[1] == lat and o[2] == 0.0, (st, lat, o)
        elif np.isfinite(st):
            assert o[0] == st or np.isnan(o[0])       # NaN * sin(0) = NaN
            assert np.isnan(o[1]) and o[2] == 0.0
        else:
            assert not np.isfinite(o[:2]).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. round trip on the generator's road
# ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_on_the_road_is_the_numpy_statements():
    """2000 points within the road's bounds -> (station, lateral) -> back: the distance to the original point is whatever
    the rule gives (the projected heading is interpolated, so it is small, not zero); the C-ABI's and the NumPy
    statement's are the same numbers"""
    center = fc.road_center()
    pts = fc.points_on_road(np.random.default_rng(21), center, 2000, half_width=2.0)
    fr = api.frenet_rows(center, pts)
    back = api.cartesian_points(center, fr[:, :2])
    stated, _, _ = frenet.frenet_rows(center, pts)
    stated_back = frenet.cartesian_points(center, stated[:, :2])
    assert same_rows(fr, stated) and same_rows(back, stated_back)
    d, d_stated = np.hypot(*(back[:, :2] - pts).T), np.hypot(*(stated_back[:, :2] - pts).T)
    assert np.array_equal(_bits(d), _bits(d_stated))
    assert (np.abs(fr[:, 1]) <= 2.0 + 1e-9).all() and (fr[:, 6] - fr[:, 1] > 0).all() and (fr[:, 1] + fr[:, 7] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_host_calls():
    L = api.lib()
    center = fc.dyadic_line(9)
    pts = np.random.default_rng(3).uniform(0, 8, (5, 2))

    def project(layout=api.ROWS_PLAN, n_center=9, n_rows=5, want_center=True, want_rows=True, want_out=True, alias=None):
        rows = fc.rows_in_layout(layout if layout in fc.LAYOUTS else api.ROWS_PLAN, pts)
        big = np.full(5 * 11 + 5 * 8, -7.0)      # out overlapping the rows: both inside one block
        out = np.full((5, 8), -7.0)
        o = out.ctypes.data
        if alias == "rows":
            big[:rows.size] = rows.ravel()
            r, o = big.ctypes.data, big.ctypes.data + 8 * (rows.size - 1)       # the last double of rows
        else:
            r = rows.ctypes.data
        if alias == "center":
            o = center.ctypes.data + 8
        before = center.copy()
        code = L.cilqr_frenet_rows(center.ctypes.data if want_center else None, n_center, layout, r if want_rows else None, n_rows,
                                   o if want_out else None)
        if code != api.OK:      # nothing was written
            assert (out == -7.0).all() and np.array_equal(center, before) and (big[rows.size:] == -7.0).all()
        return code

    assert project() == api.OK
    for what in ("want_center", "want_rows", "want_out"):
        assert project(**{what: False}) == api.ERR_NULL, what
    for bad in (dict(n_center=1), dict(n_center=0), dict(n_center=-4), dict(n_rows=0), dict(n_rows=-1), dict(layout=3), dict(layout=5),
                dict(layout=-1), dict(alias="rows"), dict(alias="center")):
        assert project(**bad) == api.ERR_ARG, bad
    for layout in fc.LAYOUTS:
        assert project(layout=layout) == api.OK and project(layout=layout, n_center=2, n_rows=1) == api.OK

    sl = np.array([[1.0, 0.5], [2.0, -0.5], [9.0, 0.0]])

    def inverse(n_center=9, n=3, want_center=True, want_sl=True, want_out=True, alias=None):
        out = np.full((3, 3), -7.0)
        block = np.full(6 + 9, -7.0)
        block[:6] = sl.ravel()
        o = out.ctypes.data
        if alias == "sl":
            o = block.ctypes.data + 8 * 5
        elif alias == "center":
            o = center.ctypes.data + 8 * (center.size - 1)
        before = center.copy()
        code = L.cilqr_cartesian_points(center.ctypes.data if want_center else None, n_center,
                                        (block.ctypes.data if alias == "sl" else sl.ctypes.data) if want_sl else None, n,
                                        o if want_out else None)
        if code != api.OK:
            assert (out == -7.0).all() and np.array_equal(center, before) and (block[6:] == -7.0).all()
        return code

    assert inverse() == api.OK and inverse(n_center=2, n=1) == api.OK
    for what in ("want_center", "want_sl", "want_out"):
        assert inverse(**{what: False}) == api.ERR_NULL, what
    for bad in (dict(n_center=1), dict(n_center=-1), dict(n=0), dict(n=-2), dict(alias="sl"), dict(alias="center")):
        assert inverse(**bad) == api.ERR_ARG, bad
    with pytest.raises(api.CilqrError) as e:
        api.frenet_rows(center[:1], pts)
    assert e.value.code == api.ERR_ARG
    with pytest.raises(ValueError):
        api.frenet_rows(center, fc.rows_in_layout(api.ROWS_PLAN, pts), api.ROWS_TRAJ)
    with pytest.raises(ValueError):
        frenet.frenet_rows(center[:1], pts)


def test_points_layout_is_refused_by_resample_and_the_audit():
    L = api.lib()
    rows, q, out = np.zeros((5, 11)), np.array([0.05]), np.zeros((1, 11))
    assert L.cilqr_resample_rows(api.ROWS_POINTS, rows.ctypes.data, 5, api.KEY_TIME, q.ctypes.data, 1, out.ctypes.data) == api.ERR_ARG
    import collision_cases as cc
    from cilqr_amd import scene_io
    flat = scene_io.flatten_scene(cc.straight_center(length=20.0), scene_io.Scene(np.zeros(4), np.zeros((1, 6)), [], []))
    with pytest.raises(api.CilqrError) as e:
        api.check_collisions(flat, np.zeros((5, 2)), api.ROWS_POINTS)
    assert e.value.code == api.ERR_ARG


def test_the_four_calls_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    L = api.lib()
    for name in ("cilqr_frenet_rows", "cilqr_cartesian_points", "cilqr_frenet_rows_batch", "cilqr_cartesian_points_batch"):
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in api.EXPORTS and hasattr(L, name), name
    assert int(re.search(r"#define CILQR_ROWS_POINTS (\d+)", hdr).group(1)) == api.ROWS_POINTS
    assert int(re.search(r"#define CILQR_FRENET_FIELDS (\d+)", hdr).group(1)) == api.FRENET_FIELDS == frenet.FRENET_FIELDS
    assert int(re.search(r"#define CILQR_ABI_VERSION (\d+)", hdr).group(1)) == api.ABI_VERSION == 7


# ---------------------------------------------------------------------------------------------------------------------
# 6. sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_crafted_cases_under_address_and_undefined_behaviour_sanitizers(crafted, randoms, inverses, tmp_path):
    """tests/cpp/frenet_test.cc -- a program of its own around include/cilqr/trajectory_queries.hpp -- built with
    -fsanitize=address,undefined and run as a child process on the crafted cases (and forty random ones) in every layout;
    what it compares against are the NumPy statements' rows."""
    exe = tmp_path / "frenet_test"
    # (the runtimes linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "frenet_test.cc"), "-o", str(exe)])
    cases = crafted + randoms[:40]
    n_rows = sum(len(c.points) for c in cases) + sum(len(v.sl) for v in inverses)
    for layout in fc.LAYOUTS:
        path = tmp_path / f"cases_{layout}.bin"
        fc.write_cases(path, cases, layout, inverses)
        run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout.strip() == f"{len(cases)} cases, {len(inverses)} inverses, {n_rows} rows, 0 failures"
