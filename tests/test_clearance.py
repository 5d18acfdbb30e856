"""Clearance on the host (cilqr_clearance_rows, DpEnvironment::Clearance in include/cilqr/dp_planner.hpp):
Polygon2d::DistanceTo(Vec2d) of the reference from the two vehicle discs to every obstacle of the scene, for every knot of
a trajectory.  Held against the reference's own classes where they build, against the NumPy restatement
scene_io.environment_clearance bit for bit, and on a crafted table whose values follow from its construction
(tests/clearance_cases.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import clearance_cases as cl
import collision_cases as cc
from cilqr_amd import api, scene_io
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE)


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def crafted():
    return cl.crafted_cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    """(clearance, nearest, min_clearance, min_knot) of two evaluations, bit for bit"""
    return (np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
            and _bits([got[2]])[0] == _bits([want[2]])[0] and got[3] == want[3])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(orc.ref_lib() is None, reason="oracle/_ref/libcilqr_ref.so is not built (no reference tree here)")
def test_columns_are_the_reference_classes_distances():
    """Static and dynamic columns against the reference's pieces composed as Polygon2d::DistanceTo composes them:
    ref_polygon_point_in decides 0, otherwise the std::min of ref_segment_distance over the edges of the vertex array,
    reversed by the reference's area sum.  The scenes of test_polygon_bits_are_the_reference_classes_verdicts: 40 scenes x
    50 poses, polygons of 3-8 vertices, concave, clockwise and 10 m ones; both sides run on the host's libm, so the values
    are held bit for bit, `nearest` included."""
    import limit_scenes
    REF = orc.ref_lib()
    REF.ref_segment_distance.restype = C.c_double
    REF.ref_segment_distance.argtypes = [C.c_void_p, C.c_double, C.c_double]
    REF.ref_polygon_point_in.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
    cfg = api.default_dp_config()
    radius, r2x, f2x = scene_io.vehicle_discs(cfg)
    center = cc.straight_center(length=60.0)
    rng = np.random.default_rng(29)

    def reference_distance(poly, px, py):
        poly = np.ascontiguousarray(poly)
        if REF.ref_polygon_point_in(poly.ctypes.data_as(C.c_void_p), len(poly), px, py):
            return 0.0
        q = poly[::-1] if limit_scenes.signed_area(poly) < 0 else poly
        d = math.inf
        for i in range(len(q)):
            seg = np.ascontiguousarray(np.concatenate([q[i], q[(i + 1) % len(q)]]))
            e = REF.ref_segment_distance(seg.ctypes.data_as(C.c_void_p), px, py)
            d = e if e < d else d
        return d

    inside = clockwise = values = 0
    for scene_i in range(40):
        n = 3 + scene_i % 6
        if scene_i % 8 == 3:
            st_body, size = limit_scenes._large_polygon(rng, n, scene_i % 2 == 1)
        else:
            size = rng.uniform(0.3, 1.5)
            st_body = limit_scenes._polygon(rng, n, size, scene_i % 3 == 0, scene_i % 2 == 1)
        dy_body = limit_scenes._polygon(rng, 3 + (scene_i + 2) % 6, rng.uniform(0.3, 1.5), scene_i % 3 == 1, scene_i % 2 == 0)
        st_at, dy_at = rng.uniform([10.0, -3.0], [50.0, 3.0]), rng.uniform([10.0, -3.0], [50.0, 3.0])
        static = np.ascontiguousarray(st_body + st_at)
        heading = rng.uniform(-3.0, 3.0)
        c, s = math.cos(heading), math.sin(heading)      # Pose::transform order, the C library's cos / sin
        placed = np.array([[dy_at[0] + vx * c - vy * s, dy_at[1] + vx * s + vy * c] for vx, vy in dy_body])
        dyn = scene_io.DynamicObstacle(dy_body, np.array([[-1.0, 0.0, 0.0, 0.0], [99.0, dy_at[0], dy_at[1], heading]]))   # t = 0.5: the second sample
        scene = scene_io.Scene(np.zeros(4), np.zeros((1, 6)), [static], [dyn])
        clockwise += int(limit_scenes.signed_area(static) < 0) + int(limit_scenes.signed_area(placed) < 0)
        K = 50
        near = np.where(rng.random(K) < 0.5, 0, 1)
        reach = np.where(near == 0, size, 1.5) + 2.5
        at = np.where(near[:, None] == 0, st_at, dy_at) + rng.uniform(-1.0, 1.0, (K, 2)) * reach[:, None]
        poses = np.concatenate([at, rng.uniform(-3.2, 3.2, (K, 1))], axis=1)
        got, nearest, lowest, knot = api.clearance_rows(scene_io.flatten_scene(center, scene),
                                                        cc.rows_in_layout(api.ROWS_PLAN, np.full(K, 0.5), poses), api.ROWS_PLAN, cfg)
        assert (nearest == 0).all()
        for k, (x, y, th) in enumerate(poses.tolist()):
            ct, st = math.cos(th), math.sin(th)
            for disc, off in ((0, r2x), (1, f2x)):
                cx, cy = x + off * ct, y + off * st
                for kind, poly in ((0, static), (1, placed)):
                    d = reference_distance(poly, cx, cy)
                    assert _bits([got[k, 2 * disc + kind]])[0] == _bits([d - radius])[0], (scene_i, k, disc, kind, got[k, 2 * disc + kind], d - radius)
                    inside += d == 0.0
                    values += 1
        assert lowest == got.min() and knot == int(np.argmax((got == got.min()).any(axis=1)))
    assert values == 40 * 50 * 4 and values // 40 < inside < values // 2 and clockwise >= 20, (inside, clockwise)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_host_call_equals_the_numpy_restatement_in_every_layout():
    below = finite = 0
    for family, n, seed in (("mix11", 12, 61), ("dyn20", 4, 63)):
        sf, cfg, times, poses = cc.path_and_shift_rows(family, n, seed)
        for b, scene in enumerate(sf.scenes):
            flat = scene_io.flatten_scene(sf.center, scene)
            for j in range(poses.shape[1]):
                want = scene_io.environment_clearance(sf.center, scene, cfg, times[b], poses[b, j])
                for layout in LAYOUTS:
                    got = api.clearance_rows(flat, cc.rows_in_layout(layout, times[b], poses[b, j]), layout, cfg)
                    assert _same(got, want), (family, b, j, layout)
                below += int((want[0] < 0).sum())
                finite += int(np.isfinite(want[0]).sum())
    assert below > 50 and finite > 2 * below      # discs that reach into polygons, and many more that do not


# ---------------------------------------------------------------------------------------------------------------------
# 3. the crafted table
# ---------------------------------------------------------------------------------------------------------------------
def test_crafted_table_with_a_census_of_the_rules_branches(crafted):
    center, cases, time_cases = crafted
    seen = set()
    for case in cases:
        want = cl.expected_rows(center, case)      # (checks the constructed values against the restatement)
        flat = scene_io.flatten_scene(center, case.scene)
        for layout in LAYOUTS:
            got = api.clearance_rows(flat, cc.rows_in_layout(layout, case.times, case.poses), layout, case.cfg)
            assert _same(got, want), (case.name, layout, got, want)
        radius, r2x, f2x = scene_io.vehicle_discs(case.cfg)
        for p in case.scene.static:
            for x, y, _ in case.poses.tolist():
                if len(p):
                    seen |= cl.branches(p, x + r2x, y) | cl.branches(p, x + f2x, y)
    assert seen == set(cl.BRANCHES), set(cl.BRANCHES) - seen
    # the audit's blind spot: both centres lie inside the strip, and its mask is 0
    strip = next(c for c in cases if c.name.startswith("the audit's thin polygon"))
    flat, rows = scene_io.flatten_scene(center, strip.scene), cc.rows_in_layout(api.ROWS_TRAJ, strip.times, strip.poses)
    radius = scene_io.vehicle_discs(strip.cfg)[0]
    got = api.clearance_rows(flat, rows, api.ROWS_TRAJ, strip.cfg)
    assert got[0][0, cl.RS] == -radius and got[0][0, cl.FS] == -radius and got[2] == -radius and got[3] == 0
    assert not api.check_collisions(flat, rows, api.ROWS_TRAJ, strip.cfg, 0.0)[0].any()
    # every time case of the audit, reread as distances
    assert len(time_cases) >= 9
    for tc in time_cases:
        got = api.clearance_rows(scene_io.flatten_scene(center, tc.scene), cc.rows_in_layout(api.ROWS_TRAJ, tc.times, tc.poses),
                                 api.ROWS_TRAJ, api.default_dp_config())
        hit = (tc.expect & cc.FD) != 0
        assert (got[0][hit, cl.FD] == cl.time_case_value(api.default_dp_config())).all() and (got[0][~hit, cl.FD] > 90.0).all(), tc.name
        assert (got[0][:, [cl.RS, cl.FS]] == math.inf).all() and (got[1][:, [cl.RS, cl.FS]] == -1).all(), tc.name


def test_reversing_a_clockwise_polygon_changes_distance_bits():
    q, px, py, ruled, plain = cl.find_reversal_that_changes_bits()
    assert ruled != plain and abs(ruled - plain) < 1e-12
    cfg = cl.dyadic_config()      # rear disc centre = the pose
    scene = scene_io.Scene(np.zeros(4), np.zeros((1, 6)), [q], [])
    got = api.clearance_rows(scene_io.flatten_scene(cc.straight_center(), scene),
                             cc.rows_in_layout(api.ROWS_TRAJ, [0.0], [[px, py, 0.0]]), api.ROWS_TRAJ, cfg)
    assert got[0][0, cl.RS] == ruled - cl.R and got[0][0, cl.RS] != plain - cl.R


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_host_call(crafted):
    center, cases, _ = crafted
    case = next(c for c in cases if c.name.startswith("a NaN pose row"))
    flat = scene_io.flatten_scene(center, case.scene)
    L, cfg = api.lib(), case.cfg

    def call(layout=api.ROWS_TRAJ, n_knots=None, want_cfg=True, want_scene=True, want_rows=True, want_clearance=True,
             want_nearest=True, want_min=True, want_knot=True, edit=None, arrays=None):
        sc, keep = api.scene_struct(dict(flat, **(arrays or {})))
        if edit:
            edit(sc)
        K = len(case.times) if n_knots is None else n_knots
        rows = cc.rows_in_layout(api.ROWS_PLAN, np.resize(case.times, max(K, 1)), np.resize(case.poses, (max(K, 1), 3)))
        clearance, nearest = np.full((max(K, 1), 4), 77.0), np.full((max(K, 1), 4), 77, dtype=np.int32)
        lowest, knot = C.c_double(77.0), C.c_int32(-7)
        rc = L.cilqr_clearance_rows(C.byref(cfg) if want_cfg else None, C.byref(sc) if want_scene else None, layout,
                                    rows.ctypes.data if want_rows else None, K, clearance.ctypes.data if want_clearance else None,
                                    nearest.ctypes.data if want_nearest else None, C.byref(lowest) if want_min else None,
                                    C.byref(knot) if want_knot else None)
        if rc != api.OK:    # nothing was written
            assert (clearance == 77.0).all() and (nearest == 77).all() and lowest.value == 77.0 and knot.value == -7
        return rc

    assert call() == api.OK and call(want_nearest=False) == api.OK
    for what in ("want_cfg", "want_scene", "want_rows", "want_clearance", "want_min", "want_knot"):
        assert call(**{what: False}) == api.ERR_NULL, what
    for field in ("center", "static_points", "static_counts", "dynamic_polygon_points", "dynamic_polygon_counts",
                  "dynamic_trajectories", "dynamic_trajectory_counts"):
        assert call(edit=lambda sc, f=field: setattr(sc, f, None)) == api.ERR_NULL, field
    assert call(layout=3) == api.ERR_ARG and call(layout=-1) == api.ERR_ARG and call(layout=api.ROWS_POINTS) == api.ERR_ARG
    assert call(n_knots=0) == api.ERR_ARG and call(n_knots=-4) == api.ERR_ARG
    assert call(edit=lambda sc: setattr(sc, "n_center", 1)) == api.ERR_ARG
    assert call(edit=lambda sc: setattr(sc, "n_dynamic", -1)) == api.ERR_ARG
    assert call(arrays=dict(static_counts=np.array([-1], dtype=np.int32))) == api.ERR_ARG
    assert call(arrays=dict(dynamic_polygon_counts=np.array([-1], dtype=np.int32))) == api.ERR_ARG
    assert call(arrays=dict(dynamic_trajectory_counts=np.array([-3], dtype=np.int32))) == api.ERR_ARG
    assert call(n_knots=api.DP_MAX_KNOTS) == api.OK and call(n_knots=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    assert call(edit=lambda sc: setattr(sc, "n_dynamic", api.DP_MAX_DYNAMIC + 1)) == api.ERR_CAPACITY
    assert call(arrays=dict(static_counts=np.array([api.DP_MAX_VERTICES + 1], dtype=np.int32))) == api.ERR_CAPACITY
    assert call(arrays=dict(dynamic_trajectory_counts=np.array([api.DP_MAX_SAMPLES + 1], dtype=np.int32))) == api.ERR_CAPACITY
    many = scene_io.flatten_scene(center, scene_io.Scene(np.zeros(4), np.zeros((1, 6)), [np.zeros((3, 2))] * (api.DP_MAX_STATIC + 1), []))
    with pytest.raises(api.CilqrError) as e:
        api.clearance_rows(many, cc.rows_in_layout(api.ROWS_TRAJ, case.times, case.poses), api.ROWS_TRAJ)
    assert e.value.code == api.ERR_CAPACITY
    with pytest.raises(api.CilqrError) as e:
        api.clearance_rows(flat, np.zeros((5, 2)), api.ROWS_POINTS)
    assert e.value.code == api.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 5. sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_crafted_table_under_address_and_undefined_behaviour_sanitizers(crafted, tmp_path):
    """tests/cpp/clearance_test.cc -- a program of its own around include/cilqr/dp_planner.hpp -- built with
    -fsanitize=address,undefined and run on the crafted table as a child process."""
    center, cases, _ = crafted
    path = tmp_path / "cases.bin"
    cl.write_cases(path, center, cases)
    exe = tmp_path / "clearance_test"
    # (the runtimes linked statically: the program then does not care what else a machine loads into its processes)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "clearance_test.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    knots = sum(len(c.times) for c in cases)
    assert run.stdout.strip() == f"{len(cases)} cases, {knots} knots, 0 failures"
