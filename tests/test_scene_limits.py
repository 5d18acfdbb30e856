"""The yardsticks of tests/test_gpu_scene_limits.py at the declared limits of the scene kernels, without a GPU: the host
planner against the line-by-line oracle on corner scenes (tests/limit_scenes.py), the packed arrays at 32 / 32 / 8 /
1024, environment_points against a loop that selects the sample by walking the trajectory, and what the scene builder
promises."""
import dataclasses

import numpy as np
import pytest

import limit_scenes as ls
from cilqr_amd import api, scenario, scene_io
from oracle import oracle as orc

EPS = scene_io.K_MATH_EPS


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _assert_host_is_oracle(sf, start, tf, over, which):
    cfg = api.default_dp_config(tf=tf, **over)
    found = []
    for b in which:
        flat = scene_io.flatten_scene(sf.center, sf.scenes[b])
        ok, co = api.dp_plan(flat, start[b, :3], cfg)
        o_ok, o_co = orc.dp_plan(flat, start[b, :3], tf=tf, **over)
        assert ok == o_ok, b
        assert co.shape == o_co.shape == (ls.dp_counts(tf)[0], 9)
        assert np.array_equal(co, o_co, equal_nan=True), (b, np.flatnonzero((co != o_co).any(axis=1))[:4])
        found.append(ok)
    return found


# scenes 4 and 5 of a row: 5 is the one whose road is blocked
@pytest.mark.parametrize("row,which", [("full_8s", (4, 5)), ("full_25s", (5, 6)), ("budget_5s", (3, 4, 5)), ("small_5s", (3, 4, 5))])
def test_host_planner_is_the_oracle_on_corner_scenes(row, which):
    r = ls.ROWS[row]
    sc, sf, over = ls.corner_scenes(8, 301, r["S"], r["D"], r["V"], r["T"], r["tf"], r["over"])
    found = _assert_host_is_oracle(sf, sc["start"], r["tf"], over, which)
    assert found[which.index(5)] is False and any(found)


@pytest.mark.parametrize("tf", [12.7, 13.2])
def test_host_planner_is_the_oracle_where_path_samples_outnumber_the_knots(tf):
    n_knots, nq = ls.dp_counts(tf)
    assert nq == n_knots + 1
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, 3, seed=302, scenarios=True)
    sf = scene_io.from_generator(sc)
    over = dict(max_velocity=10.0)
    assert any(_assert_host_is_oracle(sf, sc["start"], tf, over, range(3)))
    # and on a corner scene of that horizon
    sc, sf, over = ls.corner_scenes(2, 303, 32, 32, 8, 1024, tf, over)
    _assert_host_is_oracle(sf, sc["start"], tf, over, (1,))


def test_the_lattice_restatement_counts_what_the_planner_counts():
    """dp_counts against what the library shows of its own count: the last knot repeats its predecessor's velocity and
    acceleration exactly when it is the last path sample (ComputePathProfile), and a count above 256 is refused."""
    assert ls.dp_counts(5.0) == (51, 51) and ls.dp_counts(8.0) == (81, 81) and ls.dp_counts(10.0) == (101, 101)
    assert ls.dp_counts(25.5) == (api.DP_MAX_KNOTS, api.DP_MAX_KNOTS)
    assert ls.dp_counts(12.7) == (127, 128) and ls.dp_counts(13.2) == (132, 133) and ls.dp_counts(25.4) == (254, 255)
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, 1, seed=304, scenarios=True)
    sf = scene_io.from_generator(sc)
    flat = scene_io.flatten_scene(sf.center, sf.scenes[0])
    for tf in (8.0, 12.7, 13.2, 25.5):
        n_knots, nq = ls.dp_counts(tf)
        ok, co = api.dp_plan(flat, sc["start"][0, :3], api.default_dp_config(tf=tf, max_velocity=10.0))
        assert ok and co.shape[0] == n_knots
        assert np.array_equal(co[:, 0], 0.1 * np.arange(n_knots))
        assert bool(co[-1, 6] == co[-2, 6]) == (nq == n_knots), tf
    # every horizon on the 0.1 s grid: never fewer path samples than knots, so no knot is left as constructed
    for tf in np.round(np.arange(0.5, 25.65, 0.1), 1):
        n_knots, nq = ls.dp_counts(float(tf))
        assert n_knots <= nq <= n_knots + 1, tf


def test_pack_round_trips_at_the_limits():
    S, D, V, T = api.DP_MAX_STATIC, api.DP_MAX_DYNAMIC, api.DP_MAX_VERTICES, api.DP_MAX_SAMPLES
    assert (S, D, V, T) == (32, 32, 8, 1024)
    sc, sf, _ = ls.corner_scenes(3, 305, S, D, V, T, 8.0)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    assert (packed["max_static"], packed["max_dynamic"], packed["max_vertices"], packed["max_samples"]) == (S, D, V, T)
    assert (packed["static_counts"] >= 3).all() and (packed["dynamic_polygon_counts"] >= 3).all()
    assert packed["dynamic_trajectory_counts"].max() == T and packed["dynamic_trajectory_counts"].min() == 1
    again = scene_io.pack_scene_batch(sf.center, sf.scenes, max_static=S, max_dynamic=D, max_vertices=V, max_samples=T)
    for b in range(3):
        flat, back = scene_io.flatten_scene(sf.center, sf.scenes[b]), scene_io.unpack_scene(packed, b)
        assert flat.keys() == back.keys()
        for k in flat:
            assert flat[k].dtype == back[k].dtype and np.array_equal(flat[k], back[k]), (b, k)
            assert np.array_equal(scene_io.unpack_scene(again, b)[k], back[k])
        # what lies behind a polygon's vertices and a trajectory's samples is zero
        for o in range(S):
            assert not packed["static_points"][b, o, packed["static_counts"][b, o]:].any()
        for o in range(D):
            assert not packed["dynamic_polygon_points"][b, o, packed["dynamic_polygon_counts"][b, o]:].any()
            assert not packed["dynamic_trajectories"][b, o, packed["dynamic_trajectory_counts"][b, o]:].any()


def _walk_points(scene, times, multiple):
    """Environment::Query{Static,Dynamic}ObstaclesPoints statement by statement: the sample of a dynamic obstacle is
    found by walking its trajectory from the front.  (points per knot, the chosen sample per knot and obstacle, -1 =
    not there)."""
    pick = scene_io.sample_points if multiple else (lambda p: p)
    per_knot, chosen = [], []
    for t in times:
        pts, ids = [pick(p) for p in scene.static], []
        for d in scene.dynamic:
            tr = d.trajectory
            if tr[0, 0] > t + EPS or tr[-1, 0] < t - EPS:
                ids.append(-1)
                continue
            i = 0
            while i < len(tr) and not (t < tr[i, 0] + EPS):
                i += 1
            i = min(i, len(tr) - 1)
            ids.append(i)
            c, s = np.cos(tr[i, 3]), np.sin(tr[i, 3])
            pts.append(pick(np.stack([tr[i, 1] + d.polygon[:, 0] * c - d.polygon[:, 1] * s,
                                      tr[i, 2] + d.polygon[:, 0] * s + d.polygon[:, 1] * c], axis=1)))
        per_knot.append(np.concatenate(pts, axis=0))
        chosen.append(ids)
    return per_knot, np.array(chosen)


def tie_knots(scene, tf):
    """Per tie of limit_scenes.TIES: (the knot whose time is the tied path-sample time, the tied sample)."""
    sample_times = ls.dp_sample_times(tf)
    out = {}
    for i, name in enumerate(ls.TIES):
        tt = scene.dynamic[1 + i].trajectory[:, 0]
        j = int(np.flatnonzero(tt[1:] == tt[:-1])[0]) + 1 if name == "twin" else int(np.flatnonzero(np.isin(tt, sample_times))[0])
        out[name] = (int(round(tt[j] / 0.1)), j)
    return out


@pytest.mark.parametrize("multiple", [False, True])
def test_environment_points_on_a_corner_scene_with_the_ties(multiple):
    tf = 8.0
    sc, sf, _ = ls.corner_scenes(2, 306, 32, 32, 8, 1024, tf)
    scene = sf.scenes[1]
    K = ls.dp_counts(tf)[0]
    times = 0.1 * np.arange(K)
    pts, cnt = scene_io.environment_points(scene, times, multiple_sample=multiple)
    want, chosen = _walk_points(scene, times, multiple)
    assert np.array_equal(cnt, [len(w) for w in want]) and cnt.max() > 32 * 8 * (6 if multiple else 1)
    for k in range(K):
        assert np.array_equal(pts[k, :cnt[k]], want[k]), k
        assert not pts[k, cnt[k]:].any()
    ties = tie_knots(scene, tf)
    traj = [d.trajectory[:, 0] for d in scene.dynamic]
    # a sample time equal to a knot time (to well within 1e-10): that sample is the one shown at the knot
    k, j = ties["sample"]
    assert abs(traj[1][j] - times[k]) < 1e-12 and 0 < j < len(traj[1]) - 1 and chosen[k, 1] == j
    k, j = ties["first"]      # there from its first sample's knot on, not before
    assert j == 0 and chosen[k, 2] == 0 and (chosen[:k, 2] == -1).all()
    k, j = ties["last"]       # there up to its last sample's knot, not after
    assert j == len(traj[3]) - 1 and chosen[k, 3] == j and (chosen[k + 1:, 3] == -1).all()
    k, j = ties["single"]     # there at one knot alone
    assert len(traj[4]) == 1 and list(np.flatnonzero(chosen[:, 4] >= 0)) == [k]
    k, j = ties["twin"]       # the second of two samples with one time is never the first later one
    assert traj[5][j] == traj[5][j - 1] and not (chosen[:, 5] == j).any() and (chosen[:, 5] >= 0).any()


def test_the_builder_keeps_its_promises():
    r = ls.ROWS["full_8s"]
    sc, sf, _ = ls.corner_scenes(18, 307, r["S"], r["D"], r["V"], r["T"], r["tf"])
    sc2, sf2, _ = ls.corner_scenes(18, 307, r["S"], r["D"], r["V"], r["T"], r["tf"])
    sample_times = ls.dp_sample_times(r["tf"])
    assert len(sample_times) == 81 and sample_times[0] == 0.0 and (np.diff(sample_times) > 0).all()
    polys = []
    for a, b in zip(sf.scenes, sf2.scenes):       # deterministic from the seed
        fa, fb = scene_io.flatten_scene(sf.center, a), scene_io.flatten_scene(sf2.center, b)
        assert all(np.array_equal(fa[k], fb[k]) for k in fa)
        assert np.array_equal(a.start, b.start)
    for b, s in enumerate(sf.scenes):
        assert len(s.static) == r["S"] and len(s.dynamic) == r["D"]
        assert len(s.static[0]) == r["V"] and len(s.dynamic[0].polygon) == r["V"] and len(s.dynamic[0].trajectory) == r["T"]
        polys += list(s.static) + [d.polygon for d in s.dynamic]
        for d in s.dynamic:
            tt = d.trajectory[:, 0]
            assert 1 <= len(tt) <= r["T"] and (np.diff(tt) >= 0).all() and np.isfinite(d.trajectory).all()
        # the ties are equalities in floating point, with the planner's own expression on the other side
        for i, name in enumerate(ls.TIES):
            tt = s.dynamic[1 + i].trajectory[:, 0]
            at = np.flatnonzero(np.isin(tt, sample_times))
            if name == "sample":
                assert len(at) == 1 and 0 < at[0] < len(tt) - 1
            elif name == "first":
                assert at.tolist() == [0]
            elif name == "last":
                assert at.tolist() == [len(tt) - 1]
            elif name == "single":
                assert len(tt) == 1 and at.tolist() == [0]
            else:
                assert (tt[1:] == tt[:-1]).sum() == 1
        # the other obstacles' times are no path-sample times
        assert not any(np.isin(d.trajectory[:, 0], sample_times).any() for d in s.dynamic[6:])
    areas = np.array([ls.signed_area(q) for q in polys])
    assert (areas > 0).sum() > len(polys) // 3 and (areas < 0).sum() > len(polys) // 3        # both orientations
    assert sum(ls.is_concave(q) for q in polys) > len(polys) // 10                            # concave ones
    assert {len(q) for q in polys} == set(range(3, r["V"] + 1))                               # every vertex count
    sizes = np.array([np.hypot(*(q - q.mean(axis=0)).T).max() for q in polys])
    assert (sizes >= 10.0).sum() >= 4 and np.median(sizes) < 1.5
    windows = [(d.trajectory[0, 0] < 0, d.trajectory[-1, 0] > r["tf"]) for s in sf.scenes for d in s.dynamic]
    assert {(True, True), (True, False), (False, True), (False, False)} <= set(windows)
    lengths = [len(d.trajectory) for s in sf.scenes for d in s.dynamic]
    assert min(lengths) == 1 and max(lengths) == r["T"]
    # the small corner of the issue's table
    r = ls.ROWS["small_5s"]
    sc, sf, _ = ls.corner_scenes(6, 308, r["S"], r["D"], r["V"], r["T"], r["tf"])
    assert {len(q) for s in sf.scenes for q in s.static} == set(range(3, 8))
    assert all(len(s.static) == 3 and len(s.dynamic) == 4 for s in sf.scenes)
