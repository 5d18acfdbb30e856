"""The batched DP coarse planner on the GPU (cilqr_dp_plan_batch, kernels_dp.hip) against the host planner
cilqr_dp_plan -- which tests/test_dp_planner.py holds bit for bit to oracle/dp_oracle.cc -- and against the oracle
itself on a sample.

What "the same" means (rules 3 and 4 below are used for both yardsticks):
  3. same plan: `found` equal, the time and station columns BIT-IDENTICAL (they contain no transcendental: they differ
     only if another lattice path was chosen or a collision test flipped), the NaN pattern of all nine columns equal.
     Scenes that fail this are counted, listed in the record and capped at 0.5 % per family; each must still be a
     well-formed, collision-free plan if found.  The cap comes from a perturbation experiment on the host planner: with
     every sin / cos / atan / atan2 / hypot result moved at random by up to +-2 ulp, 0 of 1300 scenes changed their plan.
  4. same numbers: on the scenes that pass 3, every finite entry of the other columns within 1e-9, scaled per column by
     max(1, max |column|) -- the tolerance of the stage outputs (DESIGN 5 rule 3); the perturbations moved them by
     at most 2e-13.
The record of a run (scene counts, failing scenes, the largest error per column, the timings) is printed as one line that
starts with DP_BATCH_RECORD (pytest -s shows it)."""
import ctypes as C
import dataclasses
import json
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import limit_scenes
from cilqr_amd import api, scenario, scene_io
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FAMILIES = {"mix11": (5.0, 101), "demo80": (8.0, 102), "dyn20": (10.0, 103)}   # tf, seed
N_SCENES = 2048
HOST_WORKERS = 16
TOL = 1e-9
CAP = 0.005
COLS = ("time", "s", "x", "y", "theta", "kappa", "velocity", "a", "delta")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _scenes(family, n, seed, **kw):
    spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, **kw)
    return sc, scene_io.from_generator(sc)


def _host_plan(sf, start, cfg, which=None, workers=HOST_WORKERS):
    which = range(len(sf.scenes)) if which is None else which

    def one(b):
        return api.dp_plan(scene_io.flatten_scene(sf.center, sf.scenes[b]), start[b, :3], cfg)

    with ThreadPoolExecutor(workers) as pool:
        outs = list(pool.map(one, which))
    return np.array([o[0] for o in outs], dtype=bool), np.stack([o[1] for o in outs])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _device_call(opt, packed, start, cfg, K, outputs=("dp", "coarse", "knots", "station")):
    """cilqr_dp_plan_batch with every per-problem array resident on the device; returns (rc, host copies, the tensors)."""
    import torch
    dev = torch.device("cuda", 0)
    B = packed["batch"]
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    t["start"] = torch.from_numpy(np.ascontiguousarray(start[:, :3])).to(dev)
    width = dict(dp=9, coarse=6, knots=3)
    o = {k: torch.full((B, K) + ((width[k],) if k in width else ()), -7.0, dtype=torch.float64, device=dev) for k in outputs}
    o["found"] = torch.full((B,), -7, dtype=torch.int32, device=dev)
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ptr = lambda k: o[k].data_ptr() if k in o else None   # noqa: E731
    rc, nnf = opt.dp_plan_batch_raw(cfg, sb, t["start"].data_ptr(), K, ptr("dp"), ptr("coarse"), ptr("knots"), ptr("station"),
                                    o["found"].data_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["n_not_found"] = nnf
    return rc, out, dict(t, **o)


def _well_formed(co, scene, start, dt, wheel_base=1.0):
    """The properties of tests/test_dp_planner.py::test_paths_are_well_formed_and_keep_clear_of_the_obstacles."""
    K = co.shape[0]
    length = 0.96 + 1.0 + 0.929
    radius, r2x, f2x = np.hypot(0.25 * length, 0.5 * 1.942), 0.25 * length - 0.929, 0.75 * length - 0.929
    t, s, x, y, th, kap, v, a, dl = co.T
    assert np.allclose(t, np.arange(K) * dt) and np.all(np.diff(s) >= -1e-12)
    pts, cnt = scene_io.environment_points(scene, t)
    for i in range(K):
        p = pts[i, :cnt[i]]
        for off in (r2x, f2x):
            cx, cy = x[i] + off * np.cos(th[i]), y[i] + off * np.sin(th[i])
            assert not ((np.abs(p[:, 0] - cx) <= radius) & (np.abs(p[:, 1] - cy) <= radius)).any(), i
    if np.isfinite(co).all():
        acc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
        assert np.allclose(v[:-1], np.diff(acc) / dt, rtol=0, atol=1e-9) and v[-1] == v[-2]
        assert np.allclose(a[:-2], np.diff(v[:-1]) / dt, atol=1e-7) and a[-1] == a[-2]
        assert np.allclose(dl, np.arctan(kap * wheel_base))
    assert abs(co[0, 2] - start[0]) < 0.2 and abs(co[0, 3] - start[1]) < 0.2


def _compare(found, dp, ref_found, ref_dp, scenes, start, dt, what):
    """Rules 3 and 4 for one family; returns the record."""
    n = len(ref_found)
    same_plan = (found == ref_found)
    for b in range(n):
        same_plan[b] = same_plan[b] and np.array_equal(dp[b][:, :2], ref_dp[b][:, :2], equal_nan=True) and \
            np.array_equal(np.isnan(dp[b]), np.isnan(ref_dp[b]))
    failing = [int(b) for b in np.flatnonzero(~same_plan)]
    rec = dict(what=what, scenes=n, found=int(ref_found.sum()), with_nan=int(np.isnan(ref_dp).any(axis=(1, 2)).sum()),
               other_plan=failing)
    print("DP_BATCH_RECORD", json.dumps(rec), flush=True)
    assert len(failing) <= CAP * n, rec
    for b in failing:
        if found[b]:
            _well_formed(dp[b], scenes[b], start[b], dt)
    ok = np.flatnonzero(same_plan)
    err = {}
    for c in range(2, 9):
        r, g = ref_dp[ok][:, :, c], dp[ok][:, :, c]
        fin = np.isfinite(r)
        scale = max(1.0, float(np.abs(r[fin]).max())) if fin.any() else 1.0
        err[COLS[c]] = float((np.abs(g[fin] - r[fin]) / scale).max()) if fin.any() else 0.0
    rec["max_scaled_error"] = err
    print("DP_BATCH_RECORD", json.dumps(rec), flush=True)
    assert max(err.values()) <= TOL, rec
    return rec


@pytest.fixture(scope="module")
def planned():
    """Per family: N_SCENES distinct scenes, the host planner's results (HOST_WORKERS threads), the device planner's
    results from HOST arrays, and both wall times."""
    out = {}
    for family, (tf, seed) in FAMILIES.items():
        sc, sf = _scenes(family, N_SCENES, seed)
        cfg = api.default_dp_config(tf=tf)
        K = int(tf / 0.1 + 1)
        t0 = time.perf_counter()
        h_found, h_dp = _host_plan(sf, sc["start"], cfg)
        host_s = time.perf_counter() - t0
        packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
        opt = api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=1, cmax=16)
        first = opt.dp_plan_batch(packed, sc["start"], cfg)      # grows the handle's work space
        t0 = time.perf_counter()
        r = opt.dp_plan_batch(packed, sc["start"], cfg)
        dev_s = time.perf_counter() - t0
        out[family] = dict(sc=sc, sf=sf, cfg=cfg, K=K, tf=tf, packed=packed, opt=opt, host_found=h_found, host_dp=h_dp,
                           first=first, dev=r, host_s=host_s, dev_s=dev_s)
        print("DP_BATCH_RECORD", json.dumps(dict(family=family, scenes=N_SCENES, host_threads=HOST_WORKERS,
                                                 host_planner_s=host_s, device_call_from_host_arrays_s=dev_s)), flush=True)
    yield out
    for v in out.values():
        v["opt"].close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_same_plan_and_same_numbers_as_the_host_planner(planned, family):
    p = planned[family]
    r = p["dev"]
    assert r["dp"].shape == (N_SCENES, p["K"], 9) and r["n_not_found"] == int((~r["found"]).sum())
    rec = _compare(r["found"], r["dp"], p["host_found"], p["host_dp"], p["sf"].scenes, p["sc"]["start"], 0.1, family)
    assert rec["found"] > 0


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_device_call_is_faster_than_the_threaded_host_planner(planned, family):
    p = planned[family]
    assert p["dev_s"] < p["host_s"], (family, p["dev_s"], p["host_s"])


@pytest.mark.parametrize("family", list(FAMILIES))
def test_views_memories_repeats_and_batch_mates_change_no_bit(planned, family):
    p = planned[family]
    r, opt = p["dev"], p["opt"]
    assert _same_bits(r["coarse"], np.ascontiguousarray(r["dp"][:, :, [2, 3, 4, 6, 7, 8]]))
    assert _same_bits(r["knots"], np.ascontiguousarray(r["dp"][:, :, [2, 3, 4]]))
    assert _same_bits(r["station"], np.ascontiguousarray(r["dp"][:, :, 1]))
    for k in ("dp", "coarse", "knots", "station", "found"):
        assert _same_bits(r[k], p["first"][k]), k                                  # a second call
    rc, d, _ = _device_call(opt, p["packed"], p["sc"]["start"], p["cfg"], p["K"])
    assert rc == api.OK and d["n_not_found"] == r["n_not_found"]
    for k in ("dp", "coarse", "knots", "station"):
        assert _same_bits(d[k], r[k]), k                                           # DEVICE arrays
    assert np.array_equal(d["found"] != 0, r["found"])
    # outputs are optional one by one
    rc, d1, _ = _device_call(opt, p["packed"], p["sc"]["start"], p["cfg"], p["K"], outputs=("station",))
    assert rc == api.OK and _same_bits(d1["station"], r["station"]) and np.array_equal(d1["found"], d["found"])
    # a scene's result does not depend on its batch-mates
    pick = np.sort(np.random.default_rng(7).choice(N_SCENES, 64, replace=False))
    scenes = [p["sf"].scenes[b] for b in pick]
    sizes = {k: p["packed"][k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples")}
    own = opt.dp_plan_batch(scene_io.pack_scene_batch(p["sf"].center, scenes, **sizes), p["sc"]["start"][pick], p["cfg"])
    assert _same_bits(own["dp"], r["dp"][pick]) and np.array_equal(own["found"], r["found"][pick])
    for j, b in enumerate(pick):
        one = opt.dp_plan_batch(scene_io.pack_scene_batch(p["sf"].center, [scenes[j]]), p["sc"]["start"][b:b + 1], p["cfg"])
        assert _same_bits(one["dp"][0], r["dp"][b]) and one["found"][0] == r["found"][b], b


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_sample_against_the_line_by_line_oracle(planned, family):
    p = planned[family]
    pick = np.sort(np.random.default_rng(11).choice(N_SCENES, 32, replace=False))
    o_found, o_dp = [], []
    for b in pick:
        ok, co = orc.dp_plan(scene_io.flatten_scene(p["sf"].center, p["sf"].scenes[b]), p["sc"]["start"][b, :3], tf=p["tf"])
        o_found.append(ok)
        o_dp.append(co)
    _compare(p["dev"]["found"][pick], p["dev"]["dp"][pick], np.array(o_found, dtype=bool), np.stack(o_dp),
             [p["sf"].scenes[b] for b in pick], p["sc"]["start"][pick], 0.1, family + " / oracle")


def _wall_scene(sc, sf, b):
    """The wall of test_blocked_road_is_reported_as_dp_failed across the road where the ego of scene b stands."""
    scene = dataclasses.replace(sf.scenes[b], static=list(sf.scenes[b].static))
    x0, y0, th, _ = sc["road"].eval(np.array([0.5]))     # demo80 scenes start at station 0.5
    c, s_ = np.cos(th[0]), np.sin(th[0])
    wall = np.array([[1.0, 9.0], [1.0, -9.0], [-1.0, -9.0], [-1.0, 9.0]])
    scene.static.append(np.stack([x0[0] + wall[:, 0] * c - wall[:, 1] * s_, y0[0] + wall[:, 0] * s_ + wall[:, 1] * c], 1))
    return scene


def test_a_blocked_road_inside_a_batch():
    sc, sf = _scenes("demo80", 24, 31)
    cfg = api.default_dp_config()
    sizes = dict(max_static=8, max_dynamic=12)
    with api.BatchIlqrOptimizer(n_steps=80, batch_capacity=1, cmax=16) as opt:
        plain = opt.dp_plan_batch(scene_io.pack_scene_batch(sf.center, sf.scenes, **sizes), sc["start"], cfg)
        scenes = list(sf.scenes)
        scenes[5] = _wall_scene(sc, sf, 5)
        walled = opt.dp_plan_batch(scene_io.pack_scene_batch(sf.center, scenes, **sizes), sc["start"], cfg)
    assert not walled["found"][5] and np.isfinite(walled["dp"][5][:, :5]).all()
    assert walled["n_not_found"] == int((~walled["found"]).sum()) == plain["n_not_found"] + int(plain["found"][5])
    keep = np.arange(24) != 5
    for k in ("dp", "coarse", "knots", "station", "found"):
        assert _same_bits(walled[k][keep], plain[k][keep]), k
    ok, co = api.dp_plan(scene_io.flatten_scene(sf.center, scenes[5]), sc["start"][5, :3], cfg)
    assert not ok and np.array_equal(walled["dp"][5][:, :2], co[:, :2])
    assert np.abs(walled["dp"][5][:, 2:5] - co[:, 2:5]).max() < 1e-9


def _sample_pick_scenes(cfg):
    """Four scenes for the pick of a dynamic obstacle's sample (k_dp_place bisects, the host planner scans): each keeps
    its start and carries ONE dynamic obstacle, 8 m long and 4 m wide, with T = 1, 2, 3 and 1024 samples, that stands on
    the path the host planner takes through the empty scene, where the ego is at a time the sample is shown.
    Neighbouring samples stand at different places, so another index is another obstacle.  ts: the planner's own
    path-sample times.  Returns (generator dict, the scenes, the plans through the empty scenes)."""
    sc, sf = _scenes("mix11", 4, 57)
    ts = limit_scenes.dp_sample_times(5.0)
    road = sc["road"]
    body = np.array([[4.0, 2.0], [-4.0, 2.0], [-4.0, -2.0], [4.0, -2.0]])   # wider than a collision square: none passes through unseen
    bare = scene_io.SceneFile(sf.dt, sf.center, [scene_io.Scene(s.start.copy(), s.coarse.copy(), [], []) for s in sf.scenes])
    b_found, b_dp = _host_plan(bare, sc["start"], cfg, workers=4)
    assert b_found.all()

    def on_path(b, times, ego_times):
        """samples at `times` that stand where the ego of the empty scene b is at `ego_times`"""
        x, y, th = (np.interp(ego_times, b_dp[b][:, 0], b_dp[b][:, c]) for c in (2, 3, 4))
        return np.ascontiguousarray(np.stack([np.asarray(times, dtype=float), x, y, th], axis=1))

    # T = 1: there at one path-sample time alone; the sample behind the end is the last (and only) one
    t1 = on_path(0, [ts[12]], [ts[12]])
    # T = 2: from a path-sample time to the LAST path-sample time, both exactly; sample 0 is never the first behind a time
    t2 = on_path(1, [ts[4], ts[-1]], [1.0, 3.0])
    # T = 3: the run of two equal times IS a path-sample time: before it sample 1, at it the clamp to sample 2
    t3 = on_path(2, [ts[2], ts[20], ts[20]], [0.5, 1.5, ts[20]])
    # T = 1024: ascending to the last path-sample time exactly, with a run of five equal times on a path-sample time, four
    # more samples on path-sample times; the obstacle drives ahead of the ego on the centre line at 5 m/s, and every sample
    # from the run's end on stands 1.5 m further to the right
    tt = np.empty(1024)
    tt[:500] = np.linspace(-0.5, np.nextafter(ts[24], 0.0), 500)
    tt[500:505] = ts[24]
    tt[505:] = np.linspace(np.nextafter(ts[24], 9.0), ts[-1], 519)
    for j in (7, 15, 33, 41):
        tt[np.searchsorted(tt, ts[j])] = ts[j]
    assert np.all(np.diff(tt) >= 0) and tt[-1] == ts[-1] and (tt == ts[24]).sum() == 5 and all((tt == ts[j]).any() for j in (7, 15, 33, 41))
    s0 = float(road.s[np.argmin((road.x - sf.scenes[3].start[0]) ** 2 + (road.y - sf.scenes[3].start[1]) ** 2)])
    x, y, th, _ = road.eval(s0 + 10.0 + 5.0 * (tt + 0.5))
    lateral = np.where(np.arange(1024) >= 504, -1.5, 0.0)
    t1024 = np.ascontiguousarray(np.stack([tt, x - lateral * np.sin(th), y + lateral * np.cos(th), th], axis=1))
    scenes = [scene_io.Scene(sf.scenes[b].start.copy(), sf.scenes[b].coarse.copy(), [], [scene_io.DynamicObstacle(body, t)])
              for b, t in enumerate((t1, t2, t3, t1024))]
    return sc, scene_io.SceneFile(sf.dt, sf.center, scenes), b_dp


def test_the_bisected_sample_is_the_scanned_one_at_ties_runs_and_the_clamp():
    """k_dp_place picks a dynamic obstacle's sample by bisection, cilqr_dp_plan by a scan from the front: on T = 1, 2, 3 and
    1024 non-decreasing sample times -- sample times equal to path-sample times, a run of equal times on one, the last
    sample time equal to the last path-sample time -- the same plan, bit for bit in the time and station columns (rules 3
    and 4, no scene excepted).  Preconditions, asserted: the host planner finds a path in every scene, and the obstacle
    moves that path (by more than 0.5 m somewhere), so the sample that is picked matters."""
    cfg = api.default_dp_config(tf=5.0)
    sc, sf, b_dp = _sample_pick_scenes(cfg)
    assert [len(s.dynamic[0].trajectory) for s in sf.scenes] == [1, 2, 3, 1024]
    h_found, h_dp = _host_plan(sf, sc["start"], cfg, workers=4)
    assert h_found.all()
    moved = [float(np.abs(h_dp[b][:, 2:4] - b_dp[b][:, 2:4]).max()) for b in range(4)]
    assert min(moved) > 0.5, moved
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=1, cmax=16) as opt:
        r = opt.dp_plan_batch(scene_io.pack_scene_batch(sf.center, sf.scenes), sc["start"], cfg)
    rec = _compare(r["found"], r["dp"], h_found, h_dp, sf.scenes, sc["start"], 0.1, "sample pick: T = 1, 2, 3, 1024")
    assert rec["other_plan"] == [] and r["found"].all()


def test_non_default_weights_and_vehicle_reach_the_kernel():
    sc, sf = _scenes("demo80", 16, 11)
    over = dict(dp_nominal_velocity=6.0, dp_w_lateral=0.8, dp_w_lateral_change=0.1, dp_w_longitudinal_velocity_change=3.0,
                width=2.3, wheel_base=1.6, max_velocity=14.0, dp_w_obstacle=500.0)
    cfg = api.default_dp_config(**over)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    with api.BatchIlqrOptimizer(n_steps=80, batch_capacity=1, cmax=16) as opt:
        r = opt.dp_plan_batch(packed, sc["start"], cfg)
        r0 = opt.dp_plan_batch(packed, sc["start"])
    h_found, h_dp = _host_plan(sf, sc["start"], cfg, workers=8)
    _compare(r["found"], r["dp"], h_found, h_dp, sf.scenes, sc["start"], 0.1, "demo80 / other weights and vehicle")
    assert not np.array_equal(r["dp"], r0["dp"], equal_nan=True)
    f = r["found"] & r0["found"]
    assert abs(np.median(r["dp"][f][:, :, 6]) - 6.0) < abs(np.median(r0["dp"][f][:, :, 6]) - 6.0)


def test_argument_errors_launch_nothing_and_leave_the_handle_usable():
    sc, sf = _scenes("mix11", 8, 41)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    start = np.ascontiguousarray(sc["start"][:, :3])
    K = 51
    good = api.default_dp_config(tf=5.0)
    L = api.lib()
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=1, cmax=16) as opt:
        reference = opt.dp_plan_batch(packed, sc["start"], good)

        def call(cfg=good, n_knots=K, handle=opt.h, start_ptr=start.ctypes.data, found=True, edit=None, arrays=None, **sizes):
            a = dict(keep, **(arrays or {}))
            sb = api.scene_batch_struct(dict(packed, **sizes), api.MEM_HOST, **{k: a[k].ctypes.data for k in a})
            if edit:
                edit(sb)
            dp = np.full((8, K, 9), -7.0)
            fnd = np.full(8, -7, dtype=np.int32)
            nnf = C.c_int32(-7)
            rc = L.cilqr_dp_plan_batch(handle, C.byref(cfg) if cfg is not None else None, C.byref(sb), start_ptr, n_knots,
                                       dp.ctypes.data, None, None, None, fnd.ctypes.data if found else None, C.byref(nnf))
            if rc != api.OK:    # nothing was launched, nothing written
                assert (dp == -7.0).all() and (fnd == -7).all() and nnf.value == -7
            return rc

        def null(field):
            return lambda sb: setattr(sb, field, None)

        assert call(cfg=None) == api.ERR_NULL and call(start_ptr=None) == api.ERR_NULL and call(found=False) == api.ERR_NULL
        for field in ("center", "static_points", "static_counts", "dynamic_polygon_points", "dynamic_polygon_counts",
                      "dynamic_trajectories", "dynamic_trajectory_counts"):
            assert call(edit=null(field)) == api.ERR_NULL, field
        assert call(edit=lambda sb: setattr(sb, "n_center", 1)) == api.ERR_ARG
        assert call(edit=lambda sb: setattr(sb, "batch", 0)) == api.ERR_ARG
        assert call(edit=lambda sb: setattr(sb, "memory", 5)) == api.ERR_ARG
        assert call(cfg=api.default_dp_config(tf=-1.0)) == api.ERR_ARG
        assert call(cfg=api.default_dp_config(tf=5.0, delta_t=0.0)) == api.ERR_ARG
        assert call(cfg=api.default_dp_config(tf=float("nan"))) == api.ERR_ARG
        assert call(n_knots=81) == api.ERR_KNOTS
        assert call(cfg=api.default_dp_config(tf=8.0)) == api.ERR_KNOTS
        for name, lim in (("max_vertices", api.DP_MAX_VERTICES), ("max_static", api.DP_MAX_STATIC),
                          ("max_dynamic", api.DP_MAX_DYNAMIC), ("max_samples", api.DP_MAX_SAMPLES)):
            assert call(**{name: lim + 1}) == api.ERR_CAPACITY, name
        assert call(cfg=api.default_dp_config(tf=30.0), n_knots=int(30.0 / 0.1 + 1)) == api.ERR_CAPACITY
        for name, bad in (("static_counts", packed["max_vertices"] + 1), ("static_counts", -1),
                          ("dynamic_polygon_counts", packed["max_vertices"] + 1), ("dynamic_polygon_counts", -2),
                          ("dynamic_trajectory_counts", packed["max_samples"] + 1), ("dynamic_trajectory_counts", -1)):
            a = keep[name].copy()
            a[3, 0] = bad
            assert call(arrays={name: a}) == api.ERR_ARG, (name, bad)
        assert call() == api.OK
        again = opt.dp_plan_batch(packed, sc["start"], good)
        assert _same_bits(again["dp"], reference["dp"]) and np.array_equal(again["found"], reference["found"])


def test_solves_in_flight_refuse_the_planner():
    g = scenario.generate("mix11", 64, seed=3)
    sc, sf = _scenes("mix11", 4, 41)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=64, cmax=g["cmax"]) as opt:
        prob, keep = opt._host_problem(g)
        B, K, M = 64, 51, opt.cfg.max_iter
        traj, hist = np.zeros((B, K, 10)), np.zeros((B, M + 1, 5))
        nc, st, ni = (np.zeros(B, dtype=np.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_HOST, 0, traj.ctypes.data, hist.ctypes.data, nc.ctypes.data, st.ctypes.data,
                                ni.ctypes.data, None, None, None)
        assert opt.L.cilqr_submit(opt.h, C.byref(prob), C.byref(sol)) == api.OK
        with pytest.raises(api.CilqrError) as e:
            opt.dp_plan_batch(packed, sc["start"], api.default_dp_config(tf=5.0))
        assert e.value.code == api.ERR_STATE
        assert opt.L.cilqr_wait(opt.h) == api.OK
        assert opt.dp_plan_batch(packed, sc["start"], api.default_dp_config(tf=5.0))["dp"].shape == (4, 51, 9)


def test_hostile_input_inside_a_batch_harms_no_other_scene():
    """Input validation, not fault injection: every index the kernel forms is bounded by the max_* of the call, and
    non-finite coordinates run through the host planner's own comparisons."""
    sc, sf = _scenes("mix11", 32, 77)
    cfg = api.default_dp_config(tf=5.0)
    K = 51
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    start = sc["start"].copy()
    hostile = dict(packed, **{k: packed[k].copy() for k in api._SCENE_BATCH_ARRAYS})
    start_h = start.copy()
    start_h[3, 0] = np.nan                                            # a NaN start
    b_s = int(np.flatnonzero(packed["static_counts"][:, 0] > 0)[0])
    hostile["static_points"][b_s, 0, 1, 0] = np.nan                   # a NaN polygon vertex
    b_d = int(np.flatnonzero(packed["dynamic_polygon_counts"][:, 0] > 0)[-1])
    hostile["dynamic_trajectory_counts"][b_d, 0] = 0                  # a dynamic obstacle with zero samples
    bad = sorted({3, b_s, b_d})
    keep = np.array([b not in bad for b in range(32)])
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=1, cmax=16) as opt:
        plain = opt.dp_plan_batch(packed, start, cfg)
        h1 = opt.dp_plan_batch(hostile, start_h, cfg)
        h2 = opt.dp_plan_batch(hostile, start_h, cfg)
        rc, d, _ = _device_call(opt, hostile, start_h, cfg, K)
        # DEVICE arrays carry their counts unchecked to the kernel: a count beyond the arrays marks that scene alone
        worse = dict(hostile, static_counts=hostile["static_counts"].copy(), dynamic_trajectory_counts=hostile["dynamic_trajectory_counts"].copy())
        worse["static_counts"][9, 0] = 1 << 20
        worse["dynamic_trajectory_counts"][10, 0] = -5
        rc2, d2, _ = _device_call(opt, worse, start_h, cfg, K)
    for k in ("dp", "coarse", "knots", "station", "found"):
        assert _same_bits(h1[k], h2[k]), k                            # deterministic
        assert _same_bits(h1[k][keep], plain[k][keep]), k             # the others: untouched
    assert rc == api.OK and _same_bits(d["dp"], h1["dp"])
    assert not h1["found"][3] and h1["n_not_found"] == int((~h1["found"]).sum())
    # an obstacle without samples is never there: the scene is planned as without it, as cilqr_dp_plan does
    scene = dataclasses.replace(sf.scenes[b_d], dynamic=sf.scenes[b_d].dynamic[1:]) if b_d != b_s and b_d != 3 else None
    if scene is not None:
        ok, co = api.dp_plan(scene_io.flatten_scene(sf.center, scene), start[b_d, :3], cfg)
        assert ok == h1["found"][b_d] and np.array_equal(h1["dp"][b_d][:, :2], co[:, :2], equal_nan=True)
    assert rc2 == api.OK
    assert d2["found"][9] == 0 and d2["found"][10] == 0 and not d2["dp"][9].any() and not d2["dp"][10].any()
    rest = keep.copy()
    rest[[9, 10]] = False
    assert _same_bits(d2["dp"][rest], plain["dp"][rest]) and np.array_equal(d2["found"][rest] != 0, plain["found"][rest])
    assert d2["n_not_found"] == int((d2["found"] == 0).sum())


def test_scene_to_trajectory_on_the_device():
    """dp_plan_batch -> build_corridors -> solve_batch with every array in HBM, against the same three calls made with
    HOST arrays that hold the device planner's own output: bit for bit (this is the plumbing; the planner is held
    above).  A chain fed by the host planner is only reported beside it: x / y differ in the last place, and the solve
    amplifies that on a few per cent of the scenes."""
    import torch
    B = 256
    g = scenario.generate_dp("mix11", B, seed=91, workers=HOST_WORKERS)
    sf = g["scene_file"]
    K, cmax = g["n_steps"] + 1, g["cmax"]
    cfg = api.default_dp_config(tf=g["n_steps"] * g["dt"], delta_t=g["dt"])
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    dev = torch.device("cuda", 0)
    left, right = np.ascontiguousarray(g["left"]), np.ascontiguousarray(g["right"])
    P = g["obstacle_points"].shape[2]
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=B, cmax=cmax) as opt:
        M = opt.cfg.max_iter
        rc, d, t = _device_call(opt, packed, g["start"], cfg, K)
        assert rc == api.OK
        t_pts = torch.from_numpy(np.ascontiguousarray(g["obstacle_points"])).to(dev)
        t_pcnt = torch.from_numpy(np.ascontiguousarray(g["obstacle_count"])).to(dev)
        t_start4 = torch.from_numpy(np.ascontiguousarray(g["start"])).to(dev)
        d_cor = torch.zeros((B, K, cmax, 3), dtype=torch.float64, device=dev)
        d_cnt = torch.zeros((B, K), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc, nf = opt.build_corridors_raw(api.default_corridor_config(), B, K, t["knots"].data_ptr(), t_pts.data_ptr(),
                                         t_pcnt.data_ptr(), P, d_cor.data_ptr(), d_cnt.data_ptr(), cmax, api.MEM_DEVICE)
        assert rc == api.OK
        o_traj = torch.zeros((B, K, 10), dtype=torch.float64, device=dev)
        o_hist = torch.zeros((B, M + 1, 5), dtype=torch.float64, device=dev)
        o_nc, o_st = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        prob = opt.make_problem(B, t_start4.data_ptr(), t["coarse"].data_ptr(), d_cor.data_ptr(), d_cnt.data_ptr(), cmax,
                                left.ctypes.data, right.ctypes.data, left.shape[0], right.shape[0], api.MEM_DEVICE)
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, o_traj.data_ptr(), o_hist.data_ptr(), o_nc.data_ptr(), o_st.data_ptr(),
                                None, None, None)
        assert opt.solve_raw(prob, sol) == api.OK
        torch.cuda.synchronize()
        # the same three calls from HOST arrays
        r = opt.dp_plan_batch(packed, g["start"], cfg)
        for k in ("dp", "coarse", "knots", "station"):
            assert _same_bits(r[k], d[k]), k
        cor_h, cnt_h, nf_h = opt.build_corridors(r["knots"], g["obstacle_points"], g["obstacle_count"], cmax=cmax)
        assert nf_h == nf and _same_bits(cor_h, d_cor.cpu().numpy()) and _same_bits(cnt_h, d_cnt.cpu().numpy())
        host = opt.plan(dict(g, coarse=r["coarse"], corridor=cor_h, ccount=cnt_h))
        assert _same_bits(host["traj"], o_traj.cpu().numpy()) and np.array_equal(host["status"], o_st.cpu().numpy())
        assert np.array_equal(host["n_cost"], o_nc.cpu().numpy())
        # beside it, reported only: the chain behind the host planner
        knots_h = np.ascontiguousarray(g["dp"][:, :, [2, 3, 4]])
        cor2, cnt2, _ = opt.build_corridors(knots_h, g["obstacle_points"], g["obstacle_count"], cmax=cmax)
        host2 = opt.plan(dict(g, corridor=cor2, ccount=cnt2))
        print("DP_BATCH_RECORD", json.dumps(dict(chain="mix11", scenes=B, corridors_failed=nf,
                                                 status_behind_device_planner=np.bincount(host["status"], minlength=7).tolist(),
                                                 status_behind_host_planner=np.bincount(host2["status"], minlength=7).tolist())), flush=True)


def test_generate_dp_with_the_device_planner():
    gh = scenario.generate_dp("demo80", 12, seed=51, workers=8)
    gd = scenario.generate_dp("demo80", 12, seed=51, planner="device")
    assert gh.keys() == gd.keys()
    assert gd["coarse"].shape == (12, 81, 6) and gd["dp"].shape == (12, 81, 9) and gd["found"].dtype == bool
    assert np.array_equal(gd["found"], gh["found"]) and gd["found"].sum() >= 8
    assert np.array_equal(gd["dp"][:, :, :2], gh["dp"][:, :, :2], equal_nan=True)
    f = gd["found"]
    assert np.abs(gd["coarse"][f] - gh["coarse"][f]).max() < 1e-9 * max(1.0, np.abs(gh["coarse"][f]).max())
    assert np.array_equal(gd["coarse"][:, :, 0], gd["dp"][:, :, 2]) and np.array_equal(gd["coarse"][:, :, 5], gd["dp"][:, :, 8], equal_nan=True)
    for b in range(12):
        assert np.array_equal(gd["scene_file"].scenes[b].coarse, gd["coarse"][b], equal_nan=True)
