"""cilqr_amd.episode.run_episode with prediction: three planning cycles on four scenes, one of which has a pedestrian whose
recording begins at 1.0 s.  Every cycle is the public calls made by hand -- predict_scenes, plan_scenes (warm, and with
carry), track --, bit for bit; the pedestrian's slot is empty until the scene clock reaches its first sample; with
prediction = None the episode is the loop it was.  Nothing is asserted about what the planner decides."""
import dataclasses

import numpy as np
import pytest

import predict_cases as pc
import scene_window_cases as sw
from cilqr_amd import api, episode, scenario, scene_io

pytestmark = pytest.mark.gpu
B, CYCLES, N_DRIVE, WITH_PEDESTRIAN = 4, 3, 6, 1
PLANNED = ("traj", "status", "n_cost", "cost_hist", "n_iter", "plan", "dp", "outcome")
CARRY = dict(max_advance=1.0, max_start_offset=1.0, collision_buffer=0.0, refresh_every=0)
PREDICTION = dict(mode=api.PREDICT_CONSTANT_VELOCITY, max_age=0.5)
APPEARS = 1.0


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def world():
    """four mix11 scenes whose dynamic obstacles are 15 s recordings at 10 ms, one more obstacle in one of them that is first
    recorded at 1.0 s, the handle, and the episodes the tests read: computed once"""
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, B, seed=91, scenarios=True)
    sf = scene_io.from_generator(sc)
    scenes = [dataclasses.replace(s, dynamic=[scene_io.DynamicObstacle(d.polygon, sw.recording(d.trajectory)) for d in s.dynamic])
              for s in sf.scenes]
    start = np.ascontiguousarray(sc["start"], dtype=np.float64)
    t = APPEARS + np.arange(1401) * 0.01
    x, y = start[WITH_PEDESTRIAN, 0] + 25.0, start[WITH_PEDESTRIAN, 1] - 6.0
    walk = np.ascontiguousarray(np.stack([t, np.full_like(t, x), y + 1.2 * (t - APPEARS), np.zeros_like(t)], axis=1))
    slot = len(scenes[WITH_PEDESTRIAN].dynamic)
    scenes[WITH_PEDESTRIAN] = dataclasses.replace(scenes[WITH_PEDESTRIAN], dynamic=list(scenes[WITH_PEDESTRIAN].dynamic) + [
        scene_io.DynamicObstacle(np.array([[0.3, 0.3], [0.3, -0.3], [-0.3, -0.3], [-0.3, 0.3]]), walk)])
    packed = scene_io.pack_scene_batch(sf.center, scenes)
    assert packed["max_samples"] == 1501 > api.DP_MAX_SAMPLES and packed["dynamic_trajectory_counts"][WITH_PEDESTRIAN, slot] == 1401
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=B, cmax=16, max_lane_segments=256) as opt:
        run = lambda **kw: episode.run_episode(opt, packed, start, CYCLES, N_DRIVE, **kw)
        yield dict(opt=opt, packed=packed, start=start, slot=slot, plain=run(), none=run(prediction=None),
                   predicted=run(prediction=PREDICTION), both=run(prediction=PREDICTION, carry=CARRY))


def _by_hand(world, carry):
    """the cycles of an episode with prediction made of public calls: [(predicted scene, plan, driven, track_ok, t0)]"""
    opt, packed = world["opt"], world["packed"]
    dp_cfg = api.default_dp_config(tf=opt.N * opt.cfg.dt, delta_t=opt.cfg.dt)
    cor_cfg = api.default_corridor_config()
    out = scene_io.predict_out_samples(float(dp_cfg.delta_t), float(dp_cfg.tf))
    t0, start4 = np.zeros(B), world["start"].copy()
    start6 = np.concatenate([start4, np.zeros((B, 2))], axis=1)
    prev, advance, cycles = None, None, []
    for c in range(CYCLES):
        pred = opt.predict_scenes(packed, t0, float(dp_cfg.tf), PREDICTION["mode"], PREDICTION["max_age"], float(dp_cfg.delta_t), out)
        warm = None if prev is None else (prev["traj"], np.where(prev["outcome"] == 0, N_DRIVE - 1, -1).astype(np.int32), api.ROWS_TRAJ)
        if carry is None or prev is None:
            plan = opt.plan_scenes(pred, start4, dp_cfg, cor_cfg, warm=warm)
        else:
            plan = opt.plan_scenes(pred, start4, dp_cfg, cor_cfg, warm=warm, carry=dict(
                rows=prev["plan"], layout=api.ROWS_PLAN, advance=np.where(prev["outcome"] == api.PLAN_OK, advance, -1.0),
                max_advance=carry["max_advance"], max_start_offset=carry["max_start_offset"],
                collision_buffer=carry["collision_buffer"]))
        driven, ok = opt.track(plan["traj"], api.ROWS_TRAJ, start6, N_DRIVE)
        assert (ok == 1).all() and pred["predict_ok"].all(), c          # every scene stays alive: the loop below is the whole loop
        cycles.append((pred, plan, driven, ok, t0.copy()))
        advance = driven[:, N_DRIVE - 1, 0] - driven[:, 0, 0]
        t0 = t0 + advance
        start6 = np.ascontiguousarray(driven[:, N_DRIVE - 1, 1:7])
        start4 = np.ascontiguousarray(start6[:, :4])
        prev = plan
    return cycles, t0, start4


@pytest.mark.parametrize("carry", [None, CARRY], ids=["prediction", "prediction-and-carry"])
def test_every_cycle_is_the_public_calls_made_by_hand(world, carry):
    ep = world["predicted"] if carry is None else world["both"]
    cycles, t0, start4 = _by_hand(world, carry)
    out = cycles[0][0]["max_samples"]
    assert out == 52 and len(ep["cycles"]) == CYCLES
    empty, full = 0, 0
    for c, (got, (pred, plan, driven, ok, at)) in enumerate(zip(ep["cycles"], cycles)):
        assert got["alive"].all() and got["window_ok"].all() and sw.same_bits(got["t0"], at), c
        for k in PLANNED + (("source",) if carry is not None and c > 0 else ()):
            assert sw.same_bits(got[k], plan[k]), (c, k)
        assert sw.same_bits(got["driven"], driven) and np.array_equal(got["track_ok"], ok), c
        # the pedestrian: not there before its first sample has been observed, predicted from then on
        counts = pred["dynamic_trajectory_counts"]
        seen = not (scene_io.PREDICT_MARGIN < APPEARS - at[WITH_PEDESTRIAN])
        assert counts[WITH_PEDESTRIAN, world["slot"]] == (out if seen else 0), (c, at[WITH_PEDESTRIAN])
        empty, full = empty + (not seen), full + seen
        recorded = world["packed"]["dynamic_trajectory_counts"] > 0
        recorded[WITH_PEDESTRIAN, world["slot"]] = seen
        assert np.array_equal(counts, np.where(recorded, out, 0)), c
    assert empty >= 1 and full >= 1 and ep["cycles"][0]["t0"][WITH_PEDESTRIAN] == 0.0
    assert sw.same_bits(ep["t0"], t0) and sw.same_bits(ep["start4"], start4)
    if carry is not None:
        assert (ep["cycles"][0]["source"] == api.CARRY_NOT_ASKED).all() and "source" not in world["predicted"]["cycles"][1]


def test_without_prediction_the_episode_is_the_loop_it_was(world):
    for c, (a, b) in enumerate(zip(world["plain"]["cycles"], world["none"]["cycles"])):
        assert a.keys() == b.keys()
        for k in PLANNED + ("driven", "track_ok", "t0", "window_ok", "alive"):
            assert sw.same_bits(a[k], b[k]), (c, k)
    # ... and that loop reads the recording's window, which knows the pedestrian from the start
    opt, packed = world["opt"], world["packed"]
    win = opt.window_scenes(packed, np.zeros(B), opt.N * opt.cfg.dt)
    assert win["dynamic_trajectory_counts"][WITH_PEDESTRIAN, world["slot"]] > 0
    pred = opt.predict_scenes(packed, np.zeros(B), opt.N * opt.cfg.dt, PREDICTION["mode"], PREDICTION["max_age"], opt.cfg.dt)
    assert pred["dynamic_trajectory_counts"][WITH_PEDESTRIAN, world["slot"]] == 0
