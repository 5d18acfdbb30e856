"""cilqr_amd.episode.run_episode on the GPU: three planning cycles on five scenes with 15 s recordings (1501 samples per
dynamic obstacle, more than the scene kernels take) against the same public calls made by hand, the scene clocks advancing by
the driven rows' times, and a scene whose tracker fails going alive = 0 without touching the other four."""
import dataclasses

import numpy as np
import pytest

import scene_window_cases as sw
from cilqr_amd import api, episode, scenario, scene_io

pytestmark = pytest.mark.gpu
B, CYCLES, N_DRIVE, FAILING = 5, 3, 6, 2
PLANNED = ("traj", "status", "n_cost", "cost_hist", "n_iter", "plan", "dp", "outcome")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def world():
    """five mix11 scenes whose dynamic obstacles are 15 s recordings at 10 ms, the handle, and the episode run_episode makes
    of them: computed once"""
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, B, seed=91, scenarios=True)
    sf = scene_io.from_generator(sc)
    scenes = [dataclasses.replace(s, dynamic=[scene_io.DynamicObstacle(d.polygon, sw.recording(d.trajectory)) for d in s.dynamic])
              for s in sf.scenes]
    packed = scene_io.pack_scene_batch(sf.center, scenes)
    assert packed["max_samples"] == 1501 > api.DP_MAX_SAMPLES
    start = np.ascontiguousarray(sc["start"], dtype=np.float64)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=B, cmax=16, max_lane_segments=256) as opt:
        ep = episode.run_episode(opt, packed, start, CYCLES, N_DRIVE)
        yield dict(opt=opt, packed=packed, start=start, ep=ep)


def test_every_cycle_is_the_public_calls_made_by_hand(world):
    opt, packed, ep = world["opt"], world["packed"], world["ep"]
    dp_cfg = api.default_dp_config(tf=opt.N * opt.cfg.dt, delta_t=opt.cfg.dt)
    cor_cfg = api.default_corridor_config()
    assert len(ep["cycles"]) == CYCLES
    t0, start4 = np.zeros(B), world["start"].copy()
    start6 = np.concatenate([start4, np.zeros((B, 2))], axis=1)
    prev = None
    for c, got in enumerate(ep["cycles"]):
        assert got["alive"].all() and got["window_ok"].all() and (got["track_ok"] == 1).all(), c
        assert np.array_equal(got["t0"], t0), c
        win = opt.window_scenes(packed, t0, float(dp_cfg.tf))
        assert win["max_samples"] <= api.DP_MAX_SAMPLES
        warm = None if prev is None else (prev["traj"], np.where(prev["outcome"] == 0, N_DRIVE - 1, -1).astype(np.int32), api.ROWS_TRAJ)
        plan = opt.plan_scenes(win, start4, dp_cfg, cor_cfg, warm=warm)
        for k in PLANNED:
            assert sw.same_bits(got[k], plan[k]), (c, k)
        driven, ok = opt.track(plan["traj"], api.ROWS_TRAJ, start6, N_DRIVE)
        assert sw.same_bits(got["driven"], driven) and np.array_equal(got["track_ok"], ok), c
        # knot 0 of the plan is the state the vehicle really reached, with a = delta = 0
        assert sw.same_bits(plan["traj"][:, 0, 1:5], start4) and (plan["traj"][:, 0, 5:7] == 0.0).all(), c
        assert sw.same_bits(driven[:, 0, 1:7], start6), c
        # the clocks advance by the driven rows' times: five steps of dt
        step = driven[:, N_DRIVE - 1, 0] - driven[:, 0, 0]
        assert np.allclose(step, (N_DRIVE - 1) * opt.cfg.dt, rtol=0, atol=1e-9), c
        t0 = t0 + step
        start6 = np.ascontiguousarray(driven[:, N_DRIVE - 1, 1:7])
        start4 = np.ascontiguousarray(start6[:, :4])
        prev = plan
    assert sw.same_bits(ep["t0"], t0) and sw.same_bits(ep["start4"], start4) and ep["alive"].all()
    planned = np.stack([g["outcome"] == 0 for g in ep["cycles"]])
    assert planned.all(axis=0).sum() >= 2
    # the vehicles went somewhere
    moved = np.linalg.norm(ep["start4"][:, :2] - world["start"][:, :2], axis=1)
    assert (moved[planned.all(axis=0)] > 1.0).all()


class _TrackerFailsFor:
    """the handle, except that the trajectory scene `b` is asked to follow has a time column that stands still: the tracker's
    clock ends before n_drive rows are recorded, and it reports ok = 0 for that scene"""

    def __init__(self, opt, b):
        self._opt, self._b = opt, b

    def __getattr__(self, name):
        return getattr(self._opt, name)

    def track(self, rows, layout, start6=None, n_drive=None):
        rows = np.array(rows)
        rows[self._b, :, 0] = 0.0
        return self._opt.track(rows, layout, start6, n_drive)


def test_a_scene_whose_tracker_fails_goes_dead_and_the_others_do_not_notice(world):
    opt, packed, ep = world["opt"], world["packed"], world["ep"]
    hurt = episode.run_episode(_TrackerFailsFor(opt, FAILING), packed, world["start"], CYCLES, N_DRIVE)
    others = np.arange(B) != FAILING
    for c, (got, want) in enumerate(zip(hurt["cycles"], ep["cycles"])):
        assert got["track_ok"][FAILING] == 0 and not got["alive"][FAILING] and got["alive"][others].all(), c
        assert (got["driven"][FAILING] == 0.0).all()
        assert got["t0"][FAILING] == 0.0 and sw.same_bits(got["traj"][FAILING, 0, 1:5], world["start"][FAILING]), c   # it stays put
        for k in PLANNED + ("driven", "track_ok", "t0"):
            assert sw.same_bits(got[k][others], want[k][others]), (c, k)
    assert hurt["t0"][FAILING] == 0.0 and sw.same_bits(hurt["start4"][FAILING], world["start"][FAILING])
    assert sw.same_bits(hurt["t0"][others], ep["t0"][others]) and sw.same_bits(hurt["start4"][others], ep["start4"][others])
