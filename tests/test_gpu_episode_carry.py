"""cilqr_amd.episode.run_episode with carry: three planning cycles on eight scenes.  The first cycle is the cold pipeline;
with carry = None the episode is the loop it was, bit for bit; with carry on every later cycle returns `source`, a scene
whose source is not zero has the DP planner's rows, a kept scene the rows cilqr_carry_rows_batch makes of its previous plan."""
import dataclasses

import numpy as np
import pytest

import scene_window_cases as sw
from cilqr_amd import api, episode, scenario, scene_io

pytestmark = pytest.mark.gpu
B, CYCLES, N_DRIVE = 8, 3, 6
PLANNED = ("traj", "status", "n_cost", "cost_hist", "n_iter", "plan", "dp", "outcome")
CARRY = dict(max_advance=1.0, max_start_offset=1.0, collision_buffer=0.0, refresh_every=0)


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def world():
    """eight mix11 scenes, the handle, and the three episodes the tests read: computed once"""
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, B, seed=91, scenarios=True)
    sf = scene_io.from_generator(sc)
    packed = scene_io.pack_scene_batch(sf.center, list(sf.scenes))
    start = np.ascontiguousarray(sc["start"], dtype=np.float64)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=B, cmax=16, max_lane_segments=256) as opt:
        plain = episode.run_episode(opt, packed, start, CYCLES, N_DRIVE)
        none = episode.run_episode(opt, packed, start, CYCLES, N_DRIVE, carry=None)
        carried = episode.run_episode(opt, packed, start, CYCLES, N_DRIVE, carry=CARRY)
        yield dict(opt=opt, packed=packed, start=start, plain=plain, none=none, carried=carried)


def test_without_carry_the_episode_is_the_loop_it_was(world):
    """... which is the public calls made by hand: window, plan (warm), track"""
    opt, packed = world["opt"], world["packed"]
    dp_cfg = api.default_dp_config(tf=opt.N * opt.cfg.dt, delta_t=opt.cfg.dt)
    cor_cfg = api.default_corridor_config()
    t0, start4 = np.zeros(B), world["start"].copy()
    start6 = np.concatenate([start4, np.zeros((B, 2))], axis=1)
    prev = None
    for c in range(CYCLES):
        win = opt.window_scenes(packed, t0, float(dp_cfg.tf))
        warm = None if prev is None else (prev["traj"], np.where(prev["outcome"] == 0, N_DRIVE - 1, -1).astype(np.int32), api.ROWS_TRAJ)
        plan = opt.plan_scenes(win, start4, dp_cfg, cor_cfg, warm=warm)
        driven, ok = opt.track(plan["traj"], api.ROWS_TRAJ, start6, N_DRIVE)
        assert (ok == 1).all()
        for ep in (world["plain"], world["none"]):
            got = ep["cycles"][c]
            assert "source" not in got and "n_kept" not in got
            for k in PLANNED:
                assert sw.same_bits(got[k], plan[k]), (c, k)
            assert sw.same_bits(got["driven"], driven) and sw.same_bits(got["t0"], t0), c
        t0 = t0 + (driven[:, N_DRIVE - 1, 0] - driven[:, 0, 0])
        start6 = np.ascontiguousarray(driven[:, N_DRIVE - 1, 1:7])
        start4 = np.ascontiguousarray(start6[:, :4])
        prev = plan
    assert sw.same_bits(world["none"]["t0"], t0) and sw.same_bits(world["none"]["start4"], start4)


def test_the_first_cycle_is_the_cold_pipeline(world):
    first, cold = world["carried"]["cycles"][0], world["plain"]["cycles"][0]
    for k in PLANNED + ("driven", "track_ok", "t0"):
        assert sw.same_bits(first[k], cold[k]), k
    assert (first["source"] == api.CARRY_NOT_ASKED).all() and first["n_kept"] == 0


def test_later_cycles_return_source_and_plan_where_it_says(world):
    opt, packed, ep = world["opt"], world["packed"], world["carried"]
    dp_cfg = api.default_dp_config(tf=opt.N * opt.cfg.dt, delta_t=opt.cfg.dt)
    cor_cfg = api.default_corridor_config()
    kept_anywhere = 0
    for c in range(1, CYCLES):
        prev, got = ep["cycles"][c - 1], ep["cycles"][c]
        assert prev["alive"].sum() >= B - 1, c
        source = got["source"]
        assert source.dtype == np.int32 and source.shape == (B,) and set(source) <= {0, 1, 2, 3, 4}
        assert got["n_kept"] == (source == 0).sum()
        asked = (prev["outcome"] == api.PLAN_OK) & prev["alive"]
        assert (source[~asked] == api.CARRY_NOT_ASKED).all() and (source[asked] != api.CARRY_NOT_ASKED).all()
        # the cycle's inputs, as the loop made them: knot 0 of a plan is the start state it was given
        start4 = np.ascontiguousarray(got["traj"][:, 0, 1:5])
        advance = prev["driven"][:, N_DRIVE - 1, 0] - prev["driven"][:, 0, 0]
        win = opt.window_scenes(packed, got["t0"], float(dp_cfg.tf))
        cold = opt.plan_scenes(win, start4, dp_cfg, cor_cfg)                  # the DP planner for every scene
        carried = opt.carry(prev["plan"], api.ROWS_PLAN, np.where(asked, advance, -1.0), CARRY["max_advance"])
        for b in range(B):
            if source[b] != 0:
                assert sw.same_bits(got["dp"][b], cold["dp"][b]), (c, b)
            else:
                assert carried["state"][b] == 0 and sw.same_bits(got["dp"][b], carried["coarse9"][b]), (c, b)
                # the kept rows start where the vehicle is and clear the obstacles of the window
                assert np.hypot(*(got["dp"][b, 0, 2:4] - start4[b, :2])) <= CARRY["max_start_offset"]
        hits = opt.check_collisions(win, got["dp"], api.ROWS_COARSE, dp_cfg, CARRY["collision_buffer"])["first_hit"]
        assert (hits[source == 0] == -1).all(), c
        kept_anywhere += int((source == 0).sum())
    assert kept_anywhere >= 2          # the feature did something: plans were carried, not only replanned


def test_a_refresh_cycle_plans_every_scene_with_the_dp_planner(world):
    opt = world["opt"]
    ep = episode.run_episode(opt, world["packed"], world["start"], CYCLES, N_DRIVE, carry=dict(CARRY, refresh_every=2))
    assert (ep["cycles"][2]["source"] == api.CARRY_NOT_ASKED).all() and ep["cycles"][2]["n_kept"] == 0
    assert sw.same_bits(ep["cycles"][1]["source"], world["carried"]["cycles"][1]["source"])
