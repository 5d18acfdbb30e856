"""The collision audit on the GPU (cilqr_check_collisions_batch, kernels_collision.hip) against the host audit
(cilqr_check_collisions, which tests/test_collisions.py holds to the reference's own classes).

The kernel takes the vehicle heading through lean_sincos and places the obstacles with the device library's cos / sin; the
host uses the C library's.  A verdict can therefore differ only where a point lies within rounding of a square's side or
of a polygon's edge.  A knot is DECIDED if the host verdict is the same nine times over: at the given inputs, and with each
of buffer, x, y, theta moved by +-1e-9 (collision_cases.host_verdicts).  On decided knots the kernel's mask must equal the
host's bit for bit; on decided scenes (every knot decided) first_hit and n_hit too; and at most 1 % of the knots of a test
may be undecided -- a condition on the test's scenes, met with room to spare on continuous random scenes (checked on the
CPU when the scenes were chosen: none or a handful per test).  The crafted cases are exact on both sides and held exactly."""
import ctypes as C
import dataclasses
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import collision_cases as cc
import limit_scenes
from cilqr_amd import api, scenario, scene_io

pytestmark = pytest.mark.gpu

HOST_WORKERS = 16
UNDECIDED_SHARE = 0.01


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=128, cmax=16, max_lane_segments=256) as o:
        yield o


def _host(center, scenes, times, poses, cfg, buffer):
    """collision_cases.host_verdicts for every scene, on HOST_WORKERS threads: mask [B,K], first [B], n_hit [B], decided [B,K]"""
    def one(b):
        return cc.host_verdicts(scene_io.flatten_scene(center, scenes[b]), times[b], poses[b], cfg, buffer)
    with ThreadPoolExecutor(HOST_WORKERS) as pool:
        r = list(pool.map(one, range(len(scenes))))
    return (np.stack([v[0] for v in r]), np.array([v[1] for v in r]), np.array([v[2] for v in r]), np.stack([v[3] for v in r]))


def _device(opt, packed, rows, layout, cfg, buffer, want_mask=True, want_n_hit=True):
    """cilqr_check_collisions_batch with every array resident on the device: dict(mask, first_hit, n_hit, n_colliding)."""
    import torch
    dev = torch.device("cuda", 0)
    cfg = cfg or api.default_dp_config()
    B, K = rows.shape[0], rows.shape[1]
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    mask = torch.full((B, K), 77, dtype=torch.uint8, device=dev)
    first = torch.full((B,), -7, dtype=torch.int32, device=dev)
    n_hit = torch.full((B,), -7, dtype=torch.int32, device=dev)
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rc, n = opt.check_collisions_raw(cfg, sb, layout, d_rows.data_ptr(), K, buffer, mask.data_ptr() if want_mask else None,
                                     first.data_ptr(), n_hit.data_ptr() if want_n_hit else None)
    torch.cuda.synchronize()
    assert rc == api.OK, rc
    return dict(mask=mask.cpu().numpy(), first_hit=first.cpu().numpy(), n_hit=n_hit.cpu().numpy(), n_colliding=n)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("mask", "first_hit", "n_hit")) and a["n_colliding"] == b["n_colliding"]


def _hold(got, host, what):
    """The rule of the module text; returns (knots, undecided knots)."""
    mask, first, n_hit, decided = host
    assert got["mask"].shape == mask.shape, what
    wrong = decided & (got["mask"] != mask)
    assert not wrong.any(), (what, np.argwhere(wrong)[:5], got["mask"][wrong][:5], mask[wrong][:5])
    whole = decided.all(axis=1)
    assert np.array_equal(got["first_hit"][whole], first[whole]) and np.array_equal(got["n_hit"][whole], n_hit[whole]), what
    # whatever the masks are, the three outputs of a scene agree with each other
    any_hit = got["mask"] != 0
    assert np.array_equal(got["n_hit"], any_hit.sum(axis=1)), what
    assert np.array_equal(got["first_hit"], np.where(any_hit.any(axis=1), any_hit.argmax(axis=1), -1)), what
    assert got["n_colliding"] == int((got["first_hit"] >= 0).sum()), what
    return decided.size, int((~decided).sum())


def _every_bit_set_and_clear(masks):
    seen = np.concatenate([m.ravel() for m in masks])
    for bit in api.HIT_BITS:
        assert (seen & bit).any() and not (seen & bit).all(), bit


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the host call
# ---------------------------------------------------------------------------------------------------------------------
def test_generator_scenes_against_the_host_call(opt):
    knots = undecided = 0
    masks = []
    for family, n, seed in (("mix11", 256, 71), ("dyn20", 64, 72)):
        sf, cfg, times, poses = cc.path_and_shift_rows(family, n, seed, planner=opt)
        assert times.shape[1] == {"mix11": 51, "dyn20": 101}[family]
        packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
        for buffer in (0.0, 0.3):
            for j in range(poses.shape[1]):
                got = opt.check_collisions(packed, cc.rows_in_layout(api.ROWS_PLAN, times, poses[:, j]), api.ROWS_PLAN, cfg, buffer)
                a, b = _hold(got, _host(sf.center, sf.scenes, times, poses[:, j], cfg, buffer), (family, buffer, j))
                knots, undecided = knots + a, undecided + b
                masks.append(got["mask"])
    print("COLLISION_AUDIT_RECORD", dict(knots=knots, undecided=undecided), flush=True)
    assert undecided <= UNDECIDED_SHARE * knots, (undecided, knots)
    _every_bit_set_and_clear(masks)


# ---------------------------------------------------------------------------------------------------------------------
# 2. declared limits and tile edges
# ---------------------------------------------------------------------------------------------------------------------
def _road_rows(sc, sf, K, dt, seed):
    """K poses per scene along the road from the scene's start at 7 m/s, swaying 3.5 m to either side: times [B,K], poses [B,K,3]"""
    road = sc["road"]
    B = len(sf.scenes)
    rng = np.random.default_rng(seed)
    times = np.tile(np.arange(K) * dt, (B, 1))
    poses = np.zeros((B, K, 3))
    for b, scene in enumerate(sf.scenes):
        s0 = float(road.s[np.argmin((road.x - scene.start[0]) ** 2 + (road.y - scene.start[1]) ** 2)])
        s = np.minimum(s0 + 7.0 * times[b], road.length - 0.5)
        lat = -1.75 + 3.5 * np.sin(rng.uniform(0, 6.28) + rng.uniform(0.2, 0.6) * times[b]) + rng.uniform(-0.5, 0.5)
        x, y, th, _ = road.eval(s)
        poses[b] = np.stack([x - lat * np.sin(th), y + lat * np.cos(th), th + rng.uniform(-0.3, 0.3, K)], axis=1)
    return times, poses


LIMIT_ROWS = {
    # name: scenes, S, D, V, T, knots, time step
    "every limit at once": (4, 32, 32, 8, 1024, 256, 0.1),
    "one knot": (3, 3, 4, 7, 64, 1, 0.1),
    "seven knots": (3, 3, 4, 7, 64, 7, 0.7),
    "eight knots": (3, 3, 4, 7, 64, 8, 0.6),
    "nine knots": (3, 3, 4, 7, 64, 9, 0.55),
    "31 dynamic slots": (3, 5, 31, 6, 200, 51, 0.1),
    "one dynamic slot": (3, 5, 1, 6, 200, 51, 0.1),
    "no dynamic slot": (3, 5, 0, 6, 200, 51, 0.1),
    "no static slot": (3, 0, 7, 6, 200, 51, 0.1),
    "triangles only": (3, 6, 6, 3, 100, 51, 0.1),
    "a batch of one": (1, 3, 4, 7, 64, 51, 0.1),
    "a batch of 300": (300, 3, 4, 7, 64, 51, 0.1),
}


@pytest.mark.parametrize("name", list(LIMIT_ROWS))
def test_declared_limits_and_tile_edges(opt, name):
    n, S, D, V, T, K, dt = LIMIT_ROWS[name]
    tf = max((K - 1) * dt, 5.0)
    sc, sf, _ = limit_scenes.corner_scenes(n, 83, S, D, V, T, tf, on_road=0.6)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes, max_static=S, max_dynamic=D, max_vertices=V, max_samples=T)
    times, poses = _road_rows(sc, sf, K, dt, 5)
    cfg = api.default_dp_config()
    knots = undecided = 0
    for buffer in (0.0, 0.3):
        got = _device(opt, packed, cc.rows_in_layout(api.ROWS_TRAJ, times, poses), api.ROWS_TRAJ, cfg, buffer)
        a, b = _hold(got, _host(sf.center, sf.scenes, times, poses, cfg, buffer), (name, buffer))
        knots, undecided = knots + a, undecided + b
    print("COLLISION_AUDIT_RECORD", dict(rows=name, knots=knots, undecided=undecided, knots_hit=int((got["mask"] != 0).sum())), flush=True)
    assert undecided <= UNDECIDED_SHARE * knots, (undecided, knots)
    if n >= 3 and K >= 7:
        assert (got["mask"] != 0).any() and (got["mask"] == 0).any()


def _pack_cases(center, cases):
    """The crafted cases of one buffer as ONE batch: knots padded by repeating the last one, a polygon without vertices
    packed as a triangle whose count is then set to 0.  Returns (packed, times [B,K], poses [B,K,3], expect [B,K])."""
    K = max(len(c.times) for c in cases)
    pad = lambda a: np.concatenate([a, np.repeat(a[-1:], K - len(a), axis=0)], axis=0)
    empty_static, empty_dynamic, scenes = [], [], []
    tri = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    for b, c in enumerate(cases):
        static, dynamic = list(c.scene.static), list(c.scene.dynamic)
        for o, p in enumerate(static):
            if len(p) == 0:
                static[o] = tri + [c.poses[0, 0], c.poses[0, 1]]      # (would be hit if the count were not 0)
                empty_static.append((b, o))
        for o, d in enumerate(dynamic):
            if len(d.polygon) == 0:
                dynamic[o] = scene_io.DynamicObstacle(tri, d.trajectory)
                empty_dynamic.append((b, o))
        scenes.append(dataclasses.replace(c.scene, static=static, dynamic=dynamic))
    packed = scene_io.pack_scene_batch(center, scenes)
    for b, o in empty_static:
        packed["static_counts"][b, o] = 0
    for b, o in empty_dynamic:
        packed["dynamic_polygon_counts"][b, o] = 0
    return (packed, np.stack([pad(c.times) for c in cases]), np.stack([pad(c.poses) for c in cases]),
            np.stack([pad(c.expect) for c in cases]))


def test_crafted_cases_inside_a_batch_are_exact(opt):
    center, time_cases, geometry_cases = cc.crafted_cases()
    assert any(len(p) == 0 for c in time_cases for p in c.scene.static)
    for buffer in (0.0, 0.5):
        cases = [c for c in time_cases + geometry_cases if c.buffer == buffer]
        packed, times, poses, expect = _pack_cases(center, cases)
        for layout in (api.ROWS_TRAJ, api.ROWS_COARSE):
            rows = cc.rows_in_layout(layout, times, poses)
            for got in (_device(opt, packed, rows, layout, None, buffer), opt.check_collisions(packed, rows, layout, None, buffer)):
                assert np.array_equal(got["mask"], expect), [c.name for c, g, e in zip(cases, got["mask"], expect) if not np.array_equal(g, e)]
                hit = expect != 0
                assert np.array_equal(got["first_hit"], np.where(hit.any(axis=1), hit.argmax(axis=1), -1))
                assert np.array_equal(got["n_hit"], hit.sum(axis=1)) and got["n_colliding"] == int(hit.any(axis=1).sum())


# ---------------------------------------------------------------------------------------------------------------------
# 3. one result, however it is asked for
# ---------------------------------------------------------------------------------------------------------------------
def test_memories_layouts_batch_sizes_and_a_reused_work_space_change_no_bit(opt):
    sf, cfg, times, poses = cc.path_and_shift_rows("mix11", 48, 75, planner=opt)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    sizes = {k: packed[k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples")}
    rows = {layout: cc.rows_in_layout(layout, times, poses[:, 1]) for layout in (api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE)}
    first = opt.check_collisions(packed, rows[api.ROWS_PLAN], api.ROWS_PLAN, cfg, 0.3)
    assert (first["mask"] != 0).any() and (first["first_hit"] == -1).any()
    assert _same(_device(opt, packed, rows[api.ROWS_PLAN], api.ROWS_PLAN, cfg, 0.3), first)                 # DEVICE arrays
    for layout in rows:
        assert _same(opt.check_collisions(packed, rows[layout], layout, cfg, 0.3), first), layout           # the layouts
        assert _same(_device(opt, packed, rows[layout], layout, cfg, 0.3), first), layout
    # the optional outputs left out change nothing of the others
    lean = _device(opt, packed, rows[api.ROWS_TRAJ], api.ROWS_TRAJ, cfg, 0.3, want_mask=False, want_n_hit=False)
    assert np.array_equal(lean["first_hit"], first["first_hit"]) and lean["n_colliding"] == first["n_colliding"]
    assert (lean["mask"] == 77).all() and (lean["n_hit"] == -7).all()
    # a larger call grows the work space, a smaller one reuses it: the same call afterwards gives the same bits
    big_sf, big_cfg, big_times, big_poses = cc.path_and_shift_rows("mix11", 160, 76, planner=opt)
    big = scene_io.pack_scene_batch(big_sf.center, big_sf.scenes)
    opt.check_collisions(big, cc.rows_in_layout(api.ROWS_TRAJ, big_times, big_poses[:, 2]), api.ROWS_TRAJ, big_cfg, 0.0)
    small = scene_io.pack_scene_batch(sf.center, sf.scenes[:5], **sizes)
    part = opt.check_collisions(small, rows[api.ROWS_PLAN][:5], api.ROWS_PLAN, cfg, 0.3)
    assert np.array_equal(part["mask"], first["mask"][:5]) and np.array_equal(part["first_hit"], first["first_hit"][:5])
    assert _same(opt.check_collisions(packed, rows[api.ROWS_PLAN], api.ROWS_PLAN, cfg, 0.3), first)
    # batches of one, padded to the batch's sizes and to their own
    for b in (0, 7, 47):
        for kw in (sizes, {}):
            one = opt.check_collisions(scene_io.pack_scene_batch(sf.center, [sf.scenes[b]], **kw), rows[api.ROWS_PLAN][b:b + 1],
                                       api.ROWS_PLAN, cfg, 0.3)
            assert np.array_equal(one["mask"][0], first["mask"][b]) and one["first_hit"][0] == first["first_hit"][b]
            assert one["n_hit"][0] == first["n_hit"][b] and one["n_colliding"] == int(first["first_hit"][b] >= 0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. hostile inputs inside a batch
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_counts_and_non_finite_rows_stay_inside_their_scene(opt):
    sf, cfg, times, poses = cc.path_and_shift_rows("mix11", 12, 77, planner=opt)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    rows = cc.rows_in_layout(api.ROWS_TRAJ, times, poses[:, 1])
    good = _device(opt, packed, rows, api.ROWS_TRAJ, cfg, 0.3)
    assert (good["mask"] != 0).any()
    # DEVICE arrays carry their counts unchecked to the kernel: a count beyond the arrays marks that scene alone.  Input
    # validation, not fault injection: every index the kernel forms is bounded by the max_* of the call.
    worse = dict(packed, static_counts=packed["static_counts"].copy(), dynamic_polygon_counts=packed["dynamic_polygon_counts"].copy(),
                 dynamic_trajectory_counts=packed["dynamic_trajectory_counts"].copy())
    worse["static_counts"][3, 0] = packed["max_vertices"] + 1
    worse["dynamic_trajectory_counts"][6, 0] = 1 << 20
    worse["dynamic_polygon_counts"][9, 0] = -1
    got = _device(opt, worse, rows, api.ROWS_TRAJ, cfg, 0.3)
    bad = np.zeros(12, dtype=bool)
    bad[[3, 6, 9]] = True
    assert (got["first_hit"][bad] == -2).all() and (got["n_hit"][bad] == 0).all() and not got["mask"][bad].any()
    for k in ("mask", "first_hit", "n_hit"):
        assert np.array_equal(got[k][~bad], good[k][~bad]), k
    assert got["n_colliding"] == int((good["first_hit"][~bad] >= 0).sum())
    # a NaN pose and an Inf time in one row: the arithmetic decides, as on the host; the other knots and scenes stay
    b = int(np.flatnonzero(good["n_hit"] > 0)[0])
    wild_times, wild_poses = times.copy(), poses[:, 1].copy()
    wild_poses[b, 2, 0], wild_poses[b, 5, 2], wild_times[b, 7] = np.nan, np.nan, np.inf
    got = _device(opt, packed, cc.rows_in_layout(api.ROWS_TRAJ, wild_times, wild_poses), api.ROWS_TRAJ, cfg, 0.3)
    flat = scene_io.flatten_scene(sf.center, sf.scenes[b])
    host, _, _ = api.check_collisions(flat, cc.rows_in_layout(api.ROWS_TRAJ, wild_times[b], wild_poses[b]), api.ROWS_TRAJ, cfg, 0.3)
    touched = np.zeros(times.shape, dtype=bool)
    touched[b, [2, 5, 7]] = True
    assert np.array_equal(got["mask"][touched], host[[2, 5, 7]]) and not got["mask"][b, [2, 5]].any()
    assert not (got["mask"][b, 7] & (cc.RD | cc.FD))          # nothing is there at an infinite time
    assert np.array_equal(got["mask"][~touched], good["mask"][~touched])


# ---------------------------------------------------------------------------------------------------------------------
# 5. behind the pipeline
# ---------------------------------------------------------------------------------------------------------------------
def test_the_pipelines_plan_rows_are_audited_where_they_lie(opt):
    import torch
    dev = torch.device("cuda", 0)
    B, K, M = 128, opt.K, opt.cfg.max_iter
    sc, sf = cc.generator_scenes("mix11", B, 91)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    dp_cfg, cor_cfg = api.default_dp_config(tf=5.0), api.default_corridor_config()
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    start = torch.from_numpy(np.ascontiguousarray(sc["start"])).to(dev)
    traj = torch.zeros((B, K, 10), dtype=torch.float64, device=dev)
    hist = torch.zeros((B, M + 1, 5), dtype=torch.float64, device=dev)
    plan = torch.zeros((B, K, api.PLAN_FIELDS), dtype=torch.float64, device=dev)
    n_cost, status, n_iter, outcome = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                            n_iter.data_ptr(), None, None, None)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rc, n_dp, n_cor = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb, start.data_ptr(), K, sol, plan.data_ptr(), None, outcome.data_ptr())
    assert rc == api.OK
    mask = torch.full((B, K), 77, dtype=torch.uint8, device=dev)
    first, n_hit = (torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    rc, n_colliding = opt.check_collisions_raw(dp_cfg, sb, api.ROWS_PLAN, plan.data_ptr(), K, 0.0, mask.data_ptr(),
                                               first.data_ptr(), n_hit.data_ptr())
    torch.cuda.synchronize()
    assert rc == api.OK
    got = dict(mask=mask.cpu().numpy(), first_hit=first.cpu().numpy(), n_hit=n_hit.cpu().numpy(), n_colliding=n_colliding)
    rows, outcome = plan.cpu().numpy(), outcome.cpu().numpy()
    # the same rows through the traj layout of the solver's own output: one result
    again = _device(opt, packed, traj.cpu().numpy(), api.ROWS_TRAJ, dp_cfg, 0.0)
    assert _same(again, got)
    # the same rows, downloaded, through the host call (scenes the DP failed on are audited like any other)
    knots, undecided = _hold(got, _host(sf.center, sf.scenes, rows[:, :, 0], rows[:, :, 2:5], dp_cfg, 0.0), "plan rows")
    assert undecided <= UNDECIDED_SHARE * knots
    assert int((outcome == api.PLAN_DP_FAILED).sum()) == n_dp
    assert (got["first_hit"] >= -1).all() and got["n_colliding"] == int((got["first_hit"] >= 0).sum())
    by_status = {int(s): int((got["first_hit"][status.cpu().numpy() == s] >= 0).sum()) for s in np.unique(status.cpu().numpy())}
    print("COLLISION_AUDIT_RECORD", dict(pipeline="mix11", scenes=B, colliding=got["n_colliding"], colliding_by_status=by_status,
                                         dp_failed=n_dp, knots=knots, undecided=undecided), flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# 6. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing_and_leave_the_handle_usable(opt):
    sf, cfg, times, poses = cc.path_and_shift_rows("mix11", 16, 79, planner=opt)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    K = times.shape[1]
    reference = opt.check_collisions(packed, cc.rows_in_layout(api.ROWS_PLAN, times, poses[:, 1]), api.ROWS_PLAN, cfg, 0.3)
    L = api.lib()

    def call(handle=True, layout=api.ROWS_PLAN, n_knots=K, buffer=0.3, want_cfg=True, scenes=True, want_rows=True,
             want_first=True, edit=None, arrays=None, **sizes):
        a = dict(keep, **(arrays or {}))
        sb = api.scene_batch_struct(dict(packed, **sizes), api.MEM_HOST, **{k: a[k].ctypes.data for k in a})
        if edit:
            edit(sb)
        n = max(n_knots, 1)
        rows = cc.rows_in_layout(api.ROWS_PLAN, np.resize(times, (16, n)), np.resize(poses[:, 1], (16, n, 3)))
        mask = np.full((16, n), 77, dtype=np.uint8)
        first, n_hit, n_col = np.full(16, -7, dtype=np.int32), np.full(16, -7, dtype=np.int32), C.c_int32(-7)
        rc = L.cilqr_check_collisions_batch(opt.h if handle else None, C.byref(cfg) if want_cfg else None,
                                            C.byref(sb) if scenes else None, layout, rows.ctypes.data if want_rows else None,
                                            n_knots, C.c_double(buffer), mask.ctypes.data,
                                            first.ctypes.data if want_first else None, n_hit.ctypes.data, C.byref(n_col))
        if rc != api.OK:    # nothing was launched, nothing written
            assert (mask == 77).all() and (first == -7).all() and (n_hit == -7).all() and n_col.value == -7
        return rc

    assert call() == api.OK
    for what in ("handle", "want_cfg", "scenes", "want_rows", "want_first"):
        assert call(**{what: False}) == api.ERR_NULL, what
    for field in ("center", "static_points", "static_counts", "dynamic_polygon_points", "dynamic_polygon_counts",
                  "dynamic_trajectories", "dynamic_trajectory_counts"):
        assert call(edit=lambda sb, f=field: setattr(sb, f, None)) == api.ERR_NULL, field
    assert call(edit=lambda sb: setattr(sb, "batch", 0)) == api.ERR_ARG
    assert call(edit=lambda sb: setattr(sb, "n_center", 1)) == api.ERR_ARG
    assert call(edit=lambda sb: setattr(sb, "memory", 5)) == api.ERR_ARG
    assert call(edit=lambda sb: setattr(sb, "max_static", -1)) == api.ERR_ARG
    assert call(layout=3) == api.ERR_ARG and call(layout=-1) == api.ERR_ARG
    assert call(n_knots=0) == api.ERR_ARG
    for bad in (-1e-300, -0.5, np.inf, -np.inf, np.nan):
        assert call(buffer=bad) == api.ERR_ARG, bad
    for name, lim in (("max_vertices", api.DP_MAX_VERTICES), ("max_static", api.DP_MAX_STATIC),
                      ("max_dynamic", api.DP_MAX_DYNAMIC), ("max_samples", api.DP_MAX_SAMPLES)):
        assert call(**{name: lim + 1}) == api.ERR_CAPACITY, name
    assert call(n_knots=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    for name, bad in (("static_counts", packed["max_vertices"] + 1), ("static_counts", -1),
                      ("dynamic_polygon_counts", packed["max_vertices"] + 1), ("dynamic_polygon_counts", -2),
                      ("dynamic_trajectory_counts", packed["max_samples"] + 1), ("dynamic_trajectory_counts", -1)):
        a = keep[name].copy()
        a[3, 0] = bad
        assert call(arrays={name: a}) == api.ERR_ARG, (name, bad)
    # solves submitted on the handle
    g = scenario.generate("mix11", 64, seed=3)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=64, cmax=g["cmax"]) as busy:
        prob, keep_p = busy._host_problem(g)
        B, M = 64, busy.cfg.max_iter
        traj, hist = np.zeros((B, 51, 10)), np.zeros((B, M + 1, 5))
        nc, st, ni = (np.zeros(B, dtype=np.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_HOST, 0, traj.ctypes.data, hist.ctypes.data, nc.ctypes.data, st.ctypes.data,
                                ni.ctypes.data, None, None, None)
        assert busy.L.cilqr_submit(busy.h, C.byref(prob), C.byref(sol)) == api.OK
        with pytest.raises(api.CilqrError) as e:
            busy.check_collisions(packed, cc.rows_in_layout(api.ROWS_PLAN, times, poses[:, 1]), api.ROWS_PLAN, cfg, 0.3)
        assert e.value.code == api.ERR_STATE
        assert busy.L.cilqr_wait(busy.h) == api.OK
        assert _same(busy.check_collisions(packed, cc.rows_in_layout(api.ROWS_PLAN, times, poses[:, 1]), api.ROWS_PLAN, cfg, 0.3), reference)
    assert _same(opt.check_collisions(packed, cc.rows_in_layout(api.ROWS_PLAN, times, poses[:, 1]), api.ROWS_PLAN, cfg, 0.3), reference)
