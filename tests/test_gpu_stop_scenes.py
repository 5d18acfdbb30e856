"""cilqr_stop_scenes_batch (stop_pipeline.hip) against the public calls made one after the other -- stop_rows, one
check_collisions per profile, the selection written here in NumPy -- bit for bit, and the slices of a stop_rows result as
input of the other row consumers where they lie.

The scenes are crafted on a straight road along x: the ego heads along +x at 8 m/s, so every sine and cosine is exact on host
and device, and the three profiles stop after about 34 m, 18 m and 7 m.  A static polygon across the path at distance D
decides which of them stop clear; one scene has a dynamic polygon that arrives where the gentle profile stands, after it has
stopped; one starts too fast for the gentle profile to stop on the path (its status decides, not the audit)."""
import numpy as np
import pytest

import collision_cases as cc
import stop_cases as sc
from cilqr_amd import api, scenario, scene_io, stop

pytestmark = pytest.mark.gpu

PROFILES = np.array([sc.GENTLE, sc.FIRM, sc.HARD])
K, N, DT, BUFFER = 61, 51, 0.2, 0.3


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=128, cmax=16, max_lane_segments=256) as o:
        yield o


def _wall(d):
    # (narrower than a disc's square: the audit's overlap test asks for a vertex of one inside the other)
    return np.array([[d, 1.0], [d, -1.0], [d + 1.0, -1.0], [d + 1.0, 1.0]])


def crafted(B):
    """(centre line, scenes, rows [B,K,11], start_va [B,2], the kind of every scene)"""
    center = cc.straight_center(length=80.0)
    kinds = ("open", "wall_30", "wall_15", "wall_5", "arrives_late", "too_fast")
    scenes, va, names = [], np.zeros((B, 2)), []
    for b in range(B):
        kind = kinds[(b + 2) % len(kinds)] if B > 1 else "wall_15"
        shift = 0.01 * (b // len(kinds))
        static, dynamic = [], []
        va[b] = (8.0, 0.0)
        if kind.startswith("wall"):
            static = [_wall(float(kind[5:]) + shift)]
        elif kind == "arrives_late":     # the gentle profile stands at x = 36.06 from t = 8.4 s on; the others stopped long before
            body = np.array([[0.5, 0.5], [0.5, -0.5], [-0.5, -0.5], [-0.5, 0.5]])
            samples = np.array([[0.0, 36.0 + shift, 40.0, 0.0], [9.0, 36.0 + shift, 40.0, 0.0], [9.2, 36.0 + shift, 0.0, 0.0],
                                [20.0, 36.0 + shift, 0.0, 0.0]])
            dynamic = [scene_io.DynamicObstacle(body, samples)]
        elif kind == "too_fast":
            va[b] = (11.5, 0.0)              # 11.5 m/s at -1 m/s^2 needs more than the 60 m of the path
        scenes.append(scene_io.Scene(np.zeros(4), np.zeros((1, 6)), static, dynamic))
        names.append(kind)
    rows = np.repeat(sc.straight(K, 1.0, v=8.0, a=0.0)[None], B, axis=0)
    rows[:, :, 2] += 2.0                     # the path begins at x = 2: the rear disc stays on the road's table
    return center, scenes, rows, va, names


def host_choice(center, scenes, rows, va, cfg):
    """choice [B] by the host calls alone: api.stop_rows, api.check_collisions, the selection"""
    out = np.zeros(len(scenes), np.int32)
    for b, scene in enumerate(scenes):
        got = api.stop_rows(rows[b], api.ROWS_PLAN, PROFILES, DT, N, va[b])
        flat = scene_io.flatten_scene(center, scene)
        hits = [api.check_collisions(flat, got["rows"][m], api.ROWS_PLAN, cfg, BUFFER)[1] for m in range(len(PROFILES))]
        out[b] = stop.choose(got["status"], hits)
    return out


@pytest.mark.parametrize("B, memory", [(1, api.MEM_HOST), (65, api.MEM_HOST), (65, api.MEM_DEVICE), (257, api.MEM_HOST),
                                       (257, api.MEM_DEVICE), (1, api.MEM_DEVICE)])
def test_pipeline_equals_the_public_calls_one_after_the_other(opt, B, memory):
    cfg = api.default_dp_config()
    center, scenes, rows, va, names = crafted(B)
    expect = host_choice(center, scenes, rows, va, cfg)
    if B > 1:        # the scenes do make every choice, by the host audit, before the GPU result is looked at
        assert set(expect.tolist()) == {-1, 0, 1, 2}
        by_kind = {k: set(expect[[i for i, n in enumerate(names) if n == k]].tolist()) for k in set(names)}
        assert by_kind == {"open": {0}, "wall_30": {1}, "wall_15": {2}, "wall_5": {-1}, "arrives_late": {1}, "too_fast": {1}}
    packed = scene_io.pack_scene_batch(center, scenes)
    M = len(PROFILES)
    # ---- the composition
    parts = opt.stop_rows(rows, api.ROWS_PLAN, PROFILES, DT, N, va)
    first = np.stack([opt.check_collisions(packed, parts["rows"][m], api.ROWS_PLAN, cfg, BUFFER)["first_hit"] for m in range(M)])
    choice = np.array([stop.choose(parts["status"][:, b], first[:, b]) for b in range(B)], np.int32)
    want_rows = np.stack([parts["rows"][choice[b] if choice[b] >= 0 else M - 1, b] for b in range(B)])
    too_fast = [b for b, n in enumerate(names) if n == "too_fast"]
    assert (parts["status"][0, too_fast] == stop.OVERRUN).all() and (first[0, too_fast] == -1).all()
    # ---- the pipeline
    if memory == api.MEM_HOST:
        got = opt.stop_scenes(packed, rows, api.ROWS_PLAN, PROFILES, DT, N, va, cfg, BUFFER)
    else:
        import torch
        dev = torch.device("cuda", 0)
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        keep = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
        sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: v.data_ptr() for k, v in keep.items()})
        d_rows, d_va = torch.from_numpy(rows).to(dev), torch.from_numpy(va).to(dev)
        d_out = torch.empty((B, N, 11), dtype=torch.float64, device=dev)
        d_choice = torch.empty((B,), dtype=torch.int32, device=dev)
        d_status, d_first = (torch.empty((M, B), dtype=torch.int32, device=dev) for _ in range(2))
        code, n_none = opt.stop_scenes_raw(cfg, sb, api.ROWS_PLAN, d_rows.data_ptr(), K, PROFILES, d_va.data_ptr(), DT, N, BUFFER,
                                           d_out.data_ptr(), d_choice.data_ptr(), d_status.data_ptr(), d_first.data_ptr())
        assert code == api.OK
        got = dict(rows=d_out.cpu().numpy(), choice=d_choice.cpu().numpy(), status=d_status.cpu().numpy(),
                   first_hit=d_first.cpu().numpy(), n_none=n_none)
        # ... and without the two optional outputs
        d_out2, d_choice2 = torch.empty_like(d_out), torch.empty_like(d_choice)
        code, n2 = opt.stop_scenes_raw(cfg, sb, api.ROWS_PLAN, d_rows.data_ptr(), K, PROFILES, d_va.data_ptr(), DT, N, BUFFER,
                                       d_out2.data_ptr(), d_choice2.data_ptr())
        assert code == api.OK and n2 == n_none and torch.equal(d_choice2, d_choice)
        assert d_out2.cpu().numpy().tobytes() == got["rows"].tobytes()
        # ... and through the method that takes device tensors: the scene arrays uploaded by it, then resident ones
        for scene_arrays in (packed, dict(packed, **keep)):
            dev_got = opt.stop_scenes(scene_arrays, d_rows, api.ROWS_PLAN, PROFILES, DT, N, d_va, cfg, BUFFER)
            assert dev_got["rows"].is_cuda and dev_got["choice"].dtype == torch.int32 and dev_got["n_none"] == n_none
            for k in ("rows", "choice", "status", "first_hit"):
                assert dev_got[k].cpu().numpy().tobytes() == np.ascontiguousarray(got[k]).tobytes(), k
    assert np.array_equal(got["status"], parts["status"]) and np.array_equal(got["first_hit"], first)
    assert np.array_equal(got["choice"], choice) and got["n_none"] == int((choice < 0).sum())
    assert got["rows"].tobytes() == want_rows.tobytes()
    assert np.array_equal(got["choice"], expect)         # wide margins and exact headings: the host audit agrees


def test_argument_checks_are_those_of_both_calls(opt):
    cfg = api.default_dp_config()
    center, scenes, rows, va, _ = crafted(3)
    packed = scene_io.pack_scene_batch(center, scenes)
    keep = {k: np.ascontiguousarray(v) for k, v in packed.items() if isinstance(v, np.ndarray)}
    out, choice = np.full((3, N, 11), -7.0), np.full(3, -9, np.int32)

    def call(layout=api.ROWS_PLAN, rows_ptr=rows.ctypes.data, n_knots=K, profiles=PROFILES, dt=DT, n_out=N, buffer=BUFFER,
             out_ptr=out.ctypes.data, choice_ptr=choice.ctypes.data, **sizes):
        sb = api.scene_batch_struct(dict(packed, **sizes), api.MEM_HOST, **{k: api._ptr(keep[k]) for k in api._SCENE_BATCH_ARRAYS})
        code, _ = opt.stop_scenes_raw(cfg, sb, layout, rows_ptr, n_knots, profiles, va.ctypes.data, dt, n_out, buffer, out_ptr,
                                      choice_ptr)
        if code != api.OK:
            assert (out == -7.0).all() and (choice == -9).all()
        return code

    assert call(rows_ptr=None) == api.ERR_NULL and call(out_ptr=None) == api.ERR_NULL and call(choice_ptr=None) == api.ERR_NULL
    assert call(layout=3) == api.ERR_ARG and call(n_knots=1) == api.ERR_ARG and call(n_out=0) == api.ERR_ARG
    assert call(dt=0.0) == api.ERR_ARG and call(profiles=np.array([[1.0, -1.0]])) == api.ERR_ARG
    assert call(buffer=-0.1) == api.ERR_ARG and call(buffer=float("nan")) == api.ERR_ARG
    assert call(batch=0) == api.ERR_ARG
    assert call(n_out=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY and call(max_vertices=api.DP_MAX_VERTICES + 1) == api.ERR_CAPACITY
    assert call() == api.OK and (choice != -9).all()


def test_a_slice_feeds_the_other_row_consumers_where_it_lies(opt):
    """slice m of a stop_rows result, a view into the profile-major array, against the same rows copied to a fresh array"""
    import torch
    cfg = api.default_dp_config()
    B = 8
    center, scenes, rows, va, _ = crafted(B)
    packed = scene_io.pack_scene_batch(center, scenes)
    parts = opt.stop_rows(rows, api.ROWS_PLAN, PROFILES, DT, N, va)
    g = scenario.generate("mix11", B, seed=4)
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    d_parts = opt.stop_rows(torch.from_numpy(rows).to(dev), api.ROWS_PLAN, PROFILES, DT, N, torch.from_numpy(va).to(dev))
    assert d_parts["rows"].cpu().numpy().tobytes() == parts["rows"].tobytes()
    queries = torch.linspace(0.0, 20.0, 33, dtype=torch.float64, device=dev)
    for m in (1, 2):
        view = parts["rows"][m]
        assert view.base is not None and view.flags["C_CONTIGUOUS"] and view.ctypes.data != parts["rows"].ctypes.data
        a, z = opt.clearance(packed, view, api.ROWS_PLAN, cfg), opt.clearance(packed, view.copy(), api.ROWS_PLAN, cfg)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(z[k]).tobytes() for k in a)
        a, z = opt.constraint_margins(g, view, api.ROWS_PLAN), opt.constraint_margins(g, view.copy(), api.ROWS_PLAN)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(z[k]).tobytes() for k in a)
        d_view = d_parts["rows"][m]
        assert d_view.is_contiguous() and d_view.data_ptr() != d_parts["rows"].data_ptr()
        (driven_a, ok_a), (driven_z, ok_z) = opt.track(d_view, api.ROWS_PLAN, n_drive=10), opt.track(d_view.clone(), api.ROWS_PLAN, n_drive=10)
        assert torch.equal(ok_a, ok_z) and driven_a.cpu().numpy().tobytes() == driven_z.cpu().numpy().tobytes()
        r_a = opt.resample(d_view, api.ROWS_PLAN, queries, api.KEY_STATION)
        r_z = opt.resample(d_view.clone(), api.ROWS_PLAN, queries, api.KEY_STATION)
        assert r_a.cpu().numpy().tobytes() == r_z.cpu().numpy().tobytes()
