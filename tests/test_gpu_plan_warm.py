"""cilqr_plan_scenes_batch_warm on the GPU: the pipeline with a warm start against the four public calls made one after the
other with cilqr_solve_batch_warm last -- bit for bit, HOST and DEVICE arrays, the three warm layouts, a scene whose DP fails
in the batch --; all shifts negative and warm = NULL against the plain pipeline; the first iterate carries the warm controls;
every refusal leaves the outputs unwritten."""
import dataclasses

import numpy as np
import pytest

import scene_window_cases as sw
from cilqr_amd import api, scenario, scene_io

pytestmark = pytest.mark.gpu
B, WALLED = 5, 3
SOLVED = ("traj", "status", "n_cost", "cost_hist", "n_iter", "iter_trajs", "n_iter_trajs")
SHIFT = np.array([5, 0, -1, 2, 1], dtype=np.int32)


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def world():
    """five mix11 scenes, a wall across the road where the ego of scene WALLED stands (its DP finds no path), the handle and
    the cold pipeline's result: computed once, read by every test"""
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, B, seed=91, scenarios=True)
    sf = scene_io.from_generator(sc)
    scenes = list(sf.scenes)
    x0, y0, th = sc["start"][WALLED][:3]
    c, s_ = np.cos(th), np.sin(th)
    wall = np.array([[1.0, 9.0], [1.0, -9.0], [-1.0, -9.0], [-1.0, 9.0]])
    scenes[WALLED] = dataclasses.replace(scenes[WALLED], static=list(scenes[WALLED].static) + [
        np.stack([x0 + wall[:, 0] * c - wall[:, 1] * s_, y0 + wall[:, 0] * s_ + wall[:, 1] * c], 1)])
    packed = scene_io.pack_scene_batch(sf.center, scenes)
    start = np.ascontiguousarray(sc["start"], dtype=np.float64)
    dp_cfg, cor_cfg = api.default_dp_config(tf=5.0), api.default_corridor_config()
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=B, cmax=16, max_lane_segments=256) as opt:
        cold = _pipeline(opt, packed, start, dp_cfg, cor_cfg, None, api.MEM_HOST)
        assert cold["rc"] == api.OK and cold["outcome"][WALLED] == api.PLAN_DP_FAILED and (cold["outcome"] == 0).sum() >= 2
        yield dict(opt=opt, center=sf.center, packed=packed, start=start, dp_cfg=dp_cfg, cor_cfg=cor_cfg, cold=cold)


def _outputs(n, K, M, fill):
    o = dict(traj=np.full((n, K, 10), fill), cost_hist=np.full((n, M + 1, 5), fill), plan=np.full((n, K, api.PLAN_FIELDS), fill),
             dp=np.full((n, K, 9), fill), iter_trajs=np.full((n, 2, K, 10), fill))
    for k in ("n_cost", "status", "n_iter", "outcome", "n_iter_trajs"):
        o[k] = np.full(n, -9, dtype=np.int32)
    return o


def _pipeline(opt, packed, start, dp_cfg, cor_cfg, warm, memory, fill=0.0):
    """cilqr_plan_scenes_batch(_warm) through the pointer-level form, every array in `memory`; warm = None or (rows, shift,
    layout) of NumPy arrays.  Returns the outputs (NumPy) with rc."""
    n, K, M = packed["batch"], opt.K, opt.cfg.max_iter
    o = _outputs(n, K, M, fill)
    if memory == api.MEM_DEVICE:
        import torch
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ptr = lambda t: t.data_ptr()
    else:
        up = lambda a: np.ascontiguousarray(a)
        ptr = lambda a: a.ctypes.data
    t = {k: up(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    d = {k: up(v) for k, v in o.items()}
    t_start = up(start)
    sb = api.scene_batch_struct(packed, memory, **{k: ptr(t[k]) for k in t})
    sol = api.SolutionBatch(memory, 2, ptr(d["traj"]), ptr(d["cost_hist"]), ptr(d["n_cost"]), ptr(d["status"]), ptr(d["n_iter"]),
                            ptr(d["iter_trajs"]), ptr(d["n_iter_trajs"]), None)
    w = None
    if warm is not None:
        w_rows = up(np.asarray(warm[0], dtype=np.float64))
        w_shift = None if warm[1] is None else up(np.asarray(warm[1], dtype=np.int32))
        w = api.WarmStart(memory, int(warm[2]), ptr(w_rows), None if w_shift is None else ptr(w_shift))
    if memory == api.MEM_DEVICE:
        torch.cuda.synchronize()
    rc, n_dp, n_cor = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb, ptr(t_start), K, sol, ptr(d["plan"]), ptr(d["dp"]),
                                          ptr(d["outcome"]), warm=w)
    if memory == api.MEM_DEVICE:
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy() for k, v in d.items()}
    return dict(d, rc=rc, n_dp_failed=n_dp, n_corridor_failed=n_cor)


def _chain(w, warm):
    """the four public calls one after the other, HOST arrays, cilqr_solve_batch_warm last"""
    opt, packed, start = w["opt"], w["packed"], w["start"]
    r = opt.dp_plan_batch(packed, start, w["dp_cfg"])
    times = r["dp"][int(np.flatnonzero(r["found"])[0])][:, 0]
    pts, cnt, _ = opt.scene_points(packed, times, multiple_sample=bool(w["cor_cfg"].is_multiple_sample))
    cor, ccnt, _ = opt.build_corridors(r["knots"], pts, cnt, cmax=opt.cmax, cfg=w["cor_cfg"])
    left, right = api.road_barriers(w["center"])
    seg = w["cor_cfg"].lane_segment_length
    sol = opt.plan(dict(start=start, coarse=r["coarse"], corridor=cor, ccount=ccnt, left=api.lane_constraints(left, seg, True),
                        right=api.lane_constraints(right, seg, False), coarse_station=r["station"]), max_iter_trajs=2, warm=warm)
    return dict(sol, found=r["found"])


def _warm_rows(cold, layout, N):
    return {api.ROWS_TRAJ: cold["traj"], api.ROWS_PLAN: cold["plan"],
            api.ROWS_CONTROLS: np.ascontiguousarray(cold["traj"][:, :N, 8:10])}[layout]


@pytest.mark.parametrize("layout", [api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_CONTROLS], ids=["traj", "plan", "controls"])
def test_the_warm_pipeline_is_the_chain_with_a_warm_solve(world, layout):
    w, cold = world, world["cold"]
    N = w["opt"].N
    warm = (_warm_rows(cold, layout, N), SHIFT, layout)
    chain = _chain(w, warm)
    found = chain["found"]
    assert not found[WALLED] and found.sum() == B - 1
    host = _pipeline(w["opt"], w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"], warm, api.MEM_HOST)
    dev = _pipeline(w["opt"], w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"], warm, api.MEM_DEVICE)
    assert host["rc"] == api.OK and dev["rc"] == api.OK
    for k in SOLVED:
        got, want = host[k][found], chain[k][found]
        if k == "iter_trajs":      # entries behind n_iter_trajs are unspecified
            filled = np.minimum(chain["n_iter_trajs"][found], 2)
            got = np.concatenate([g[:n].ravel() for g, n in zip(got, filled)])
            want = np.concatenate([g[:n].ravel() for g, n in zip(want, filled)])
        assert sw.same_bits(got, want), k
    for k in SOLVED + ("plan", "dp", "outcome"):
        if k == "iter_trajs":
            for b in range(B):
                n = min(int(host["n_iter_trajs"][b]), 2)
                assert sw.same_bits(dev[k][b, :n], host[k][b, :n]), (k, b)
        else:
            assert sw.same_bits(dev[k], host[k]), k
    assert (host["n_dp_failed"], host["n_corridor_failed"]) == (cold["n_dp_failed"], cold["n_corridor_failed"]) == \
        (dev["n_dp_failed"], dev["n_corridor_failed"])
    assert np.array_equal(host["outcome"], cold["outcome"]) and sw.same_bits(host["dp"], cold["dp"])
    # the scene with shift < 0 has the bits of the cold pipeline; the scene that is not optimised ends as it does there
    b = int(np.flatnonzero(SHIFT < 0)[0])
    for k in ("traj", "status", "n_cost", "cost_hist", "plan", "n_iter"):
        assert sw.same_bits(host[k][b], cold[k][b]), k
    assert host["status"][WALLED] == api.ST_NO_CORRIDOR and host["n_cost"][WALLED] == 1
    # the first iterate carries the warm controls: U_i = the controls of row i + shift, zeros past the end
    controls = cold["traj"][:, :, 8:10]
    changed = 0
    for b in np.flatnonzero((SHIFT >= 0) & (cold["outcome"] == 0)):
        want = np.zeros((N, 2))
        want[:N - SHIFT[b]] = controls[b, SHIFT[b]:N]
        assert host["n_iter_trajs"][b] >= 1 and sw.same_bits(host["iter_trajs"][b, 0, :N, 8:10], want), b
        assert sw.same_bits(host["iter_trajs"][b, 0, 0, 1:5], w["start"][b])
        changed += not sw.same_bits(host["iter_trajs"][b, 0], cold["iter_trajs"][b, 0])
    assert changed >= 1


def test_no_warm_start_is_the_plain_pipeline(world):
    w, cold = world, world["cold"]
    args = (w["opt"], w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"])
    all_cold = (cold["traj"], np.full(B, -1, np.int32), api.ROWS_TRAJ)
    for memory in (api.MEM_HOST, api.MEM_DEVICE):
        plain = _pipeline(*args, None, memory)
        shifted = _pipeline(*args, all_cold, memory)
        for k in ("traj", "status", "n_cost", "cost_hist", "n_iter", "plan", "dp", "outcome", "n_iter_trajs"):
            assert sw.same_bits(plain[k], cold[k]), (k, memory)                # warm = NULL: cilqr_plan_scenes_batch
            assert sw.same_bits(shifted[k], cold[k]), (k, memory)              # every shift < 0
    # the Python form: warm=None is the call it was, warm=(...) the warm one
    py_cold = w["opt"].plan_scenes(w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"])
    py_warm = w["opt"].plan_scenes(w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"], warm=(cold["traj"], SHIFT, api.ROWS_TRAJ))
    host = _pipeline(*args, (cold["traj"], SHIFT, api.ROWS_TRAJ), api.MEM_HOST)
    for k in ("traj", "status", "n_cost", "cost_hist", "plan", "dp", "outcome"):
        assert sw.same_bits(py_cold[k], cold[k]) and sw.same_bits(py_warm[k], host[k]), k
    assert not sw.same_bits(py_warm["cost_hist"], py_cold["cost_hist"])


def test_every_refusal_leaves_the_outputs_unwritten(world):
    w, cold = world, world["cold"]
    opt, N = w["opt"], world["opt"].N
    args = (opt, w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"])
    K, M = opt.K, opt.cfg.max_iter

    def refused(warm_struct, memory=api.MEM_HOST):
        o = _outputs(B, K, M, -5.5)
        keep = {k: np.ascontiguousarray(w["packed"][k]) for k in api._SCENE_BATCH_ARRAYS}
        sb = api.scene_batch_struct(w["packed"], memory, **{k: keep[k].ctypes.data for k in keep})
        sol = api.SolutionBatch(api.MEM_HOST, 2, o["traj"].ctypes.data, o["cost_hist"].ctypes.data, o["n_cost"].ctypes.data,
                                o["status"].ctypes.data, o["n_iter"].ctypes.data, o["iter_trajs"].ctypes.data,
                                o["n_iter_trajs"].ctypes.data, None)
        rc, _, _ = opt.plan_scenes_raw(w["dp_cfg"], w["cor_cfg"], sb, w["start"].ctypes.data, K, sol, o["plan"].ctypes.data,
                                       o["dp"].ctypes.data, o["outcome"].ctypes.data, warm=warm_struct)
        for k, v in o.items():
            assert (v == (-5.5 if v.dtype == np.float64 else -9)).all(), k
        return rc
    rows, shift = np.ascontiguousarray(cold["traj"]), SHIFT.copy()
    W = lambda memory, layout, r, s: api.WarmStart(memory, layout, r, s)
    assert refused(W(api.MEM_HOST, api.ROWS_TRAJ, None, shift.ctypes.data)) == api.ERR_NULL
    assert refused(W(api.MEM_HOST, api.ROWS_COARSE, rows.ctypes.data, None)) == api.ERR_ARG
    assert refused(W(api.MEM_HOST, 17, rows.ctypes.data, None)) == api.ERR_ARG
    assert refused(W(api.MEM_DEVICE, api.ROWS_TRAJ, rows.ctypes.data, None)) == api.ERR_ARG      # not where the scenes are
    assert refused(W(5, api.ROWS_TRAJ, rows.ctypes.data, None)) == api.ERR_ARG
    # the handle is as usable as before
    again = _pipeline(*args, (cold["traj"], None, api.ROWS_TRAJ), api.MEM_HOST)
    zero = _pipeline(*args, (cold["traj"], np.zeros(B, np.int32), api.ROWS_TRAJ), api.MEM_HOST)
    assert again["rc"] == api.OK and sw.same_bits(again["traj"], zero["traj"])                    # a NULL shift array: 0 for all
