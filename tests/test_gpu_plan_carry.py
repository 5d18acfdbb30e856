"""cilqr_plan_scenes_batch_carry on the GPU: the pipeline of a later cycle against the public calls made one after the other
-- cilqr_carry_rows_batch, cilqr_check_collisions_batch, the selection rule on the host, cilqr_dp_plan_batch on the listed
scenes as a batch of their own, the merge, cilqr_scene_points_batch, cilqr_build_corridors, cilqr_solve_batch_warm -- bit
for bit, HOST and DEVICE arrays, warm and not warm.  Seven mix11 scenes windowed at scene time 0.5, one population of the
selection per scene (tests/plan_carry_cases.py settles them on the CPU): two kept, five for the DP planner."""
import numpy as np
import pytest

import plan_carry_cases as pc
import scene_window_cases as sw
from cilqr_amd import api, carry

pytestmark = pytest.mark.gpu
B, K = pc.B, pc.K
SOLVED = ("traj", "status", "n_cost", "cost_hist", "n_iter")
ALL = SOLVED + ("plan", "dp", "outcome", "source")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def world():
    """the scenes, the handle, the cold pipeline's result and the chain's: computed once, read by every test"""
    w = pc.build()
    assert np.array_equal(w["source"], pc.WANT), w["source"]          # every population, settled by the host calls
    cor_cfg = api.default_corridor_config()
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=B, cmax=16, max_lane_segments=256) as opt:
        w.update(opt=opt, cor_cfg=cor_cfg)
        w["cold"] = run(w, None, None, api.MEM_HOST)
        assert w["cold"]["rc"] == api.OK and (w["cold"]["outcome"] == 0).sum() >= 4
        yield w


def spec(w, rows=None, layout=api.ROWS_COARSE, advance=None, max_advance=pc.MAX_ADVANCE, offset=pc.MAX_START_OFFSET,
         buffer=pc.BUFFER):
    return dict(rows=w["rows"] if rows is None else rows, layout=layout, advance=w["advance"] if advance is None else advance,
                max_advance=max_advance, max_start_offset=offset, collision_buffer=buffer)


def outputs(fill):
    M = 200
    o = dict(traj=np.full((B, K, 10), fill), cost_hist=np.full((B, M + 1, 5), fill), plan=np.full((B, K, api.PLAN_FIELDS), fill),
             dp=np.full((B, K, 9), fill))
    for k in ("n_cost", "status", "n_iter", "outcome", "source"):
        o[k] = np.full(B, -9, dtype=np.int32)
    return o


def run(w, cy, warm, memory, fill=0.0, carry_struct=None, packed=None):
    """cilqr_plan_scenes_batch_carry (cy = a spec) or _warm (cy = None) through the pointer-level form, every array in
    `memory`; warm = None or (rows, shift, layout).  Returns the outputs (NumPy) with rc, the counts and n_kept."""
    opt, packed = w["opt"], packed or w["packed"]
    assert opt.cfg.max_iter == 200
    o = outputs(fill)
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
    t_start = up(w["start"])
    sb = api.scene_batch_struct(packed, memory, **{k: ptr(t[k]) for k in t})
    sol = api.SolutionBatch(memory, 0, ptr(d["traj"]), ptr(d["cost_hist"]), ptr(d["n_cost"]), ptr(d["status"]), ptr(d["n_iter"]),
                            None, None, None)
    ws = None
    if warm is not None:
        w_rows, w_shift = up(np.asarray(warm[0], dtype=np.float64)), up(np.asarray(warm[1], dtype=np.int32))
        ws = api.WarmStart(memory, int(warm[2]), ptr(w_rows), ptr(w_shift))
    cs = carry_struct
    if cy is not None and cs is None:
        c_rows, c_adv = up(np.asarray(cy["rows"], dtype=np.float64)), up(np.asarray(cy["advance"], dtype=np.float64))
        cs = api.Carry(memory, cy["layout"], int(c_rows.shape[1]), 0, ptr(c_rows), ptr(c_adv), cy["max_advance"],
                       cy["max_start_offset"], cy["collision_buffer"])
    if memory == api.MEM_DEVICE:
        torch.cuda.synchronize()
    res = opt.plan_scenes_raw(w["dp_cfg"], w["cor_cfg"], sb, ptr(t_start), K, sol, ptr(d["plan"]), ptr(d["dp"]), ptr(d["outcome"]),
                              warm=ws, carry=cs, source_ptr=ptr(d["source"]) if cs is not None else None)
    if memory == api.MEM_DEVICE:
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy() for k, v in d.items()}
    return dict(d, rc=res[0], n_dp_failed=res[1], n_corridor_failed=res[2], n_kept=res[3] if len(res) > 3 else None)


def chain(w, cy, warm):
    """the public calls one after the other, HOST arrays"""
    opt, packed, start = w["opt"], w["packed"], w["start"]
    c = opt.carry(cy["rows"], cy["layout"], cy["advance"], cy["max_advance"], K, pc.DT)
    hits = opt.check_collisions(packed, c["coarse9"], api.ROWS_COARSE, w["dp_cfg"], cy["collision_buffer"])["first_hit"]
    source = np.array([carry.source_of(c["state"][b], start[b, :2], c["coarse9"][b, 0, 2:4], hits[b], cy["max_start_offset"])
                       for b in range(B)], dtype=np.int32)
    sel = np.flatnonzero(source)
    dp, coarse, knots, station = c["coarse9"].copy(), c["coarse6"].copy(), c["knots3"].copy(), c["station"].copy()
    found = np.ones(B, dtype=bool)
    if len(sel):      # the listed scenes as a batch of their own, with the batch's max_*
        sub = dict(packed, batch=len(sel), **{k: np.ascontiguousarray(packed[k][sel]) for k in api._SCENE_BATCH_ARRAYS})
        r = opt.dp_plan_batch(sub, start[sel], w["dp_cfg"])
        dp[sel], coarse[sel], knots[sel], station[sel], found[sel] = r["dp"], r["coarse"], r["knots"], r["station"], r["found"]
    pts, cnt, _ = opt.scene_points(packed, pc.DT * np.arange(K), multiple_sample=bool(w["cor_cfg"].is_multiple_sample))
    cor, ccnt, _ = opt.build_corridors(knots, pts, cnt, cmax=opt.cmax, cfg=w["cor_cfg"])
    left, right = api.road_barriers(w["center"])
    seg = w["cor_cfg"].lane_segment_length
    sol = opt.plan(dict(start=start, coarse=coarse, corridor=cor, ccount=ccnt, left=api.lane_constraints(left, seg, True),
                        right=api.lane_constraints(right, seg, False), coarse_station=station), warm=warm)
    return dict(sol, dp=dp, found=found, source=source, sel=sel)


def same(got, want, keys, what, mask=None):
    for k in keys:
        g, x = (got[k], want[k]) if mask is None else (got[k][mask], want[k][mask])
        assert sw.same_bits(g, x), (what, k)


@pytest.mark.parametrize("warm", [False, True], ids=["cold solve", "warm solve"])
def test_the_carry_pipeline_is_the_chain_of_public_calls(world, warm):
    w, cold = world, world["cold"]
    shift = np.where(cold["outcome"] == 0, 4, -1).astype(np.int32)
    warm = (cold["traj"], shift, api.ROWS_TRAJ) if warm else None
    cy = spec(w)
    want = chain(w, cy, warm)
    assert np.array_equal(want["source"], pc.WANT)                     # the device audit agrees with the host's
    assert list(want["sel"]) == [0, 3, 4, 5, 6]
    host, dev = run(w, cy, warm, api.MEM_HOST), run(w, cy, warm, api.MEM_DEVICE)
    assert host["rc"] == api.OK and dev["rc"] == api.OK
    same(dev, host, ALL, "device arrays against host arrays")
    assert host["n_kept"] == dev["n_kept"] == 2
    assert (host["n_dp_failed"], host["n_corridor_failed"]) == (dev["n_dp_failed"], dev["n_corridor_failed"])
    assert np.array_equal(host["source"], want["source"]) and sw.same_bits(host["dp"], want["dp"])
    assert np.array_equal(host["outcome"] == api.PLAN_DP_FAILED, ~want["found"]) and host["n_dp_failed"] == (~want["found"]).sum()
    solved = want["found"] & (host["outcome"] == 0)
    assert solved[[pc.KEPT_A, pc.KEPT_B]].all() and solved.sum() >= 4
    same(host, want, SOLVED, "pipeline against chain", solved)
    # a kept scene starts from the carried rows, a listed scene from the DP planner's: those of the cold pipeline
    for b in (pc.KEPT_A, pc.KEPT_B):
        assert sw.same_bits(host["dp"][b], w["carried"][b]) and not sw.same_bits(host["dp"][b], cold["dp"][b])
    for b in want["sel"]:
        assert sw.same_bits(host["dp"][b], cold["dp"][b]), b
    if warm is None:      # ... and with a cold solve their whole result is the cold pipeline's
        same(host, cold, SOLVED + ("plan", "outcome"), "listed scenes against the cold pipeline", want["sel"])


def test_no_carry_is_the_warm_pipeline(world):
    w, cold = world, world["cold"]
    shift = np.where(cold["outcome"] == 0, 4, -1).astype(np.int32)
    warm = (cold["traj"], shift, api.ROWS_TRAJ)
    keys = SOLVED + ("plan", "dp", "outcome")
    for memory in (api.MEM_HOST, api.MEM_DEVICE):
        for wm in (None, warm):
            plain = run(w, None, wm, memory)
            negative = run(w, spec(w, advance=np.full(B, -0.25)), wm, memory)
            assert plain["rc"] == api.OK and negative["rc"] == api.OK
            same(negative, plain, keys, ("every advance negative", memory))
            assert (negative["source"] == carry.NOT_ASKED).all() and negative["n_kept"] == 0
            if wm is None:
                same(plain, cold, keys, ("carry = NULL", memory))
    # the Python form: carry=None is the call it was
    py = w["opt"].plan_scenes(w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"])
    same(py, cold, keys, "plan_scenes(carry=None)")
    assert "source" not in py
    py = w["opt"].plan_scenes(w["packed"], w["start"], w["dp_cfg"], w["cor_cfg"], carry=spec(w))
    assert np.array_equal(py["source"], pc.WANT) and py["n_kept"] == 2


def test_none_one_and_all_scenes_listed(world):
    w, cold = world, world["cold"]
    # all: the planner runs on the batch as it lies (an advance above the limit everywhere)
    everyone = run(w, spec(w, advance=np.full(B, 5.0)), None, api.MEM_DEVICE)
    assert (everyone["source"] == carry.REFUSED).all() and everyone["n_kept"] == 0
    same(everyone, cold, SOLVED + ("plan", "dp", "outcome"), "all listed")
    # none: every scene a copy of a kept one -- nothing is launched for the planner
    packed = dict(w["packed"], **{k: np.ascontiguousarray(np.repeat(w["packed"][k][pc.KEPT_A:pc.KEPT_A + 1], B, axis=0))
                                  for k in api._SCENE_BATCH_ARRAYS})
    alike = dict(w, packed=packed, start=np.repeat(w["start"][pc.KEPT_A:pc.KEPT_A + 1], B, axis=0))
    cy = spec(w, rows=np.repeat(w["rows"][pc.KEPT_A:pc.KEPT_A + 1], B, axis=0), advance=np.full(B, pc.T0))
    nobody = run(alike, cy, None, api.MEM_DEVICE)
    assert nobody["rc"] == api.OK and (nobody["source"] == carry.KEPT).all() and nobody["n_kept"] == B
    kept = run(w, spec(w), None, api.MEM_HOST)
    for b in range(B):
        same({k: nobody[k][b] for k in SOLVED + ("plan", "dp")}, {k: kept[k][pc.KEPT_A] for k in SOLVED + ("plan", "dp")},
             SOLVED + ("plan", "dp"), ("none listed", b))
    # one: the last of these scenes off its start
    alike["start"] = alike["start"].copy()
    alike["start"][B - 1, :2] += [40.0, 40.0]
    one = run(alike, cy, None, api.MEM_HOST)
    assert list(one["source"]) == [0] * (B - 1) + [carry.OFF_START] and one["n_kept"] == B - 1
    want = chain(alike, cy, None)
    assert list(want["sel"]) == [B - 1] and sw.same_bits(one["dp"], want["dp"])
    same(one, nobody, SOLVED + ("plan", "dp"), "the scenes beside the listed one", np.arange(B - 1))


def test_a_chunk_border_inside_the_list(world):
    w = world
    whole = run(w, spec(w), None, api.MEM_DEVICE)
    w["opt"].set_option(api.OPT_SCENE_CHUNK, 2)                        # five listed scenes: chunks of 2, 2 and 1
    try:
        for memory in (api.MEM_HOST, api.MEM_DEVICE):
            parts = run(w, spec(w), None, memory)
            assert parts["rc"] == api.OK and parts["n_kept"] == 2
            same(parts, whole, ALL, ("chunks of two", memory))
    finally:
        w["opt"].set_option(api.OPT_SCENE_CHUNK, 0)


def test_the_previous_plan_rows_as_the_rows_to_carry(world):
    """a second cycle as an episode makes it: the rows are the cold pipeline's `plan` rows (ROWS_PLAN), whatever populations
    that gives -- equality with the chain only"""
    w, cold = world, world["cold"]
    cy = spec(w, rows=cold["plan"], layout=api.ROWS_PLAN, advance=np.where(cold["outcome"] == 0, 0.3, -1.0), offset=50.0)
    want = chain(w, cy, None)
    for memory in (api.MEM_HOST, api.MEM_DEVICE):
        got = run(w, cy, None, memory)
        assert got["rc"] == api.OK and np.array_equal(got["source"], want["source"]) and sw.same_bits(got["dp"], want["dp"])
        assert got["n_kept"] == (want["source"] == 0).sum()
        same(got, want, SOLVED, ("plan rows", memory), want["found"] & (got["outcome"] == 0))


def test_every_refusal_leaves_the_outputs_unwritten(world):
    w = world
    rows, adv = np.ascontiguousarray(w["rows"]), np.ascontiguousarray(w["advance"])

    def refused(memory=api.MEM_HOST, layout=api.ROWS_COARSE, n_rows=K, r=True, a=True, max_advance=pc.MAX_ADVANCE,
                offset=pc.MAX_START_OFFSET, buffer=pc.BUFFER):
        cs = api.Carry(memory, layout, n_rows, 0, rows.ctypes.data if r else None, adv.ctypes.data if a else None, max_advance,
                       offset, buffer)
        got = run(w, None, None, api.MEM_HOST, fill=-5.5, carry_struct=cs)
        for k, v in outputs(-5.5).items():
            assert (got[k] == v).all(), k
        return got["rc"]

    assert refused(r=False) == api.ERR_NULL and refused(a=False) == api.ERR_NULL
    assert refused(layout=17) == api.ERR_ARG and refused(layout=api.ROWS_CONTROLS) == api.ERR_ARG
    assert refused(memory=api.MEM_DEVICE) == api.ERR_ARG and refused(memory=5) == api.ERR_ARG        # not where the scenes are
    assert refused(n_rows=1) == api.ERR_ARG and refused(n_rows=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    for bad in (-0.1, float("nan"), float("inf")):
        assert refused(max_advance=bad) == api.ERR_ARG and refused(offset=bad) == api.ERR_ARG and refused(buffer=bad) == api.ERR_ARG
    again = run(w, spec(w), None, api.MEM_HOST)                        # the handle is as usable as before
    assert again["rc"] == api.OK and np.array_equal(again["source"], pc.WANT)
