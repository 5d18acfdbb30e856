"""The three scene kernels -- cilqr_dp_plan_batch, cilqr_scene_points_batch, cilqr_plan_scenes_batch -- at the limits
include/cilqr.h declares (8 vertices, 32 static and 32 dynamic slots, 1024 trajectory samples, 256 knots / path samples)
and across the chunks in which they process a large batch.  The scenes come from tests/limit_scenes.py (polygons of 3 - 8
vertices, concave and clockwise ones, trajectories whose times are no knot times, ties with the planner's sample times);
tests/test_scene_limits.py pins the yardsticks on them without a GPU.

Nothing is judged by a rule of its own: the planner by rules 3 and 4 of tests/test_gpu_dp_batch.py (_compare, CAP, TOL),
the points by rules 1 - 3 of tests/test_gpu_scene_points.py (_against_host, _numpy_points, _loop_points, TOL), the
pipeline by that module's _chain / _check_outcome / _check_plan_rows.  The records of a run are printed in lines that
start with DP_BATCH_RECORD / SCENE_POINTS_RECORD (pytest -s)."""
import json
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import limit_scenes as ls
import test_gpu_dp_batch as dpb
import test_gpu_scene_points as spt
from cilqr_amd import api, scene_io
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HOST_WORKERS = dpb.HOST_WORKERS
# scenes per row: CAP (0.5 %) of a row is at least one scene.  The host planner takes about 1 s per scene of the 8 s row
# and 4 - 5 s per scene at 256 knots (one thread), so the long row stays at the floor of 200.
DP_ROWS = {
    "full_8s": dict(ls.ROWS["full_8s"], scenes=256, seed=401),
    "full_25s": dict(ls.ROWS["full_25s"], scenes=200, seed=402),                                # K = nq = 256
    "full_12.7s": dict(ls.ROWS["full_8s"], tf=12.7, over=dict(max_velocity=10.0), scenes=256, seed=403),   # nq = K + 1
}
PLACED_BYTES_CAP = 1 << 30     # planner_batch.hip: kPlacedBytesCap
POINTS_BYTES_CAP = 1 << 30     # scene_pipeline.hip: kPointsBytesCap


def dp_chunk(nq, max_dynamic, max_vertices):
    """Scenes per chunk of cilqr_dp_plan_batch (planner_batch.hip: rec, per_scene, chunk)."""
    rec = 4 + 2 * max_vertices
    return max(1, PLACED_BYTES_CAP // (nq * max_dynamic * (rec * 8 + 4)))


def points_chunk(n_knots, max_points):
    """Scenes per chunk of the points loop of cilqr_plan_scenes_batch (scene_pipeline.hip: per_scene, chunk)."""
    return max(1, POINTS_BYTES_CAP // (n_knots * (max_points * 2 * 8 + 4)))


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


# ---------------------------------------------------------------------------------------------------------------------
# cilqr_dp_plan_batch at the corners
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    """Per row: the corner scenes, the host planner's results (HOST_WORKERS threads) and the device planner's from HOST
    arrays, with both wall times."""
    out = {}

    def get(name):
        if name in out:
            return out[name]
        r = DP_ROWS[name]
        n, tf = r["scenes"], r["tf"]
        sc, sf, over = ls.corner_scenes(n, r["seed"], r["S"], r["D"], r["V"], r["T"], tf, r["over"])
        cfg = api.default_dp_config(tf=tf, **over)
        K, nq = ls.dp_counts(tf)
        t0 = time.perf_counter()
        h_found, h_dp = dpb._host_plan(sf, sc["start"], cfg)
        host_s = time.perf_counter() - t0
        packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
        assert tuple(packed[k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples")) == (r["S"], r["D"], r["V"], r["T"])
        opt = api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=1, cmax=16)
        opt.dp_plan_batch(packed, sc["start"], cfg)      # grows the handle's work space
        t0 = time.perf_counter()
        dev = opt.dp_plan_batch(packed, sc["start"], cfg)
        dev_s = time.perf_counter() - t0
        out[name] = dict(sc=sc, sf=sf, over=over, cfg=cfg, K=K, nq=nq, tf=tf, packed=packed, opt=opt, host_found=h_found,
                         host_dp=h_dp, dev=dev, n=n)
        print("DP_BATCH_RECORD", json.dumps(dict(row=name, scenes=n, knots=K, path_samples=nq, host_threads=HOST_WORKERS,
                                                 host_planner_s=host_s, device_call_from_host_arrays_s=dev_s,
                                                 chunk=dp_chunk(nq, r["D"], r["V"]))), flush=True)
        return out[name]

    yield get
    for v in out.values():
        v["opt"].close()


def test_the_path_sample_counts_are_the_library_s():
    """tf = 25.5 is the longest horizon the planner takes (256 knots, 256 path samples); the next one is refused."""
    assert ls.dp_counts(25.5) == (api.DP_MAX_KNOTS, api.DP_MAX_KNOTS) and ls.dp_counts(12.7) == (127, 128)
    sc, sf = dpb._scenes("mix11", 4, 41)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=1, cmax=16) as opt:
        r = opt.dp_plan_batch(packed, sc["start"], api.default_dp_config(tf=25.5, max_velocity=10.0))
        assert r["dp"].shape == (4, 256, 9) and r["found"].any()
        with pytest.raises(api.CilqrError) as e:
            opt.dp_plan_batch(packed, sc["start"], api.default_dp_config(tf=25.6, max_velocity=10.0))
        assert e.value.code == api.ERR_CAPACITY
        # the last knot repeats its predecessor's velocity exactly where it is the last path sample (nq = K)
        for tf in (8.0, 12.7, 13.2, 25.5):
            K, nq = ls.dp_counts(tf)
            r = opt.dp_plan_batch(packed, sc["start"], api.default_dp_config(tf=tf, max_velocity=10.0))
            assert r["dp"].shape[1] == K and r["found"].any()
            repeats = [bool(r["dp"][b][-1, 6] == r["dp"][b][-2, 6]) for b in np.flatnonzero(r["found"])]
            assert all(repeats) if nq == K else not all(repeats), (tf, repeats)
            assert all(np.array_equal(r["dp"][b][:, 0], 0.1 * np.arange(K)) for b in range(4))


@pytest.mark.parametrize("row", list(DP_ROWS))
def test_dp_corners_same_plan_and_same_numbers_as_the_host_planner(planned, row):
    p = planned(row)
    r, n = p["dev"], p["n"]
    assert n * dpb.CAP >= 1
    assert r["dp"].shape == (n, p["K"], 9) and r["n_not_found"] == int((~r["found"]).sum())
    rec = dpb._compare(r["found"], r["dp"], p["host_found"], p["host_dp"], p["sf"].scenes, p["sc"]["start"], 0.1, row)
    assert rec["found"] >= n // 2 and rec["found"] < n, rec        # ... and a blocked road is among them
    # the other views, a second call and DEVICE arrays: no other bit
    assert dpb._same_bits(r["coarse"], np.ascontiguousarray(r["dp"][:, :, [2, 3, 4, 6, 7, 8]]))
    assert dpb._same_bits(r["knots"], np.ascontiguousarray(r["dp"][:, :, [2, 3, 4]]))
    assert dpb._same_bits(r["station"], np.ascontiguousarray(r["dp"][:, :, 1]))
    rc, d, _ = dpb._device_call(p["opt"], p["packed"], p["sc"]["start"], p["cfg"], p["K"])
    assert rc == api.OK and d["n_not_found"] == r["n_not_found"]
    for k in ("dp", "coarse", "knots", "station"):
        assert dpb._same_bits(d[k], r[k]), k
    assert np.array_equal(d["found"] != 0, r["found"])


@pytest.mark.parametrize("row", list(DP_ROWS))
def test_dp_corners_a_sample_against_the_line_by_line_oracle(planned, row):
    p = planned(row)
    pick = np.sort(np.random.default_rng(11).choice(p["n"], 32, replace=False))

    def one(b):
        return orc.dp_plan(scene_io.flatten_scene(p["sf"].center, p["sf"].scenes[b]), p["sc"]["start"][b, :3], tf=p["tf"], **p["over"])

    with ThreadPoolExecutor(HOST_WORKERS) as pool:
        outs = list(pool.map(one, pick))
    dpb._compare(p["dev"]["found"][pick], p["dev"]["dp"][pick], np.array([o[0] for o in outs], dtype=bool),
                 np.stack([o[1] for o in outs]), [p["sf"].scenes[b] for b in pick], p["sc"]["start"][pick], 0.1, row + " / oracle")


# ---------------------------------------------------------------------------------------------------------------------
# cilqr_scene_points_batch at the corners
# ---------------------------------------------------------------------------------------------------------------------
# S, D, knots, scenes: the full corner; a tile tail (K % 8 = 5); D = 31 and D = 1 for the (knot, obstacle) pairing of the
# lanes; no dynamic slot at all, no static slot at all
POINT_CASES = {
    "full": (32, 32, 256, 12),
    "tile_tail": (32, 32, 253, 6),
    "d31": (32, 31, 51, 6),
    "d1": (32, 1, 51, 6),
    "s32_d0": (32, 0, 51, 6),
    "s0_d32": (0, 32, 51, 6),
}


def _host_call_with_sentinel(opt, packed, times, multiple, max_points):
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_HOST, **{k: keep[k].ctypes.data for k in keep})
    B, K = packed["batch"], len(times)
    pts, cnt = np.full((B, K, max_points, 2), -7.0), np.full((B, K), -7, dtype=np.int32)
    ok = np.full(B, -7, dtype=np.int32)
    rc = opt.scene_points_raw(sb, K, times, multiple, max_points, pts.ctypes.data, cnt.ctypes.data, ok.ctypes.data)
    return rc, pts, cnt, ok


@pytest.mark.parametrize("multiple", [False, True], ids=["corners", "six_per_edge"])
@pytest.mark.parametrize("case", list(POINT_CASES))
def test_points_at_the_corners(case, multiple):
    S, D, K, B = POINT_CASES[case]
    V, T = api.DP_MAX_VERTICES, api.DP_MAX_SAMPLES
    sc, sf, _ = ls.corner_scenes(B, 420 + list(POINT_CASES).index(case), S, D, V, T, 25.5 if K > 200 else 5.0)
    times = 0.1 * np.arange(K)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes, max_static=S, max_dynamic=D, max_vertices=V,
                                       max_samples=T if D else 1)
    P = (S + D) * V * (6 if multiple else 1)
    if case == "full":
        assert P == 64 * 8 * (6 if multiple else 1) and K == api.DP_MAX_KNOTS
    t0 = time.perf_counter()
    host = spt._host_points(sf.scenes, times, multiple=multiple)
    host_s = time.perf_counter() - t0
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=1, cmax=16) as opt:
        rc_h, pts, cnt, ok = _host_call_with_sentinel(opt, packed, times, multiple, P)
        rc_d, d_pts, d_cnt, d_ok, dev_s = spt._device_points(opt, packed, times, multiple=multiple, warm=True)
        trig = spt._trig_table(opt, sf.scenes)
        cos_t, sin_t = spt._device_trig(opt, packed) if D and not multiple else (None, None)
    assert rc_h == api.OK and rc_d == api.OK and (ok == 1).all() and (d_ok == 1).all()
    live = np.arange(P)[None, None, :] < cnt[:, :, None]
    # the sentinel behind point_count is untouched, from HOST and from DEVICE arrays; both give the same bits
    assert (pts[~live] == -7.0).all() and (d_pts[~live] == -7.0).all()
    assert np.array_equal(d_cnt, cnt) and spt._same_bits(d_pts[live], pts[live])
    # rules 1 and 3: environment_points (counts exactly, coordinates to 1e-12)
    shown = np.where(live[..., None], pts, 0.0)
    worst = spt._against_host(shown, cnt, host, case)
    # rule 2: the documented expressions with the device library's cos / sin, every bit
    if multiple or not D:
        for b, scene in enumerate(sf.scenes):
            want, _ = spt._loop_points(scene, times, trig, multiple=multiple)
            for k in range(K):
                assert cnt[b, k] == len(want[k]) and spt._same_bits(pts[b, k, :cnt[b, k]], want[k]), (b, k)
    else:
        want, want_cnt = spt._numpy_points(packed, times, cos_t, sin_t)
        assert np.array_equal(cnt, want_cnt) and spt._same_bits(shown, want)
    n_static = np.array([sum(len(q) for q in s.static) for s in sf.scenes]) * (6 if multiple else 1)
    assert (cnt >= n_static[:, None]).all()
    assert not D or ((cnt > n_static[:, None]).any() and (np.diff(cnt, axis=1) != 0).any())    # obstacles come and go
    if case == "full":
        assert cnt.max() > P // 2
    print("SCENE_POINTS_RECORD", json.dumps(dict(case=case, multiple_sample=multiple, scenes=B, knots=K, max_static=S,
                                                 max_dynamic=D, max_points=P, live_points=int(cnt.sum()),
                                                 most_points_in_a_row=int(cnt.max()),
                                                 max_scaled_error_against_host_libm=worst, tolerance=spt.TOL,
                                                 environment_points_s=host_s, device_call_from_device_arrays_s=dev_s)), flush=True)
    assert worst <= spt.TOL, (case, worst)


# ---------------------------------------------------------------------------------------------------------------------
# the chunks of cilqr_dp_plan_batch
# ---------------------------------------------------------------------------------------------------------------------
def test_dp_chunks_change_no_bit():
    """850 scenes at 256 path samples, packed with 32 dynamic slots of 8 vertices: 1.34 MB of placed polygons per scene,
    so the call plans them in chunks of 799 -- the second chunk starts at scene 799 -- against the same scenes in their
    natural packing, which is one chunk."""
    B, tf = 850, 25.5
    sc, sf = dpb._scenes("dyn20", B, 431)
    cfg = api.default_dp_config(tf=tf, max_velocity=10.0)
    K, nq = ls.dp_counts(tf)
    natural = scene_io.pack_scene_batch(sf.center, sf.scenes)
    wide = scene_io.pack_scene_batch(sf.center, sf.scenes, max_dynamic=32, max_vertices=8)
    chunk_wide = dp_chunk(nq, 32, 8)
    chunk_natural = dp_chunk(nq, natural["max_dynamic"], natural["max_vertices"])
    assert chunk_wide == 799 and chunk_wide < B <= chunk_natural
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=1, cmax=16) as opt:
        one = opt.dp_plan_batch(natural, sc["start"], cfg)
        t0 = time.perf_counter()
        two = opt.dp_plan_batch(wide, sc["start"], cfg)
        wide_s = time.perf_counter() - t0
        rc1, d_one, _ = dpb._device_call(opt, natural, sc["start"], cfg, K)
        rc2, d_two, _ = dpb._device_call(opt, wide, sc["start"], cfg, K)
    print("DP_BATCH_RECORD", json.dumps(dict(what="chunks", scenes=B, knots=K, path_samples=nq, chunk=chunk_wide,
                                             chunk_of_the_natural_packing=chunk_natural, found=int(one["found"].sum()),
                                             not_found=one["n_not_found"], device_call_from_host_arrays_s=wide_s)), flush=True)
    assert rc1 == api.OK and rc2 == api.OK
    assert one["found"][chunk_wide:].any() and one["n_not_found"] == int((~one["found"]).sum())
    assert len({one["dp"][b].tobytes() for b in range(B)}) == B           # the scenes differ: a shifted row would show
    for k in ("dp", "coarse", "knots", "station", "found"):
        assert dpb._same_bits(two[k], one[k]), k                                   # HOST arrays
    assert two["n_not_found"] == one["n_not_found"]
    for k in ("dp", "coarse", "knots", "station", "found"):
        assert dpb._same_bits(d_two[k], d_one[k]), k                               # DEVICE arrays
    assert d_two["n_not_found"] == d_one["n_not_found"] == one["n_not_found"]
    assert dpb._same_bits(d_one["dp"], one["dp"]) and np.array_equal(d_one["found"] != 0, one["found"])


# ---------------------------------------------------------------------------------------------------------------------
# cilqr_plan_scenes_batch at its point budget and across both caps
# ---------------------------------------------------------------------------------------------------------------------
COR_MAX_POINTS = 320     # kernels_corridor.hip: kCorMaxPts, the points of a knot plus the 8 (24) of the road box


@pytest.mark.parametrize("multiple", [False, True], ids=["corners", "six_per_edge"])
def test_pipeline_at_its_point_budget(multiple):
    B = 128
    r = ls.ROWS["small_5s"] if multiple else ls.ROWS["budget_5s"]
    S, D, V, T = r["S"], r["D"], r["V"], r["T"]
    if multiple:
        assert (S + D) * V == 49 and (S + D) * V * 6 + 24 <= COR_MAX_POINTS < (S + D + 1) * V * 6 + 24
    else:
        assert (S + D) * V + 8 == COR_MAX_POINTS
    sc, sf, over = ls.corner_scenes(B, 441 + multiple, S, D, V, T, r["tf"], r["over"])
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    assert (packed["max_static"], packed["max_dynamic"], packed["max_vertices"]) == (S, D, V)
    start = np.ascontiguousarray(sc["start"])
    dp_cfg, cor_cfg = api.default_dp_config(tf=r["tf"], **over), api.default_corridor_config()
    cor_cfg.is_multiple_sample = int(multiple)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=B, cmax=16, max_lane_segments=256) as opt:
        chain = spt._chain(opt, sf.center, packed, start, dp_cfg, cor_cfg)
        host = opt.plan_scenes(packed, start, dp_cfg, cor_cfg)
        dev = spt._plan_on_device(opt, packed, start, dp_cfg, cor_cfg)
        # one slot more is one point too many
        over_budget = scene_io.pack_scene_batch(sf.center, sf.scenes, max_static=S + 1)
        with pytest.raises(api.CilqrError) as e:
            opt.plan_scenes(over_budget, start, dp_cfg, cor_cfg)
        assert e.value.code == api.ERR_CAPACITY
    found = chain["found"]
    assert spt._same_bits(host["dp"], chain["dp"])
    for k in spt.SOLVED:
        assert spt._same_bits(host[k][found], chain[k][found]), k              # HOST arrays
        assert spt._same_bits(dev[k], host[k]), k                              # DEVICE arrays
    for k in ("plan", "dp", "outcome"):
        assert spt._same_bits(dev[k], host[k]), k
    assert (host["n_dp_failed"], host["n_corridor_failed"]) == (dev["n_dp_failed"], dev["n_corridor_failed"])
    spt._check_outcome(host, chain)
    spt._check_plan_rows(host)
    print("SCENE_POINTS_RECORD", json.dumps(dict(pipeline="point budget", multiple_sample=multiple, scenes=B, max_static=S,
                                                 max_dynamic=D, max_vertices=V, outcome=np.bincount(host["outcome"], minlength=3).tolist(),
                                                 status=np.bincount(host["status"], minlength=7).tolist())), flush=True)
    assert host["n_dp_failed"] >= 1                                            # the blocked roads
    assert (host["status"] != api.ST_NO_CORRIDOR).sum() >= B // 4


def test_pipeline_across_the_dp_cap_and_the_points_cap():
    """4300 scenes packed to 7 static and 32 dynamic slots of 8 vertices: the planner takes them in chunks of 4011, the
    points loop in chunks of 4214 -- one call crosses both -- against the same scenes in their natural packing."""
    B, tf = 4300, 5.0
    sc, sf = spt._scenes("mix11", B, 451, workers=HOST_WORKERS)
    start = np.ascontiguousarray(sc["start"])
    K, nq = ls.dp_counts(tf)
    natural = scene_io.pack_scene_batch(sf.center, sf.scenes)
    wide = scene_io.pack_scene_batch(sf.center, sf.scenes, max_static=7, max_dynamic=32, max_vertices=8)
    chunks = dict(dp=dp_chunk(nq, 32, 8), points=points_chunk(K, (7 + 32) * 8),
                  dp_natural=dp_chunk(nq, natural["max_dynamic"], natural["max_vertices"]),
                  points_natural=points_chunk(K, (natural["max_static"] + natural["max_dynamic"]) * natural["max_vertices"]))
    assert (chunks["dp"], chunks["points"]) == (4011, 4214)
    assert chunks["dp"] < B and chunks["points"] < B and chunks["dp_natural"] >= B and chunks["points_natural"] >= B
    dp_cfg, cor_cfg = api.default_dp_config(tf=tf), api.default_corridor_config()
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=B, cmax=16, max_lane_segments=256) as opt:
        assert opt.get_option(api.OPT_SCENE_CHUNK)[0] == 0
        one = opt.plan_scenes(natural, start, dp_cfg, cor_cfg)
        t0 = time.perf_counter()
        two = opt.plan_scenes(wide, start, dp_cfg, cor_cfg)
        wide_s = time.perf_counter() - t0
        dev = spt._plan_on_device(opt, wide, start, dp_cfg, cor_cfg)
    print("SCENE_POINTS_RECORD", json.dumps(dict(pipeline="both caps", scenes=B, chunks=chunks,
                                                 outcome=np.bincount(one["outcome"], minlength=3).tolist(),
                                                 status=np.bincount(one["status"], minlength=7).tolist(),
                                                 plan_scenes_from_host_arrays_s=wide_s)), flush=True)
    tail = slice(max(chunks["dp"], chunks["points"]), B)
    assert (one["status"][tail] != api.ST_NO_CORRIDOR).any()      # solved scenes behind both chunk borders
    for k in spt.SOLVED + ("plan", "dp", "outcome"):
        assert spt._same_bits(two[k], one[k]), k                               # HOST arrays
        assert spt._same_bits(dev[k], one[k]), k                               # DEVICE arrays
    assert (two["n_dp_failed"], two["n_corridor_failed"]) == (one["n_dp_failed"], one["n_corridor_failed"]) == \
        (dev["n_dp_failed"], dev["n_corridor_failed"])
    spt._check_plan_rows(two)
