"""cilqr_predict_scenes_batch (kernels_scene_predict.hip) on the GPU: the kernel against the host call cilqr_predict_scene bit
for bit -- batch sizes, slot counts on both sides of the workgroup's four slots, source lengths that need one, two and three
rounds of the wave's search, output lengths on both sides of the wave (64) and a second pass of the store loop, both modes,
HOST and DEVICE arrays, device pointers on an odd double (the 8-byte path), rows of a slot with count 0 or -1 untouched behind
a sentinel --, t0 walked over the borders of every piece of the search, a scene alone against the same scene in a batch, the
DEVICE-side refusals, the crafted table of tests/predict_cases.py as scenes of one call, and the DP planner and the audit
downstream on the device's prediction against the host call's."""
import numpy as np
import pytest

import predict_cases as pc
from cilqr_amd import api, scene_io

pytestmark = pytest.mark.gpu
FILL = pc.SENTINEL
SPAN = pc.SPAN

# (B, D, source samples, out_samples, sample_dt, mode): every value of B in {1, 3, 64}, D in {1, 4, 5, 9, 32}, source in
# {1, 2, 64, 65, 1501, 5000}, out_samples in {2, 52, 64, 65, 1024}; (out_samples - 1) * sample_dt >= 5 + 1e-9 in each
SHAPES = [(1, 1, 1, 2, 6.0, pc.CV), (3, 4, 2, 52, 0.1, pc.CV), (3, 5, 64, 64, 0.08, pc.HOLD), (64, 1, 65, 65, 0.08, pc.CV),
          (64, 5, 1501, 52, 0.1, pc.CV), (3, 32, 5000, 1024, 0.005, pc.CV), (1, 9, 64, 2, 5.5, pc.HOLD), (64, 9, 2, 64, 0.08, pc.CV)]
MAX_AGE = 2.0


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=8, cmax=16, max_lane_segments=256) as o:
        yield o


def _same(got, want, what):
    rows, counts, ok, rc, n = got
    w_rows, w_counts, w_ok = want
    assert rc == api.OK, what
    assert np.array_equal(counts, w_counts), what
    assert pc.same_bits(rows, w_rows), what             # sentinels included: rows of a slot with count 0 are untouched
    assert np.array_equal(ok, w_ok) and n == int((w_ok == 0).sum()), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-D%d-S%d-out%d" % s[:4])
def test_the_kernel_is_the_host_call(opt, shape):
    B, D, S, out, dt, mode = shape
    rng = np.random.default_rng(sum(shape[:4]))
    packed, t0 = pc.random_batch(rng, B, D, S)
    args = (mode, MAX_AGE, SPAN, dt, out, FILL)
    want = pc.host_batch(packed, t0, *args)
    assert want[1][0, 0] == out and set(np.unique(want[1])) <= {0, out} and (B * D < 8 or (want[1] == 0).any())
    _same(pc.host_arrays_predict(opt, packed, t0, *args), want, "HOST")
    _same(pc.device_arrays_predict(opt, packed, t0, *args), want, "DEVICE, 16-byte stores")
    _same(pc.device_arrays_predict(opt, packed, t0, *args, odd=True), want, "DEVICE, 8-byte stores")
    other = (pc.HOLD if mode == pc.CV else pc.CV,) + args[1:]
    _same(pc.device_arrays_predict(opt, packed, t0, *other), pc.host_batch(packed, t0, *other), "DEVICE, the other mode")


def test_the_wave_search_returns_what_the_halving_returns(opt):
    """J on the first and the last sample of every piece of the first round (5000 samples: 64 pieces of 79), on every sample of
    the first, a middle and the last piece -- the pieces of two of the second round and the places of the last --, and at T"""
    S, step = 5000, 79
    rng = np.random.default_rng(5)
    times = np.cumsum(rng.uniform(0.002, 0.006, S))                       # strictly increasing, steps far above 1e-9
    first = np.arange(0, S, step)
    inside = np.concatenate([np.arange(0, step), np.arange(31 * step, 32 * step), np.arange(63 * step, S)])
    J = np.unique(np.concatenate([first, np.minimum(first + step - 1, S - 1), first[1:] - 1, inside]))
    J = J[J >= 1]                                                         # J = 0 is the unseen obstacle: below
    t0 = np.concatenate([times[J] - 2e-9, [times[0] - 1.0, times[-1] + 0.001]])   # the first J with time - t0 > 1e-9 is J
    B = len(t0)
    packed = pc.empty_batch(B, 1, S)
    packed["dynamic_trajectories"][:, 0] = pc.traj_of(times)
    packed["dynamic_trajectory_counts"][:] = S
    args = (pc.CV, 0.5, SPAN, 0.1, 52, FILL)
    want = pc.host_batch(packed, t0, *args)
    latest = np.round((want[0][:-2, 0, 0, 3] - 0.1) / 0.001).astype(int)  # predict_cases.traj_of: the heading names the sample
    assert np.array_equal(latest, J - 1) and want[1][-2, 0] == 0 and want[1][-1, 0] == 52 and (want[1][:-2] == 52).all()
    _same(pc.device_arrays_predict(opt, packed, t0, *args), want, "borders")


def test_a_scene_does_not_depend_on_the_batch_around_it(opt):
    rng = np.random.default_rng(11)
    packed, t0 = pc.random_batch(rng, 64, 5, 200)
    args = (pc.CV, MAX_AGE, SPAN, 0.1, 52, FILL)
    whole = pc.device_arrays_predict(opt, packed, t0, *args)
    assert whole[3] == api.OK
    for b in (0, 17, 63):
        alone = pc.empty_batch(1, 5, 200)
        alone["dynamic_trajectories"][0] = packed["dynamic_trajectories"][b]
        alone["dynamic_trajectory_counts"][0] = packed["dynamic_trajectory_counts"][b]
        rows, counts, ok, rc, n = pc.device_arrays_predict(opt, alone, t0[b:b + 1], *args)
        assert rc == api.OK and np.array_equal(counts[0], whole[1][b]) and pc.same_bits(rows[0], whole[0][b]), b


def test_refusals_on_the_device(opt):
    rng = np.random.default_rng(65)
    packed, t0 = pc.random_batch(rng, 64, 5, 100)
    args = (pc.CV, MAX_AGE, SPAN, 0.1, 52, FILL)
    plain = pc.device_arrays_predict(opt, packed, t0, *args)
    _same(plain, pc.host_batch(packed, t0, *args), "plain")
    assert plain[4] == 0 and (plain[2] == 1).all()
    # a source count above max_samples, and a negative one: every slot of those scenes -1, nothing written, ok 0
    hurt = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in packed.items()}
    hurt["dynamic_trajectory_counts"][40, 1] = 101
    hurt["dynamic_trajectory_counts"][17, 4] = -1
    rows, counts, ok, rc, n = pc.device_arrays_predict(opt, hurt, t0, *args)
    others = np.setdiff1d(np.arange(64), [17, 40])
    assert rc == api.OK and n == 2 and ok[17] == 0 and ok[40] == 0 and ok.sum() == 62
    assert (counts[[17, 40]] == -1).all() and (rows[[17, 40]] == FILL).all()
    assert pc.same_bits(rows[others], plain[0][others]) and np.array_equal(counts[others], plain[1][others])
    # a t0 that is no time: that scene alone; the same arrays in HOST memory are refused before the launch
    t0_bad = t0.copy()
    for bad in (float("nan"), float("inf"), float("-inf")):
        t0_bad[5] = bad
        r2, c2, ok2, rc, n = pc.device_arrays_predict(opt, hurt, t0_bad, *args)
        keep = others[others != 5]
        assert rc == api.OK and n == 3 and ok2[5] == 0 and (c2[5] == -1).all() and (r2[5] == FILL).all() and ok2.sum() == 61
        assert pc.same_bits(r2[keep], plain[0][keep]) and np.array_equal(c2[keep], plain[1][keep])
        host = pc.host_arrays_predict(opt, packed, t0_bad, *args)
        assert host[3] == api.ERR_ARG and (host[0] == FILL).all() and (host[1] == -9).all()
    assert pc.host_arrays_predict(opt, hurt, t0, *args)[3] == api.ERR_ARG


def test_the_crafted_table_as_scenes_of_one_call(opt):
    cases = pc.crafted()
    seen = 0
    for (t0, mode, max_age), members in pc.groups(cases).items():
        S = max(1, max(len(cases[i]["traj"]) for i in members))
        packed = pc.empty_batch(1, len(members), S)
        for d, i in enumerate(members):
            T = len(cases[i]["traj"])
            packed["dynamic_trajectories"][0, d, :T] = cases[i]["traj"]
            packed["dynamic_trajectory_counts"][0, d] = T
        for odd in (False, True):
            rows, counts, ok, rc, n = pc.device_arrays_predict(opt, packed, np.array([t0]), mode, max_age, SPAN, pc.SAMPLE_DT,
                                                               pc.OUT, FILL, odd=odd)
            assert rc == api.OK and n == 0 and ok[0] == 1
            for d, i in enumerate(members):
                want_rows, want_count = pc.expected(cases[i], FILL)
                assert counts[0, d] == want_count, cases[i]["name"]
                assert pc.same_bits(rows[0, d], want_rows), cases[i]["name"]
        seen += len(members)
    assert seen == len(cases)


def test_argument_checks_launch_nothing(opt):
    rng = np.random.default_rng(9)
    packed, t0 = pc.random_batch(rng, 3, 2, 40)
    good = pc.host_arrays_predict(opt, packed, t0, pc.CV, MAX_AGE, SPAN, 0.1, 52, FILL)
    assert good[3] == api.OK
    for kw in (dict(span=-1.0), dict(span=float("nan")), dict(mode=2), dict(max_age=-1.0), dict(max_age=float("inf")), dict(dt=0.0),
               dict(dt=float("nan")), dict(out=1, dt=9.0), dict(out=51)):
        r = pc.host_arrays_predict(opt, packed, t0, kw.get("mode", pc.CV), kw.get("max_age", MAX_AGE), kw.get("span", SPAN),
                                   kw.get("dt", 0.1), kw.get("out", 52), FILL)
        assert r[3] == api.ERR_ARG and (r[0] == FILL).all() and (r[1] == -9).all() and (r[2] == -9).all(), kw
    r = pc.host_arrays_predict(opt, packed, t0, pc.CV, MAX_AGE, SPAN, 0.1, api.DP_MAX_SAMPLES + 1, FILL)
    assert r[3] == api.ERR_CAPACITY and (r[0] == FILL).all()
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_HOST, **{k: keep[k].ctypes.data for k in keep})
    rows, counts = np.zeros((3, 2, 52, 4)), np.zeros((3, 2), np.int32)
    call = lambda t, r, c: opt.predict_scenes_raw(sb, t, SPAN, pc.CV, MAX_AGE, 0.1, 52, r, c)
    assert call(None, rows.ctypes.data, counts.ctypes.data)[0] == api.ERR_NULL
    assert call(t0.ctypes.data, None, counts.ctypes.data)[0] == api.ERR_NULL
    assert call(t0.ctypes.data, rows.ctypes.data, None)[0] == api.ERR_NULL
    rc, n = call(t0.ctypes.data, rows.ctypes.data, counts.ctypes.data)                                         # ok is optional
    assert rc == api.OK and n == 0 and np.array_equal(counts, good[1])
    # the handle stays usable, and the Python form shares every other array with its input
    pred = opt.predict_scenes(packed, t0, SPAN, pc.CV, MAX_AGE, 0.1)
    assert pred["max_samples"] == 52 and pred["n_refused"] == 0 and pred["predict_ok"].all()
    assert pred["dynamic_polygon_points"] is packed["dynamic_polygon_points"]
    assert np.array_equal(pred["dynamic_trajectory_counts"], good[1])
    assert pc.same_bits(np.where(good[0] == FILL, 0.0, good[0]), pred["dynamic_trajectories"])


def test_the_scene_kernels_downstream(opt):
    """cilqr_dp_plan_batch and cilqr_check_collisions_batch on the device's prediction and on the host call's, B = 8"""
    rng = np.random.default_rng(400)
    cfg = api.default_dp_config(tf=5.0)
    B, D, T = 8, 3, 400
    scenes, t0 = [], np.zeros(B)
    for b in range(B):
        trajs = [pc.sw.random_trajectory(rng, T, rng.uniform(-1.0, 0.5), 0.05, x0=rng.uniform(10.0, 30.0), lane=rng.uniform(-2.5, 2.5))
                 for _ in range(D)]
        scenes.append(pc.scene_with(trajs, static=[pc.BODY + np.array([45.0, 4.0])]))
        t0[b] = rng.uniform(0.0, T * 0.05 - 6.0)
    packed = scene_io.pack_scene_batch(pc.CENTER, scenes)
    pred = opt.predict_scenes(packed, t0, float(cfg.tf), pc.CV, 0.5, float(cfg.delta_t))
    out = pred["max_samples"]
    assert pred["predict_ok"].all() and (pred["dynamic_trajectory_counts"] == out).all()
    by_host = scene_io.pack_scene_batch(pc.CENTER, [
        scene_io.Scene(s.start, s.coarse, s.static, [scene_io.DynamicObstacle(d.polygon, r) for d, r in zip(
            s.dynamic, pc.host_predict([d.trajectory for d in s.dynamic], float(t), pc.CV, 0.5, float(cfg.tf), float(cfg.delta_t), out)[0])])
        for s, t in zip(scenes, t0)])
    assert pc.same_bits(pred["dynamic_trajectories"], by_host["dynamic_trajectories"])
    start3 = np.tile([2.0, 0.0, 0.0], (B, 1))
    results = []
    for p in (pred, by_host):
        r = opt.dp_plan_batch(p, start3, cfg)
        hit = opt.check_collisions(p, r["dp"], api.ROWS_COARSE, cfg, buffer=0.5)
        results.append(dict(dp=r["dp"], coarse=r["coarse"], found=r["found"], mask=hit["mask"], first_hit=hit["first_hit"],
                            n_hit=hit["n_hit"]))
    for k in results[0]:
        assert pc.same_bits(np.asarray(results[0][k]), np.asarray(results[1][k])), k
    assert results[0]["found"].any()
