"""cilqr_window_scenes_batch (kernels_scene_window.hip) on the GPU: the kernel against the host call cilqr_window_scene bit for
bit -- batch sizes, slot counts, source lengths and window capacities on both sides of the wave (64) and of the workgroup's
four slots, a t0 per scene, HOST and DEVICE arrays, device pointers on an odd double (the 8-byte path), rows behind a count
untouched behind a NaN sentinel, the crafted table of tests/scene_window_cases.py at places 0, 63 and 64 of a batch --, an
overflowing scene and one with a bad source count inside a batch, the scene kernels downstream on the device's window
against the shifted full scene, and a 15 s recording that the scene kernels refuse and its window which they take."""
import numpy as np
import pytest

import scene_window_cases as sw
from cilqr_amd import api, scene_io

pytestmark = pytest.mark.gpu
NAN = float("nan")

# (B, D, source samples, out_samples): every value of B in {1, 3, 65}, D in {1, 5, 32}, source in {1, 63, 64, 65, 1501, 5000},
# out_samples in {1, 7, 64, 1024}
SHAPES = [(1, 1, 1, 1), (3, 5, 63, 7), (3, 5, 64, 64), (65, 1, 65, 64), (65, 5, 1501, 64), (3, 32, 5000, 1024), (1, 32, 64, 7),
          (65, 32, 63, 1)]


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
    assert sw.same_bits(rows, w_rows), what             # NaN sentinels included: rows behind a count are untouched
    assert np.array_equal(ok, w_ok) and n == int((w_ok == 0).sum()), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-D%d-S%d-out%d" % s)
def test_the_kernel_is_the_host_call(opt, shape):
    B, D, S, out = shape
    rng = np.random.default_rng(sum(shape))
    packed, t0 = sw.random_batch(rng, B, D, S)
    want = sw.host_batch(packed, t0, sw.SPAN, out, NAN)
    assert (want[1] > 0).any() and (out >= 64 or S < 8 or (want[1] < 0).any())      # windows, and overflows where they must be
    _same(sw.host_arrays_window(opt, packed, t0, sw.SPAN, out, NAN), want, "HOST")
    _same(sw.device_arrays_window(opt, packed, t0, sw.SPAN, out, NAN), want, "DEVICE, 16-byte accesses")
    _same(sw.device_arrays_window(opt, packed, t0, sw.SPAN, out, NAN, odd=True), want, "DEVICE, 8-byte accesses")
    if shape == SHAPES[0]:
        assert want[1][0, 0] == 1


def test_the_wave_search_returns_what_the_halving_returns(opt):
    """every border position of one long trajectory: t0 on, just before and just behind every 61st of 5000 samples, so that
    L and H fall into every piece of every round of the wave's search"""
    S = 5000
    times = sw.random_times(np.random.default_rng(5), S, 0.0, 0.004)
    at = np.arange(0, S, 61)
    t0 = np.concatenate([times[at], times[at] - 2e-9, times[at] + 2e-9, [-50.0, times[-1] + 50.0]])
    B = len(t0)
    packed = sw.empty_batch(B, 1, S)
    packed["dynamic_trajectories"][:, 0] = sw.traj_of(times)
    packed["dynamic_trajectory_counts"][:] = S
    span = 0.25
    want = sw.host_batch(packed, t0, span, 128, NAN)
    assert want[1].min() >= 1 and want[1].max() <= 128 and len(np.unique(want[0][:, 0, 0, 1])) > 60
    _same(sw.device_arrays_window(opt, packed, t0, span, 128, NAN), want, "borders")


@pytest.mark.parametrize("place", [0, 63, 64])
def test_the_crafted_table_inside_a_batch(opt, place):
    cases = sw.crafted()
    rng = np.random.default_rng(place)
    for span in (sw.SPAN, 0.0):
        group = [c for c in cases if c["span"] == span]
        S = max(len(c["traj"]) for c in group)
        filler, t0 = sw.random_batch(rng, 65, 1, 80)
        packed = sw.empty_batch(65, 1, S)
        packed["dynamic_trajectories"][:, :, :80] = filler["dynamic_trajectories"]
        packed["dynamic_trajectory_counts"][:] = filler["dynamic_trajectory_counts"]
        for c in group:
            T = len(c["traj"])
            packed["dynamic_trajectories"][place, 0, :T] = c["traj"]
            packed["dynamic_trajectory_counts"][place, 0] = T
            t0[place] = c["t0"]
            rows, counts, ok, rc, n = sw.device_arrays_window(opt, packed, t0, span, sw.OUT, NAN)
            want_rows, want_count = sw.expected(c["traj"], c["t0"], span, sw.OUT, NAN)
            assert rc == api.OK and counts[place, 0] == want_count and ok[place] == int(want_count >= 0), c["name"]
            assert sw.same_bits(rows[place, 0], want_rows), c["name"]


def test_an_overflow_and_a_bad_count_inside_a_batch(opt):
    rng = np.random.default_rng(65)
    filler, t0 = sw.random_batch(rng, 65, 5, 100)
    packed = sw.empty_batch(65, 5, 200)
    packed["dynamic_trajectories"][:, :, :100] = filler["dynamic_trajectories"]
    packed["dynamic_trajectory_counts"][:] = filler["dynamic_trajectory_counts"]
    out = int(sw.host_batch(packed, t0, sw.SPAN, 200, NAN)[1].max())       # every window fits: at most 100 samples
    plain = sw.device_arrays_window(opt, packed, t0, sw.SPAN, out, NAN)
    assert plain[3] == api.OK and plain[4] == 0 and (plain[2] == 1).all() and plain[1].max() == out
    hurt = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in packed.items()}
    hurt["dynamic_trajectories"][17, 3, :200] = sw.traj_of(t0[17] + np.arange(200) * 0.001)    # 200 samples inside the span
    hurt["dynamic_trajectory_counts"][17, 3] = 200
    hurt["dynamic_trajectory_counts"][40, 1] = 201                                              # above max_samples
    t0_bad = t0.copy()
    rows, counts, ok, rc, n = sw.device_arrays_window(opt, hurt, t0_bad, sw.SPAN, out, NAN)
    assert rc == api.OK and n == 2 and ok[17] == 0 and ok[40] == 0 and ok.sum() == 63
    assert counts[17, 3] == -1 and (counts[40] == -1).all()
    assert np.isnan(rows[17, 3]).all() and np.isnan(rows[40]).all()                            # nothing written there
    others = np.setdiff1d(np.arange(65), [17, 40])
    assert sw.same_bits(rows[others], plain[0][others]) and np.array_equal(counts[others], plain[1][others])
    keep = [d for d in range(5) if d != 3]
    assert sw.same_bits(rows[17, keep], plain[0][17, keep]) and np.array_equal(counts[17, keep], plain[1][17, keep])
    # a t0 that is no time, on the device: that scene alone; the same arrays in HOST memory are refused before the launch
    for bad in (NAN, float("inf")):
        t0_bad[5] = bad
        r2, c2, ok2, rc, n = sw.device_arrays_window(opt, hurt, t0_bad, sw.SPAN, out, NAN)
        assert rc == api.OK and n == 3 and ok2[5] == 0 and (c2[5] == -1).all() and np.isnan(r2[5]).all()
        assert sw.same_bits(r2[others[others != 5]], rows[others[others != 5]])
        assert sw.host_arrays_window(opt, packed, t0_bad, sw.SPAN, out, NAN)[3] == api.ERR_ARG
    assert sw.host_arrays_window(opt, hurt, t0, sw.SPAN, out, NAN)[3] == api.ERR_ARG


def test_argument_checks_launch_nothing(opt):
    rng = np.random.default_rng(9)
    packed, t0 = sw.random_batch(rng, 3, 2, 40)
    good = sw.host_arrays_window(opt, packed, t0, sw.SPAN, 64, NAN)
    assert good[3] == api.OK
    for kw in (dict(span=-1.0), dict(span=NAN), dict(span=float("inf")), dict(out=0)):
        r = sw.host_arrays_window(opt, packed, t0, kw.get("span", sw.SPAN), kw.get("out", 64), NAN)
        assert r[3] == api.ERR_ARG and np.isnan(r[0]).all() and (r[1] == -9).all() and (r[2] == -9).all(), kw
    r = sw.host_arrays_window(opt, packed, t0, sw.SPAN, api.DP_MAX_SAMPLES + 1, NAN)
    assert r[3] == api.ERR_CAPACITY and np.isnan(r[0]).all()
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_HOST, **{k: keep[k].ctypes.data for k in keep})
    rows, counts = np.zeros((3, 2, 64, 4)), np.zeros((3, 2), np.int32)
    assert opt.window_scenes_raw(sb, None, sw.SPAN, 64, rows.ctypes.data, counts.ctypes.data)[0] == api.ERR_NULL
    assert opt.window_scenes_raw(sb, t0.ctypes.data, sw.SPAN, 64, None, counts.ctypes.data)[0] == api.ERR_NULL
    assert opt.window_scenes_raw(sb, t0.ctypes.data, sw.SPAN, 64, rows.ctypes.data, None)[0] == api.ERR_NULL
    rc, n = opt.window_scenes_raw(sb, t0.ctypes.data, sw.SPAN, 64, rows.ctypes.data, counts.ctypes.data)      # ok is optional
    assert rc == api.OK and n == 0 and np.array_equal(counts, good[1])
    # the handle stays usable, and the Python form shares every other array with its input
    win = opt.window_scenes(packed, t0, sw.SPAN)
    assert win["max_samples"] == good[1].max() == win["dynamic_trajectory_counts"].max() and win["n_overflow"] == 0
    assert win["dynamic_polygon_points"] is packed["dynamic_polygon_points"] and win["window_ok"].all()
    assert sw.same_bits(np.where(np.isnan(good[0]), 0.0, good[0])[:, :, :win["max_samples"]], win["dynamic_trajectories"])


# ---------------------------------------------------------------------------------------------------------------------
# downstream
# ---------------------------------------------------------------------------------------------------------------------
def _road_scenes(rng, B, D, T, step):
    """(scenes with recordings of T samples that drive along the straight road ahead of x = 2, their t0)"""
    scenes, t0 = [], np.zeros(B)
    for b in range(B):
        trajs = [sw.random_trajectory(rng, T, rng.uniform(-1.0, 0.5), step, x0=rng.uniform(10.0, 30.0), lane=rng.uniform(-2.5, 2.5))
                 for _ in range(D)]
        scenes.append(sw.scene_with(trajs, static=[sw.BODY + np.array([45.0, 4.0])]))
        t0[b] = rng.uniform(0.0, T * step - 6.0)
    t0[0] = scenes[0].dynamic[0].trajectory[T // 3, 0]                 # a cycle that starts on a sample
    return scenes, t0


def _scene_calls(opt, packed, start3, cfg):
    """the four scene calls on a packed batch: every array they return"""
    r = opt.dp_plan_batch(packed, start3, cfg)
    times = r["dp"][0][:, 0]
    out = dict(dp=r["dp"], coarse=r["coarse"], knots=r["knots"], station=r["station"], found=r["found"])
    for multiple in (False, True):
        pts, cnt, ok = opt.scene_points(packed, times, multiple_sample=multiple)
        out.update({f"points{int(multiple)}": pts, f"point_count{int(multiple)}": cnt, f"points_ok{int(multiple)}": ok})
    hit = opt.check_collisions(packed, r["dp"], api.ROWS_COARSE, cfg, buffer=0.5)
    out.update(mask=hit["mask"], first_hit=hit["first_hit"], n_hit=hit["n_hit"])
    cl = opt.clearance(packed, r["dp"], api.ROWS_COARSE, cfg)
    out.update({"clearance_" + k: np.asarray(v) for k, v in cl.items()})
    return out


def _assert_same_results(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert sw.same_bits(a[k], b[k]), k


def test_the_scene_kernels_cannot_tell_the_window_from_the_shifted_scene(opt):
    rng = np.random.default_rng(400)
    cfg = api.default_dp_config(tf=5.0)
    scenes, t0 = _road_scenes(rng, 5, 3, 400, 0.05)
    packed = scene_io.pack_scene_batch(sw.CENTER, scenes)
    full = scene_io.pack_scene_batch(sw.CENTER, [scene_io.shift_scene(s, t) for s, t in zip(scenes, t0)])
    win = opt.window_scenes(packed, t0, float(cfg.tf), 128)
    assert win["window_ok"].all() and win["max_samples"] == 128 and full["max_samples"] == 400
    assert 90 < win["dynamic_trajectory_counts"].min() and win["dynamic_trajectory_counts"].max() < 128
    start3 = np.tile([2.0, 0.0, 0.0], (5, 1))
    on_window, on_full = _scene_calls(opt, win, start3, cfg), _scene_calls(opt, full, start3, cfg)
    _assert_same_results(on_window, on_full)
    assert on_full["found"].any() and (on_full["point_count0"] > 4).any()       # dynamic polygons were there to be read


def test_a_long_recording_is_refused_and_its_window_is_not(opt):
    rng = np.random.default_rng(1501)
    cfg = api.default_dp_config(tf=5.0)
    scenes, t0 = _road_scenes(rng, 5, 2, 1501, 0.01)
    packed = scene_io.pack_scene_batch(sw.CENTER, scenes)
    assert packed["max_samples"] == 1501 > api.DP_MAX_SAMPLES
    start3 = np.tile([2.0, 0.0, 0.0], (5, 1))
    times = np.arange(51) * 0.1
    rows = np.zeros((5, 51, 9))
    for call in (lambda: opt.dp_plan_batch(packed, start3, cfg), lambda: opt.scene_points(packed, times),
                 lambda: opt.check_collisions(packed, rows, api.ROWS_COARSE, cfg), lambda: opt.clearance(packed, rows, api.ROWS_COARSE, cfg)):
        with pytest.raises(api.CilqrError) as e:
            call()
        assert e.value.code == api.ERR_CAPACITY
    win = opt.window_scenes(packed, t0, float(cfg.tf))
    by_rule = scene_io.pack_scene_batch(sw.CENTER, [scene_io.window_scene(s, t, float(cfg.tf)) for s, t in zip(scenes, t0)])
    assert 500 < win["max_samples"] == by_rule["max_samples"] < 600
    assert sw.same_bits(win["dynamic_trajectories"], by_rule["dynamic_trajectories"])
    assert np.array_equal(win["dynamic_trajectory_counts"], by_rule["dynamic_trajectory_counts"])
    _assert_same_results(_scene_calls(opt, win, start3, cfg), _scene_calls(opt, by_rule, start3, cfg))
