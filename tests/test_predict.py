"""The scene prediction (include/cilqr.h, "scene prediction"; include/cilqr/scene_predict.hpp) on the CPU: the declarations and
bindings of the two new calls, cilqr_predict_scene against the NumPy statement scene_io.predict_trajectory bit for bit on the
crafted table of tests/predict_cases.py with a branch census, the span condition at its edge and the other argument checks,
the tie to the window (a recording that moves as the rule assumes is predicted with the window's bits, and the host scene
calls return the same bits on both), the presence of every predicted obstacle at every query time of [0, span], and a C++
program of its own over the header under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import predict_cases as pc
from cilqr_amd import api, scene_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cilqr_predict_scene", "cilqr_predict_scenes_batch")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def crafted_host():
    """[(rows, count)] of the host call for every crafted case, each alone in its scene: computed once"""
    out = []
    for c in pc.crafted():
        rows, counts, n = pc.host_predict([c["traj"]], c["t0"], c["mode"], c["max_age"])
        assert n == 0
        out.append((rows[0], int(counts[0])))
    return out


def test_header_and_bindings_agree():
    hdr = open(api.HEADER_PATH).read()
    L = api.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (cilqr_[a-z_0-9]+)", out))
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in api.EXPORTS and hasattr(L, name) and name in exported, name
    assert L.cilqr_abi_version() == 7 == api.ABI_VERSION
    assert int(re.search(r"#define CILQR_ABI_VERSION (\d+)", hdr).group(1)) == 7
    for meth in ("predict_scenes", "predict_scenes_raw"):
        assert callable(getattr(api.BatchIlqrOptimizer, meth))
    assert callable(api.predict_scene) and callable(scene_io.predict_trajectory) and callable(scene_io.predict_scene)
    assert scene_io.PREDICT_MARGIN == 1e-9
    for name, value in (("CILQR_PREDICT_HOLD", api.PREDICT_HOLD), ("CILQR_PREDICT_CONSTANT_VELOCITY", api.PREDICT_CONSTANT_VELOCITY)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value
    assert (api.PREDICT_HOLD, api.PREDICT_CONSTANT_VELOCITY) == (0, 1)
    assert os.path.exists(os.path.join(ROOT, "include", "cilqr", "scene_predict.hpp"))


def test_host_call_is_the_numpy_statement(crafted_host):
    cases = pc.crafted()
    seen = set()
    for c, (rows, count) in zip(cases, crafted_host):
        want_rows, want_count = pc.expected(c)
        assert count == want_count, (c["name"], count, want_count)
        assert pc.same_bits(rows, want_rows), c["name"]        # the sentinel where nothing is written
        seen |= pc.census(c)
    assert seen == set(pc.BRANCHES), set(pc.BRANCHES) ^ seen
    by_name = dict(zip((c["name"] for c in cases), crafted_host))
    count = lambda name: by_name[name][1]
    row = lambda name, m: by_name[name][0][m]
    assert count("no sample") == 0 and count("one sample after t0") == 0 and count("one sample before t0") == pc.OUT
    # the borders themselves
    assert count("one sample at 1e-9: observed") == pc.OUT and count("one sample one double above 1e-9: unseen") == 0
    theta = lambda k: 0.1 + 0.001 * float(k)                   # predict_cases.traj_of: the heading names the sample
    assert row("the latest at 1e-9", 0)[3] == theta(2) and row("the latest one double above 1e-9 is not observed", 0)[3] == theta(1)
    assert count("age exactly max_age") == pc.OUT and count("age one double above max_age") == 0
    assert count("age exactly max_age = 0") == pc.OUT and count("age one double above max_age = 0") == 0
    assert count("the recording ended before t0") == 0
    still, moving = by_name["step exactly 1e-10"][0], by_name["step one double above 1e-10"][0]
    assert (still[:, 1] == still[0, 1]).all() and moving[1, 1] > moving[0, 1] + 1e8
    assert (by_name["two samples at one time"][0][:, 1] == 2.0).all()
    # the heading is the observed one, and a held obstacle stays where it was seen
    held, cv = by_name["moving, held"][0], by_name["moving"][0]
    assert (held[:, 1:] == [2.0, -0.3 * 2.0, theta(2)]).all() and (cv[:, 3] == theta(2)).all()
    assert cv[0, 1] == 2.0 + 3.0 * 0.25 and cv[10, 1] == (2.0 + 3.0 * 0.25) + 3.0 * (10 * 0.1) and cv[51, 0] == 51 * 0.1
    assert np.isnan(by_name["NaN x at the latest"][0][:, 1]).all() and np.isfinite(by_name["NaN x at the latest"][0][:, 2]).all()
    assert np.isnan(by_name["NaN heading"][0][:, 3]).all() and count("the latest at -inf") == 0
    assert (by_name["the sample before at -inf"][0][:, 1] == 1.25).all()


def test_a_scene_of_cases_the_scene_form_and_a_bad_count():
    """every case of the largest group in ONE scene, against the Scene form; then a negative source count among them"""
    cases = pc.crafted()
    (t0, mode, max_age), members = max(pc.groups(cases).items(), key=lambda kv: len(kv[1]))
    trajs = [cases[i]["traj"] for i in members]
    assert len(trajs) > 20 and any(len(t) == 0 for t in trajs)
    rows, counts, n = pc.host_predict(trajs, t0, mode, max_age)
    scene = scene_io.predict_scene(pc.scene_with(trajs), t0, mode, max_age, pc.SAMPLE_DT, pc.OUT)
    assert n == 0 and set(counts) == {0, pc.OUT}
    for d, dob in enumerate(scene.dynamic):
        assert counts[d] == len(dob.trajectory) and pc.same_bits(rows[d, :counts[d]], dob.trajectory)
        assert (rows[d, counts[d]:] == pc.SENTINEL).all()
    # a bad source count among good slots: that obstacle alone is refused, nothing is written to its rows, it takes no
    # samples of the packed array and the others are what they were
    some = [cases[i]["traj"] for i in members if len(cases[i]["traj"]) in (3, 4)][:4]
    good_rows, good_counts, _ = pc.host_predict(some, t0, mode, max_age)
    hurt = [some[0], np.zeros((0, 4)), some[1], some[2], np.zeros((0, 4)), some[3]]
    declared = [len(some[0]), -1, len(some[1]), len(some[2]), -7, len(some[3])]
    rows, counts, n = pc.host_predict(hurt, t0, mode, max_age, counts=declared)
    assert n == 2 and list(counts) == [good_counts[0], -1, good_counts[1], good_counts[2], -1, good_counts[3]]
    assert (rows[[1, 4]] == pc.SENTINEL).all() and pc.same_bits(rows[[0, 2, 3, 5]], good_rows)


def test_the_span_condition_and_the_argument_checks():
    L = api.lib()
    flat = scene_io.flatten_scene(pc.CENTER, pc.scene_with([pc.traj_of([-1.0, -0.5, 2.0])]))
    sc, keep = api.scene_struct(flat)
    out, counts, n = np.full((1, 64, 4), pc.SENTINEL), np.full(1, -9, np.int32), C.c_int32(-9)

    def call(scene=sc, t0=0.0, span=5.0, mode=api.PREDICT_CONSTANT_VELOCITY, max_age=1.0, dt=0.1, m=52, rows=out, cnt=counts):
        return L.cilqr_predict_scene(C.byref(scene) if scene is not None else None, C.c_double(t0), C.c_double(span), mode,
                                     C.c_double(max_age), C.c_double(dt), m, rows.ctypes.data if rows is not None else None,
                                     cnt.ctypes.data if cnt is not None else None, C.byref(n))
    # 50 * 0.1 = 5.0 does not reach 5 + 1e-9; 51 * 0.1 does
    assert not scene_io.predict_covers(51, 0.1, 5.0) and scene_io.predict_covers(52, 0.1, 5.0)
    assert scene_io.predict_out_samples(0.1, 5.0) == 52 and scene_io.predict_out_samples(0.125, 5.0) == 42
    assert scene_io.predict_out_samples(10.0, 5.0) == 2 and scene_io.predict_out_samples(0.005, 5.0) == 1002
    assert call(m=51) == api.ERR_ARG
    assert call(m=41, dt=0.125) == api.ERR_ARG          # 40 * 0.125 = 5.0 exactly: the margin is asked for
    assert call(scene=None) == api.ERR_NULL and call(rows=None) == api.ERR_NULL and call(cnt=None) == api.ERR_NULL
    for bad in (dict(t0=np.nan), dict(t0=np.inf), dict(span=np.nan), dict(span=np.inf), dict(span=-1e-300), dict(mode=2),
                dict(mode=-1), dict(max_age=-1e-300), dict(max_age=np.nan), dict(max_age=np.inf), dict(dt=0.0), dict(dt=-0.1),
                dict(dt=np.nan), dict(dt=np.inf), dict(m=1, dt=10.0), dict(m=0, dt=10.0), dict(m=-3, dt=10.0)):
        assert call(**bad) == api.ERR_ARG, bad
    no_src, _ = api.scene_struct(flat)
    no_src.dynamic_trajectories = None
    assert call(scene=no_src) == api.ERR_NULL
    assert (out == pc.SENTINEL).all() and counts[0] == -9 and n.value == -9      # every refusal wrote nothing
    assert call() == api.OK and counts[0] == 52 and n.value == 0 and (out[0, 52:] == pc.SENTINEL).all()
    assert call(m=42, dt=0.125) == api.OK and counts[0] == 42
    assert call(m=2, dt=10.0, mode=api.PREDICT_HOLD, max_age=0.5) == api.OK and counts[0] == 2
    assert call(span=0.0, m=2, dt=1e-8) == api.OK and call(span=0.0, m=2, dt=1e-9) == api.OK and call(span=0.0, m=2, dt=0.9e-9) == api.ERR_ARG
    assert L.cilqr_predict_scene(C.byref(sc), C.c_double(0.0), C.c_double(5.0), 1, C.c_double(1.0), C.c_double(0.1), 52,
                                 out.ctypes.data, counts.ctypes.data, None) == api.OK
    with pytest.raises(api.CilqrError):
        api.predict_scene(flat, 0.0, 5.0, api.PREDICT_HOLD, 1.0, 0.1, 51)
    with pytest.raises(ValueError):
        api.predict_scene(flat, 0.0, 5.0, api.PREDICT_HOLD, 1.0, 0.1, 52, np.zeros((1, 52, 4), dtype=np.float32))
    # a source of any length
    long = scene_io.flatten_scene(pc.CENTER, pc.scene_with([pc.traj_of(np.arange(100000) * 0.01)]))
    rows, cnt, refused = api.predict_scene(long, 512.345, 5.0, api.PREDICT_CONSTANT_VELOCITY, 0.02, 0.1, 52)
    assert cnt[0] == 52 and refused == 0 and rows[0, 0, 3] == 0.1 + 0.001 * 51234.0


def _same_bits_all(a, b):
    return all(pc.same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_a_recording_that_moves_as_assumed_is_predicted_with_the_windows_bits():
    cfg = api.default_dp_config(tf=5.0)
    span = float(cfg.tf)
    assert span == 5.0
    recs = [pc.dyadic_recording(200, 0.125, v=(1.5, -0.25), start=(12.0, 1.0)),
            pc.dyadic_recording(160, 0.125, v=(2.0, 0.125), start=(2.0, -2.5), theta=0.0625),
            pc.dyadic_recording(200, 0.125, v=(0.0, 0.0), start=(30.0, 0.5))]
    scene = pc.scene_with(recs, static=[pc.BODY + np.array([40.0, 4.0])])
    t0 = float(recs[0][40, 0])                                  # on a sample
    out = scene_io.predict_out_samples(0.125, span)
    assert t0 == 5.0 and out == 42
    win = scene_io.window_scene(scene, t0, span)
    pred = scene_io.predict_scene(scene, t0, api.PREDICT_CONSTANT_VELOCITY, 0.5, 0.125, out)
    for w, p in zip(win.dynamic, pred.dynamic):
        from_zero = w.trajectory[w.trajectory[:, 0] >= 0.0]
        assert len(w.trajectory) == out + 1 and w.trajectory[0, 0] == -0.125
        assert pc.same_bits(from_zero, p.trajectory)
    # the C call makes the same prediction
    rows, counts, _ = pc.host_predict(recs, t0, api.PREDICT_CONSTANT_VELOCITY, 0.5, span, 0.125, out)
    assert (counts == out).all() and _same_bits_all(rows, [p.trajectory for p in pred.dynamic])
    flat_w, flat_p = scene_io.flatten_scene(pc.CENTER, win), scene_io.flatten_scene(pc.CENTER, pred)
    found_w, coarse_w = api.dp_plan(flat_w, [2.0, 0.0, 0.0], cfg)
    found_p, coarse_p = api.dp_plan(flat_p, [2.0, 0.0, 0.0], cfg)
    assert found_w == found_p and pc.same_bits(coarse_w, coarse_p) and found_w
    rng = np.random.default_rng(7)
    q = np.sort(np.concatenate([[0.0, span], np.arange(41) * 0.125, np.arange(41) * 0.125 + 0.6e-10, rng.uniform(0.0, span, 30)]))
    q = q[q <= span]
    at = np.clip(np.searchsorted(recs[0][:, 0] - t0, q, side="right"), 0, len(recs[0]) - 1)
    rows10 = np.zeros((len(q), 10))
    rows10[:, 0] = q
    rows10[:, 1] = recs[0][at, 1] - 3.0 + rng.uniform(-1.5, 1.5, len(q))
    rows10[:, 2] = recs[0][at, 2] + rng.uniform(-1.5, 1.5, len(q))
    mw, fw, nw = api.check_collisions(flat_w, rows10, api.ROWS_TRAJ, cfg)
    mp, fp, npred = api.check_collisions(flat_p, rows10, api.ROWS_TRAJ, cfg)
    assert pc.same_bits(mw, mp) and (fw, nw) == (fp, npred) and 10 < nw < len(q)
    cw, kw, lw, aw = api.clearance_rows(flat_w, rows10, api.ROWS_TRAJ, cfg)
    cp, kp, lp, ap = api.clearance_rows(flat_p, rows10, api.ROWS_TRAJ, cfg)
    assert pc.same_bits(cw, cp) and pc.same_bits(kw, kp) and (lw, aw) == (lp, ap)


def test_every_predicted_obstacle_is_there_at_every_query_time():
    rng = np.random.default_rng(20250318)
    cfg = api.default_dp_config(tf=5.0)
    span = float(cfg.tf)
    dynamic_bits = api.HIT_REAR_DYNAMIC | api.HIT_FRONT_DYNAMIC
    predicted, absent = 0, 0
    for i in range(16):                                   # 16 scenes of four trajectories: 64 trajectories
        trajs = []
        for d in range(4):
            T = 1024 if (i, d) == (0, 0) else int(rng.integers(2, 1025))
            step = float(rng.choice([0.01, 0.02, 0.05]))
            trajs.append(pc.sw.random_trajectory(rng, T, rng.uniform(-3.0, 20.0), step, x0=rng.uniform(8.0, 30.0), lane=rng.uniform(-2.0, 2.0)))
        t0 = float(trajs[0][len(trajs[0]) // 2, 0]) if i % 4 == 0 else float(rng.uniform(-4.0, 45.0))
        mode = api.PREDICT_CONSTANT_VELOCITY if i % 2 else api.PREDICT_HOLD
        sample_dt = (0.1, 0.125, 0.07, 2.6)[i % 4]
        out = scene_io.predict_out_samples(sample_dt, span)
        rows, counts, refused = pc.host_predict(trajs, t0, mode, 0.5, span, sample_dt, out)
        assert refused == 0 and set(counts) <= {0, out}
        last = (out - 1) * sample_dt
        q = np.array([0.0, span, np.nextafter(span, 0.0), 0.5 * span, *np.arange(out) * sample_dt, *(np.arange(out) * sample_dt + 0.6e-10),
                      *rng.uniform(0.0, span, 8)])
        q = np.sort(q[q <= span])
        assert last >= span + 1e-9
        for d in range(4):
            if counts[d] == 0:
                absent += 1
                continue
            predicted += 1
            one = pc.scene_with([rows[d]])
            flat = scene_io.flatten_scene(pc.CENTER, one)
            found, coarse = api.dp_plan(flat, [2.0, 0.0, 0.0], cfg)        # the planner accepts the scene
            assert coarse.shape[1] == 9
            # the Query...Points form: the obstacle's polygon is among the points at every query time
            pts, cnt = scene_io.environment_points(one, q)
            assert (np.asarray(cnt) > 0).all(), (i, d)
            # the audit's plain form: a vehicle placed on the obstacle hits it at every query time
            at = np.clip(np.searchsorted(rows[d][:, 0], q, side="right"), 0, out - 1)
            rows10 = np.zeros((len(q), 10))
            rows10[:, 0], rows10[:, 1], rows10[:, 2] = q, rows[d][at, 1], rows[d][at, 2]
            mask, first, n_hit = api.check_collisions(flat, rows10, api.ROWS_TRAJ, cfg)
            assert ((mask & dynamic_bits) != 0).all() and first == 0 and n_hit == len(q), (i, d)
            cl, _, lowest, _ = api.clearance_rows(flat, rows10, api.ROWS_TRAJ, cfg)
            assert np.isfinite(lowest) and lowest <= 0.0
    print("PREDICT_RECORD", dict(predicted=predicted, absent=absent))
    assert predicted >= 16 and absent >= 8


def test_cpp_program_over_the_header(tmp_path, crafted_host):
    """tests/cpp/scene_predict_test.cc, built with AddressSanitizer and UndefinedBehaviorSanitizer, on the crafted table with the
    host call's results as expected values."""
    cases = pc.crafted()
    path = tmp_path / "scene_predict_cases.bin"
    pc.write_cases(str(path), cases, crafted_host)
    exe = tmp_path / "scene_predict_test"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scene_predict_test.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{len(cases)} cases" in out.stdout and "0 failures" in out.stdout
