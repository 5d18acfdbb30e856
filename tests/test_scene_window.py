"""The scene window (include/cilqr.h, "scene window"; include/cilqr/scene_window.hpp) on the CPU: the declarations and
bindings of the three new calls, cilqr_window_scene against the NumPy statement scene_io.window_trajectory bit for bit on the
crafted table of tests/scene_window_cases.py with a branch census, the equivalence the window exists for -- the host scene
calls return the same bits on the windowed scene as on the full shifted one --, the argument checks, and a C++ program of its
own over the header under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scene_window_cases as sw
from cilqr_amd import api, scene_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cilqr_window_scene", "cilqr_window_scenes_batch", "cilqr_plan_scenes_batch_warm")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def crafted_host():
    """[(rows, count)] of the host call for every crafted case, each alone in its scene: computed once"""
    out = []
    for c in sw.crafted():
        rows, counts, n = sw.host_window([c["traj"]], c["t0"], c["span"], c["out_samples"])
        assert n == int(counts[0] < 0)
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
    for meth in ("window_scenes", "window_scenes_raw"):
        assert callable(getattr(api.BatchIlqrOptimizer, meth))
    assert callable(api.window_scene) and callable(scene_io.window_trajectory) and callable(scene_io.window_scene)
    assert "1e-9" in hdr and scene_io.WINDOW_MARGIN == 1e-9


def test_host_call_is_the_numpy_statement(crafted_host):
    cases = sw.crafted()
    seen = set()
    for c, (rows, count) in zip(cases, crafted_host):
        want_rows, want_count = sw.expected(c["traj"], c["t0"], c["span"], c["out_samples"])
        assert count == want_count, (c["name"], count, want_count)
        assert sw.same_bits(rows, want_rows), c["name"]        # the sentinel behind the count, and all of it on overflow
        seen |= sw.census(c)
    assert seen == set(sw.BRANCHES), set(sw.BRANCHES) - seen
    by_name = dict(zip((c["name"] for c in cases), crafted_host))
    assert by_name["a window of exactly out_samples"][1] == sw.OUT
    assert by_name["a window of one more: overflow"][1] == -1
    assert by_name["no sample"][1] == 0 and by_name["one sample before"][1] == 1 and by_name["5000 samples"][1] > 50
    # the borders themselves: a sample at -1e-9 opens the window, one double below it is the predecessor that is kept too
    assert by_name["a sample at -1e-9"][1] == 4 and by_name["a sample one double below -1e-9"][1] == 3
    assert by_name["a sample at span + 1e-9"][1] == 4 and by_name["a sample one double above span + 1e-9"][1] == 3


def test_a_scene_of_all_cases_and_the_scene_form():
    """every case of one span in ONE scene at one t0 (with a slot of count 0 among them), against the Scene form"""
    cases = [c for c in sw.crafted() if c["span"] == sw.SPAN and c["t0"] == 0.0] + [sw.crafted()[0]]
    trajs = [c["traj"] for c in cases]
    rows, counts, n = sw.host_window(trajs, 0.0, sw.SPAN, sw.OUT)
    scene = scene_io.window_scene(sw.scene_with(trajs), 0.0, sw.SPAN)
    assert n == 0 and counts[-1] == 0
    for d, dob in enumerate(scene.dynamic):
        assert counts[d] == len(dob.trajectory) and sw.same_bits(rows[d, :counts[d]], dob.trajectory)
        assert (rows[d, counts[d]:] == sw.SENTINEL).all()
    # an overflow among them is counted, its rows stay as they were, the others are unaffected
    small, small_counts, n = sw.host_window(trajs, 0.0, sw.SPAN, 3)
    assert n == int((counts > 3).sum()) > 0 and np.array_equal(small_counts, np.where(counts > 3, -1, counts))
    for d in range(len(trajs)):
        assert sw.same_bits(small[d], np.full((3, 4), sw.SENTINEL) if counts[d] > 3 else rows[d, :3])


def _queries(rng, s_times, span):
    """knot times in [0, span]: both ends, times on samples of the shifted trajectories, within 1e-10 of them and one double
    either side"""
    q = [0.0, span, 0.5 * span]
    inside = s_times[(s_times >= 0.0) & (s_times <= span)]
    for v in rng.choice(inside, size=min(5, len(inside)), replace=False) if len(inside) else []:
        q += [v, v - 0.6e-10, v + 0.6e-10, v - 1.0e-10, v + 1.0e-10, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)]
    q += list(rng.uniform(0.0, span, 4))
    q = np.array(q)
    return np.sort(q[(q >= 0.0) & (q <= span)])


def test_the_scene_calls_cannot_tell_the_window_from_the_shifted_scene():
    rng = np.random.default_rng(20240607)
    cfg = api.default_dp_config()
    span = float(cfg.tf)
    K = int(cfg.tf / cfg.delta_t + 1)
    cut, total, hits, present = 0, 0, 0, 0
    for i in range(16):                                   # 16 scenes of four trajectories: 64 trajectories
        trajs = []
        for d in range(4):
            T = 1024 if (i, d) == (0, 0) else int(rng.integers(2, 1025))
            step = float(rng.choice([0.01, 0.02, 0.05]))
            trajs.append(sw.random_trajectory(rng, T, rng.uniform(-3.0, 40.0), step, x0=rng.uniform(8.0, 30.0), lane=rng.uniform(-2.0, 2.0)))
        lo_t, hi_t = min(t[0, 0] for t in trajs), max(t[-1, 0] for t in trajs)
        t0 = float(rng.uniform(lo_t - 1.0, hi_t + 1.0)) if i % 4 else float(trajs[0][len(trajs[0]) // 2, 0])
        scene = sw.scene_with(trajs, static=[sw.BODY + np.array([40.0, 6.0])])
        win, full = scene_io.window_scene(scene, t0, span), scene_io.shift_scene(scene, t0)
        flat_w, flat_f = scene_io.flatten_scene(sw.CENTER, win), scene_io.flatten_scene(sw.CENTER, full)
        cut += sum(len(d.trajectory) for d in win.dynamic)
        total += sum(len(d.trajectory) for d in full.dynamic)
        # the host call makes the same window
        rows, counts, _ = sw.host_window(trajs, t0, span, 1024)
        for d, dob in enumerate(win.dynamic):
            assert counts[d] == len(dob.trajectory) and sw.same_bits(rows[d, :counts[d]], dob.trajectory)
        # DpPlanner::Plan
        found_w, coarse_w = api.dp_plan(flat_w, [2.0, 0.0, 0.0], cfg)
        found_f, coarse_f = api.dp_plan(flat_f, [2.0, 0.0, 0.0], cfg)
        assert found_w == found_f and sw.same_bits(coarse_w, coarse_f) and coarse_w.shape == (K, 9), i
        # Query...ObstaclesPoints (the 1e-10 form)
        q = _queries(rng, np.concatenate([d.trajectory[:, 0] for d in full.dynamic]), span)
        for multiple in ((False, True) if i % 4 == 0 else (False,)):   # the sample points of a polygon do not read the times
            pw, cw = scene_io.environment_points(win, q, multiple)
            pf, cf = scene_io.environment_points(full, q, multiple)
            assert sw.same_bits(pw, pf) and sw.same_bits(cw, cf), i
        present += int((cw > 4).sum())
        # the audit and the clearance (the plain form): poses beside where the first obstacle is at the query time
        tr = full.dynamic[0].trajectory
        at = np.clip(np.searchsorted(tr[:, 0], q, side="right"), 0, len(tr) - 1)
        rows10 = np.zeros((len(q), 10))
        rows10[:, 0] = q
        rows10[:, 1] = tr[at, 1] - 3.0 + rng.uniform(-1.5, 1.5, len(q))
        rows10[:, 2] = tr[at, 2] + rng.uniform(-1.5, 1.5, len(q))
        mw, fw, nw = api.check_collisions(flat_w, rows10, api.ROWS_TRAJ, cfg)
        mf, ff, nf = api.check_collisions(flat_f, rows10, api.ROWS_TRAJ, cfg)
        assert sw.same_bits(mw, mf) and (fw, nw) == (ff, nf), i
        hits += nw
        cw4, nw4, lw, kw = api.clearance_rows(flat_w, rows10, api.ROWS_TRAJ, cfg)
        cf4, nf4, lf, kf = api.clearance_rows(flat_f, rows10, api.ROWS_TRAJ, cfg)
        assert sw.same_bits(cw4, cf4) and sw.same_bits(nw4, nf4) and (lw, kw) == (lf, kf), i
    print("SCENE_WINDOW_RECORD", dict(samples_full=total, samples_window=cut, knots_with_a_dynamic_polygon=present, knots_hit=hits))
    assert cut < total // 2 and hits > 50 and present > 100       # the window cuts, and the queries meet obstacles


def test_argument_checks():
    L = api.lib()
    flat = scene_io.flatten_scene(sw.CENTER, sw.scene_with([sw.traj_of([0.0, 1.0, 2.0])]))
    sc, keep = api.scene_struct(flat)
    out, counts, n = np.full((1, 4, 4), sw.SENTINEL), np.full(1, -9, np.int32), C.c_int32(-9)

    def call(scene=sc, t0=0.5, span=1.0, m=4, rows=out, cnt=counts):
        return L.cilqr_window_scene(C.byref(scene) if scene is not None else None, C.c_double(t0), C.c_double(span), m,
                                    rows.ctypes.data if rows is not None else None, cnt.ctypes.data if cnt is not None else None,
                                    C.byref(n))
    assert call(scene=None) == api.ERR_NULL and call(rows=None) == api.ERR_NULL and call(cnt=None) == api.ERR_NULL
    for bad in (dict(t0=np.nan), dict(t0=np.inf), dict(span=np.nan), dict(span=np.inf), dict(span=-1e-300), dict(m=0), dict(m=-3)):
        assert call(**bad) == api.ERR_ARG, bad
    neg, _ = api.scene_struct(dict(flat, dynamic_trajectory_counts=np.array([-1], np.int32)))
    assert call(scene=neg) == api.ERR_ARG
    no_src, _ = api.scene_struct(flat)
    no_src.dynamic_trajectories = None
    assert call(scene=no_src) == api.ERR_NULL
    assert (out == sw.SENTINEL).all() and counts[0] == -9 and n.value == -9      # every refusal wrote nothing
    assert call() == api.OK and counts[0] == 3 and n.value == 0
    assert call(span=0.0) == api.OK and counts[0] == 2
    assert L.cilqr_window_scene(C.byref(sc), C.c_double(0.5), C.c_double(1.0), 4, out.ctypes.data, counts.ctypes.data, None) == api.OK
    with pytest.raises(api.CilqrError):
        api.window_scene(flat, 0.0, -1.0, 4)
    with pytest.raises(ValueError):
        api.window_scene(flat, 0.0, 1.0, 4, np.zeros((1, 4, 4), dtype=np.float32))
    # a source of any length
    long = scene_io.flatten_scene(sw.CENTER, sw.scene_with([sw.traj_of(np.arange(100000) * 0.01)]))
    rows, cnt, over = api.window_scene(long, 512.345, 5.0, 600)
    assert cnt[0] == 502 and over == 0 and rows[0, 0, 0] < 0.0 < rows[0, 1, 0] and rows[0, 501, 0] > 5.0 > rows[0, 500, 0]


def test_cpp_program_over_the_header(tmp_path, crafted_host):
    """tests/cpp/scene_window_test.cc, built with AddressSanitizer and UndefinedBehaviorSanitizer, on the crafted table with the
    host call's results as expected values."""
    cases = sw.crafted()
    path = tmp_path / "scene_window_cases.bin"
    sw.write_cases(str(path), cases, crafted_host)
    exe = tmp_path / "scene_window_test"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scene_window_test.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{len(cases)} cases" in out.stdout and "0 failures" in out.stdout
