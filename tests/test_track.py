"""cilqr_track_rows (include/cilqr.h, "track"; include/cilqr/tracker.hpp) on the CPU: the host call against the same rule
in plain Python (cilqr_amd/track.py) bit for bit, against the tracker oracle at STAGE_TOL on the 128 base cases of
tests/track_cases.py, the n_drive prefix and layout invariance as equalities, the failure rule and the bound of the
simulation loop, the argument checks, and the C++ adapter's own program.  No GPU.

Yardstick figures (oracle.tracker_init_guess on the 128 base cases, default configuration): the smallest DARE stopping margin
is 4.0e-6, so no case is excluded on it; the host call's distance to the oracle is printed by the test before it asserts.
"""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import track_cases as tk
import tracker_cases as tc
from cilqr_amd import api, track
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_TOL = 1e-9      # tests/test_gpu_tracker.py
MARGIN = 1e-9         # a DARE stopping test this close (relative) to its tolerance is undecidable (tests/test_gpu_tracker.py)
MAX_EXCLUDED = 2


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def crafted_host():
    """[(driven, ok)] of the host call for every crafted case: computed once, read by several tests"""
    return [tk.host(c) for c in tk.crafted()]


# ---------------------------------------------------------------------------------------------
# C1: the host call is the Python statement, bit for bit
def test_host_call_is_the_python_statement(crafted_host):
    cases = tk.crafted()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    seen_fail = 0
    for c, (driven, ok) in zip(cases, crafted_host):
        cfg, t = tk.configs(c["tracker"], c["vehicle"])
        want, want_ok = track.track_rows(cfg, t, c["rows"], c["layout"], c["start6"], c["n_drive"])
        assert ok == want_ok, c["name"]
        assert tk.same_bits(driven, want), (c["name"], np.abs(driven - want).max())
        seen_fail += not ok
        if ok:
            K = c["rows"].shape[0]
            D = K if c["n_drive"] is None else c["n_drive"]
            assert driven.shape == (D, 10) and np.all(driven[D - 1, tk.CONTROLS] == 0.0)
            assert driven[0, 0] == c["rows"][0, 0]
    assert seen_fail == 0      # every crafted case is one the tracker completes


def test_crafted_table_reaches_its_branches(crafted_host):
    """what the table is for: the clamps and the floor of the lateral model are really met"""
    by_name = {c["name"]: d for c, (d, _) in zip(tk.crafted(), crafted_host)}
    assert by_name["brakes_to_zero"][:, 4].min() == 0.0                    # v clamped at 0
    assert by_name["slow_start"][:, 4].max() < 2.0                         # v < 2 throughout
    assert by_name["start_at_upper_bounds"][0, 5] == 5.0 and by_name["start_at_lower_bounds"][0, 5] == -5.0
    assert by_name["coarse_t0_3p7"][0, 0] == 3.7
    t = by_name["traj_nonuniform"][:, 0]
    assert np.allclose(np.diff(t)[:3], [0.1, 0.15, 0.05], atol=0.011)      # kept at the first clock value past each knot
    row0 = next(c for c in tk.crafted() if c["name"] == "plan_from_row0")["rows"][0]
    assert np.array_equal(by_name["plan_from_row0"][0, 1:7], row0[[2, 3, 4, 6, 7, 8]])


# ---------------------------------------------------------------------------------------------
# C2: the host call against the oracle on the 128 base cases
def _oracle_compare(rows, start6, over, what):
    cfg, t = tk.configs({k: v for k, v in over.items() if k in tc.TRACKER_FIELDS},
                        {k: v for k, v in over.items() if k in tc.VEHICLE_FIELDS})
    worst, excluded, min_margin = 0.0, [], np.inf
    for b in range(rows.shape[0]):
        driven, ok = api.track_rows(cfg, t, rows[b], api.ROWS_TRAJ, start6[b])
        X, U, margin = orc.tracker_init_guess(start6[b, :4], rows[b, :, 1:7], None, 0.1, **over)
        assert ok, (what, b)
        err = max(np.abs(driven[:, tk.STATE] - X).max(), np.abs(driven[:-1, tk.CONTROLS] - U).max())
        min_margin = min(min_margin, margin)
        if not err < STAGE_TOL:
            assert margin < MARGIN, (what, b, err, margin)     # the only evidence that excludes: the yardstick's own
            excluded.append((b, err, margin))
            print(f"{what}: trajectory {b} excluded: oracle stopping margin {margin:.2e}, distance {err:.2e}")
            continue
        worst = max(worst, err)
    print(f"{what}: {rows.shape[0]} trajectories, largest distance to the oracle {worst:.2e}, smallest oracle margin "
          f"{min_margin:.2e}, excluded {len(excluded)}")
    assert len(excluded) <= MAX_EXCLUDED, excluded


@pytest.mark.parametrize("name,tracker,vehicle", (("default", {}, {}),) + tk.CONFIGS, ids=lambda v: v if isinstance(v, str) else "")
def test_host_call_against_the_oracle(name, tracker, vehicle):
    rows, start6 = tk.base_rows()
    assert rows.shape == (128, 51, 10)
    _oracle_compare(rows, start6, dict(tracker, **vehicle), name)


@pytest.mark.parametrize("knots", [2, 3, 6])
def test_host_call_against_the_oracle_on_prefixes(knots):
    rows, start6 = tk.base_rows(knots)
    _oracle_compare(rows[::4], start6[::4], {}, f"K={knots}")


# ---------------------------------------------------------------------------------------------
# C3 / C4: equalities
def test_n_drive_is_a_prefix(crafted_host):
    """rows 0 ... n_drive - 1 of a longer run, bit for bit, except the controls of the last row, which are those of a step the
    shorter run does not take: zero"""
    checked = 0
    for c, (full, ok) in zip(tk.crafted(), crafted_host):
        K = c["rows"].shape[0]
        if c["n_drive"] is not None or not ok or not (c["name"].endswith("_uniform") or c["name"].endswith("t0_3p7")):
            continue
        for nd in (1, 2, 6, K - 1, K):
            part, ok_p = tk.host(dict(c, n_drive=nd))
            assert ok_p and part.shape == (nd, 10)
            assert tk.same_bits(part[:nd - 1], full[:nd - 1]) and tk.same_bits(part[nd - 1, :8], full[nd - 1, :8]), (c["name"], nd)
            assert np.all(part[nd - 1, tk.CONTROLS] == 0.0)
            checked += 1
    assert checked >= 20


def test_layouts_carry_the_same_trajectory():
    N, dt = 50, 0.1
    arc, arc_s = tc.path(N, dt, 7.0, 0.05, x0=2.0, y0=1.0, th0=0.3)
    arc[:, 4], arc[:, 5] = 0.3, -0.1
    t = 1.5 + tk.axis(N + 1)
    cfg, tcfg = tk.configs()
    for start6 in (None, np.r_[tc._offset(arc, 1.0, 0.2, v=6.0), 0.4, 0.1]):
        coarse, _ = api.track_rows(cfg, tcfg, tk.make_rows(api.ROWS_COARSE, t, arc, arc_s), api.ROWS_COARSE, start6)
        plan, _ = api.track_rows(cfg, tcfg, tk.make_rows(api.ROWS_PLAN, t, arc, arc_s), api.ROWS_PLAN, start6)
        assert tk.same_bits(coarse, plan)
        traj, _ = api.track_rows(cfg, tcfg, tk.make_rows(api.ROWS_TRAJ, t, arc), api.ROWS_TRAJ, start6)
        chord, _ = api.track_rows(cfg, tcfg, tk.make_rows(api.ROWS_COARSE, t, arc, tk.chord(arc)), api.ROWS_COARSE, start6)
        assert tk.same_bits(traj, chord)
        assert not tk.same_bits(traj, coarse)      # (arc length and chord length differ on an arc: the station column is read)


# ---------------------------------------------------------------------------------------------
# C5: failure, and the bound of the loop
def test_a_clock_that_misses_knots_fails():
    c = next(c for c in tk.crafted() if c["name"] == "coarse_uniform")
    cfg, t = tk.configs(dict(sumulation_dt=0.03))
    driven = np.full((51, 10), 7.0)
    rc = api.lib().cilqr_track_rows(C.byref(cfg), C.byref(t), c["layout"], c["rows"].ctypes.data, 51, c["start6"].ctypes.data, 51,
                                    driven.ctypes.data)
    assert rc == api.ERR_STATE and np.all(driven == 0.0)
    d, ok = api.track_rows(cfg, t, c["rows"], c["layout"], c["start6"])
    assert not ok and np.all(d == 0.0)
    # the same through the Python statement
    d, ok = track.track_rows(cfg, t, c["rows"], c["layout"], c["start6"])
    assert not ok and np.all(d == 0.0)
    # ... while a prefix the clock does reach is no failure
    d, ok = api.track_rows(cfg, t, c["rows"], c["layout"], c["start6"], n_drive=1)
    assert ok


@pytest.mark.parametrize("last", [np.inf, 1e300, np.nan], ids=["inf", "1e300", "nan"])
def test_the_loop_is_bounded(last):
    """a time column the clock can never finish: the call returns promptly (at most CILQR_TRACKER_MAX_SIM_STEPS rounds)"""
    c = next(c for c in tk.crafted() if c["name"] == "K2_n_drive2")
    rows = c["rows"].copy()
    rows[1, 0] = last
    cfg, t = tk.configs(dict(max_num_iteration=1))
    t0 = time.monotonic()
    d, ok = api.track_rows(cfg, t, rows, c["layout"], c["start6"])
    elapsed = time.monotonic() - t0
    assert not ok and np.all(d == 0.0)
    assert elapsed < 5.0, elapsed
    assert api.TRACKER_MAX_SIM_STEPS == 32768 and track.MAX_SIM_STEPS == 32768
    # a NaN inside the column is no error either: the arithmetic decides
    wide = next(c for c in tk.crafted() if c["name"] == "coarse_uniform")
    rows = wide["rows"].copy()
    rows[25, 0] = last
    t0 = time.monotonic()
    api.track_rows(cfg, t, rows, wide["layout"], wide["start6"])
    assert time.monotonic() - t0 < 5.0


# ---------------------------------------------------------------------------------------------
# C6: argument checks and the agreement of header and bindings
def test_argument_checks():
    L = api.lib()
    c = next(c for c in tk.crafted() if c["name"] == "coarse_uniform")
    cfg, t = tk.configs()
    rows, s6, out = c["rows"], c["start6"], np.zeros((51, 10))

    def call(cfg_=cfg, t_=t, layout=api.ROWS_COARSE, rows_=rows.ctypes.data, K=51, start=s6.ctypes.data, D=51, out_=out.ctypes.data):
        return L.cilqr_track_rows(C.byref(cfg_) if cfg_ is not None else None, C.byref(t_) if t_ is not None else None, layout,
                                  rows_, K, start, D, out_)

    assert call() == api.OK
    assert call(start=None) == api.OK
    assert call(cfg_=None) == api.ERR_NULL and call(t_=None) == api.ERR_NULL
    assert call(rows_=None) == api.ERR_NULL and call(out_=None) == api.ERR_NULL
    for layout in (-1, api.ROWS_CONTROLS, api.ROWS_POINTS, 5):
        assert call(layout=layout) == api.ERR_ARG
    assert call(K=1, D=1) == api.ERR_ARG and call(K=0, D=0) == api.ERR_ARG
    assert call(D=0) == api.ERR_ARG and call(D=52) == api.ERR_ARG and call(D=-1) == api.ERR_ARG
    for field, value in (("sumulation_dt", 0.0), ("sumulation_dt", np.nan), ("dt", -0.1), ("tolerance", -1.0), ("weight_l", np.inf),
                         ("max_num_iteration", 0), ("max_num_iteration", api.TRACKER_MAX_ITERATIONS + 1)):
        _, bad = tk.configs({field: value})
        assert call(t_=bad) == api.ERR_ARG, field
    with pytest.raises(ValueError):
        api.track_rows(cfg, t, rows[:, :8], api.ROWS_COARSE)
    with pytest.raises(api.CilqrError):
        api.track_rows(cfg, t, rows, api.ROWS_COARSE, n_drive=0)


def test_header_and_bindings_agree():
    hdr = open(api.HEADER_PATH).read()
    L = api.lib()
    for name in ("cilqr_track_rows", "cilqr_track_rows_batch"):
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in api.EXPORTS and hasattr(L, name), name
    assert L.cilqr_abi_version() == 7 == api.ABI_VERSION
    assert int(re.search(r"#define CILQR_TRACKER_MAX_SIM_STEPS (\d+)", hdr).group(1)) == api.TRACKER_MAX_SIM_STEPS
    for meth in ("track", "track_raw"):
        assert callable(getattr(api.BatchIlqrOptimizer, meth))
    assert [track.ROWS_TRAJ, track.ROWS_PLAN, track.ROWS_COARSE] == [api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE]
    assert {k: v[0] for k, v in track.COLUMNS.items()} == api.ROWS_FIELDS


# ---------------------------------------------------------------------------------------------
# C7: the C++ adapter's own program
def test_cpp_adapter_program(tmp_path, crafted_host):
    """tests/cpp/tracker_test.cc -- a program of its own around include/cilqr/tracker.hpp -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer against the stand-in types, on the crafted table with the host call's results as expected
    values and one failing case."""
    cases = list(tk.crafted())
    expected = list(crafted_host)
    fail = dict(next(c for c in cases if c["name"] == "coarse_uniform"), tracker=dict(sumulation_dt=0.03))
    cases.append(fail)
    expected.append(tk.host(fail))
    assert not expected[-1][1]
    path = tmp_path / "track_cases.bin"
    tk.write_cases(str(path), cases, expected)
    exe = tmp_path / "tracker_test"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tracker_test.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{len(cases)} cases" in out.stdout and "0 failures" in out.stdout
