"""Followed trajectories with start states for cilqr_track_rows / cilqr_track_rows_batch (include/cilqr.h, "track"), shared by
tests/test_track.py (the host call against cilqr_amd/track.py and the tracker oracle) and tests/test_gpu_track.py (the
kernel against the host call).  A helper module: nothing here is collected.

A case is a dict: name, layout, rows [K,F], start6 [6] or None (row 0), n_drive or None (K), tracker = overrides of
cilqr_tracker_config, vehicle = overrides of the cilqr_config fields the tracker reads.  crafted() is the table; base() are
128 mix11 trajectories (64 scenes, each from its own and from a displaced start) as CILQR_ROWS_TRAJ rows on the axis dt * i; CONFIGS the non-default configurations
the base cases are also run under.
"""
import numpy as np

import tracker_cases as tc
from cilqr_amd import api, scenario

ROWS_TRAJ, ROWS_PLAN, ROWS_COARSE = api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE
FIELDS = {ROWS_TRAJ: 10, ROWS_PLAN: 11, ROWS_COARSE: 9}
# layout -> the columns of x y theta v a delta
COLS = {ROWS_TRAJ: (1, 2, 3, 4, 5, 6), ROWS_PLAN: (2, 3, 4, 6, 7, 8), ROWS_COARSE: (2, 3, 4, 6, 7, 8)}
# columns of a driven row (CILQR_ROWS_TRAJ)
STATE, CONTROLS = slice(1, 7), slice(8, 10)

# every case of tests/tracker_cases.py with a short horizon, and these of its N = 50 table
LIFTED = ("arc_left", "through_pi", "exactly_pi_offset", "stopped", "stopped_moving_start", "stops_halfway", "slow_1mps",
          "offset_start", "start_far_faster", "standing_start", "curvature_0p3_right", "start_beyond_the_end",
          "start_before_the_path", "dt0.08_offset", "sim0.02_arc", "sim0.05_offset", "tol0.0_cap7_arc", "tol0.01_cap1_slow_offset",
          "weights_offset", "vehicle_tight", "vehicle_far_faster")

TRACKER_A = dict(weight_l=0.7, weight_theta=0.3, weight_delta=0.05, weight_delta_rate=0.4, preview_time=0.5, weight_s=0.2,
                 weight_v=0.6, weight_a=0.03, weight_j=0.25, dt=0.05)
TRACKER_B = dict(sumulation_dt=0.02, tolerance=1e-6, max_num_iteration=40)
VEHICLE_A = dict(wheel_base=2.8, delta_min=-0.5, delta_max=0.45, delta_rate_min=-0.3, delta_rate_max=0.25, jerk_min=-6.0,
                 jerk_max=4.0, min_acceleration=-3.0, max_acceleration=2.0)
# (name, tracker overrides, vehicle overrides): two non-default tracker configurations and one non-default vehicle
CONFIGS = (("tracker_a", TRACKER_A, {}), ("tracker_b", TRACKER_B, {}), ("vehicle_a", {}, VEHICLE_A))


def make_rows(layout, times, coarse, station=None, controls=(0.37, -0.11)):
    """coarse [K,6] = x y theta v a delta -> rows [K,F] of `layout`.  The columns the rule does not read (kappa, the controls)
    hold numbers that would show if it did."""
    coarse = np.asarray(coarse, float)
    K = coarse.shape[0]
    r = np.zeros((K, FIELDS[layout]))
    r[:, 0] = times
    if layout == ROWS_TRAJ:
        r[:, 1:7] = coarse
        r[:, 7] = 0.77
        r[:, 8:10] = controls
    else:
        r[:, 1] = station
        r[:, 2:5] = coarse[:, :3]
        r[:, 5] = 0.77
        r[:, 6:9] = coarse[:, 3:6]
        if layout == ROWS_PLAN:
            r[:, 9:11] = controls
    return r


def chord(coarse):
    """the accumulated chord length as cilqr_amd/track.py evaluates it"""
    from cilqr_amd import track
    s = np.zeros(len(coarse))
    for k in range(1, len(coarse)):
        s[k] = s[k - 1] + track.hypot_ref(coarse[k, 0] - coarse[k - 1, 0], coarse[k, 1] - coarse[k - 1, 1])
    return s


def _case(name, layout, rows, start6=None, n_drive=None, tracker=None, vehicle=None):
    return dict(name=name, layout=layout, rows=np.ascontiguousarray(rows), start6=None if start6 is None else np.asarray(start6, float),
                n_drive=n_drive, tracker=dict(tracker or {}), vehicle=dict(vehicle or {}))


def axis(K, dt=0.1):
    return np.array([dt * i for i in range(K)])   # the bits of dt * i, as k_init_guess_tracker forms them


_CRAFTED = []


def crafted():
    if _CRAFTED:
        return _CRAFTED
    out = _CRAFTED
    # ---- tests/tracker_cases.py lifted into rows: CILQR_ROWS_COARSE with the stations the paths were drawn with
    for c in tc.cases():
        if c["n_steps"] <= 5 or c["name"] in LIFTED:
            K = c["n_steps"] + 1
            out.append(_case("lifted_" + c["name"], ROWS_COARSE, make_rows(ROWS_COARSE, axis(K, c["knot_dt"]), c["coarse"], c["station"]),
                             np.r_[c["start"], 0.0, 0.0], tracker=c["tracker"], vehicle=c["vehicle"]))
    N, dt = 50, 0.1
    K = N + 1
    arc, arc_s = tc.path(N, dt, 7.0, 0.05, x0=2.0, y0=1.0, th0=0.3)
    arc[:, 4] = 0.4 * np.sin(np.arange(K))        # a and delta of the rows: read of row 0 only, and only without start6
    arc[:, 5] = 0.1 * np.cos(np.arange(K))
    off = np.r_[tc._offset(arc, 1.0, 0.2, v=6.0), 0.0, 0.0]
    uniform = axis(K)
    steps = np.resize([0.1, 0.15, 0.05], N)
    nonuniform = np.concatenate([[0.0], np.cumsum(steps)])          # 0, 0.1, 0.25, 0.3, ...
    twice = uniform.copy()
    twice[11] = twice[10]                                            # two equal consecutive times
    for layout in (ROWS_TRAJ, ROWS_PLAN, ROWS_COARSE):
        tag = {ROWS_TRAJ: "traj", ROWS_PLAN: "plan", ROWS_COARSE: "coarse"}[layout]
        out.append(_case(f"{tag}_uniform", layout, make_rows(layout, uniform, arc, arc_s), off))
        out.append(_case(f"{tag}_from_row0", layout, make_rows(layout, uniform, arc, arc_s)))
        out.append(_case(f"{tag}_t0_3p7", layout, make_rows(layout, 3.7 + uniform, arc, arc_s), off))
        out.append(_case(f"{tag}_nonuniform", layout, make_rows(layout, nonuniform, arc, arc_s), off))
        out.append(_case(f"{tag}_equal_times", layout, make_rows(layout, twice, arc, arc_s), off))
        for nd in (1, 2):
            out.append(_case(f"{tag}_n_drive{nd}", layout, make_rows(layout, uniform, arc, arc_s), off, n_drive=nd))
    # two equal consecutive stations (and points): the path stands still for one step
    v = np.full(K, 6.0)
    v[20] = 0.0
    still, still_s = tc.path(N, dt, v, 0.03)
    out.append(_case("equal_stations", ROWS_COARSE, make_rows(ROWS_COARSE, uniform, still, still_s), np.r_[still[0, :4], 0.0, 0.0]))
    out.append(_case("equal_stations_chord", ROWS_TRAJ, make_rows(ROWS_TRAJ, uniform, still), np.r_[still[0, :4], 0.0, 0.0]))
    # the start's a and delta, each at a bound of the default vehicle
    d40 = 40.0 / 180 * np.pi
    out.append(_case("start_at_upper_bounds", ROWS_COARSE, make_rows(ROWS_COARSE, uniform, arc, arc_s), np.r_[arc[0, :4], 5.0, d40]))
    out.append(_case("start_at_lower_bounds", ROWS_TRAJ, make_rows(ROWS_TRAJ, uniform, arc), np.r_[arc[0, :4], -5.0, -d40]))
    out.append(_case("start_at_bounds_vehicle", ROWS_PLAN, make_rows(ROWS_PLAN, uniform, arc, arc_s), np.r_[arc[0, :4], 2.0, -0.5],
                     vehicle=VEHICLE_A))
    # v < 2 (the lateral model's floor), and v clamped at 0: a slow start that brakes at the bound
    slow, slow_s = tc.path(N, dt, 1.0, 0.1)
    out.append(_case("slow_start", ROWS_COARSE, make_rows(ROWS_COARSE, uniform, slow, slow_s), [0.0, 0.2, 0.1, 1.5, 0.0, 0.05]))
    out.append(_case("brakes_to_zero", ROWS_COARSE, make_rows(ROWS_COARSE, uniform, slow, slow_s), [0.0, -0.2, 0.0, 0.5, -5.0, 0.0]))
    # K = 2 and K = 3, with every n_drive
    for n in (1, 2):
        short, short_s = tc.path(n, dt, 6.0, 0.05, th0=-0.4)
        s6 = np.r_[tc._offset(short, 0.3, 0.1), 0.2, -0.05]
        for nd in range(1, n + 2):
            out.append(_case(f"K{n + 1}_n_drive{nd}", ROWS_PLAN, make_rows(ROWS_PLAN, axis(n + 1), short, short_s), s6, n_drive=nd))
            out.append(_case(f"K{n + 1}_chord_n_drive{nd}", ROWS_TRAJ, make_rows(ROWS_TRAJ, 1.0 + axis(n + 1), short), s6, n_drive=nd))
    return out


_BASE = []


def base():
    """[(start4, coarse [K,6])]: scenario.generate("mix11", 64, seed=5), each problem once from its own start and once from a
    displaced one -- 128 trajectories of 51 knots on the axis 0.1 * i."""
    if not _BASE:
        sc = scenario.generate("mix11", 64, seed=5)
        rng = np.random.default_rng(1)
        for b in range(64):
            _BASE.append((sc["start"][b].copy(), sc["coarse"][b]))
        for b in range(64):
            _BASE.append((sc["start"][b] + np.array([0.3, -0.4, 0.08, 1.0]) * rng.uniform(-1, 1, 4), sc["coarse"][b]))
    return _BASE


def base_rows(knots=None):
    """(rows [128,K,10] CILQR_ROWS_TRAJ, start6 [128,6]) of base(), the first `knots` knots of every trajectory"""
    b = base()
    K = b[0][1].shape[0] if knots is None else knots
    rows = np.stack([make_rows(ROWS_TRAJ, axis(K), c[:K]) for _, c in b])
    start6 = np.stack([np.r_[s, 0.0, 0.0] for s, _ in b])
    return rows, start6


def configs(tracker=None, vehicle=None, n_steps=50):
    """(api.Config, api.TrackerConfig) with the overrides of a case"""
    import ctypes as C
    cfg = api.default_config(n_steps, **(vehicle or {}))
    t = api.TrackerConfig()
    api.lib().cilqr_default_tracker_config(C.byref(t))
    for k, v in (tracker or {}).items():
        setattr(t, k, v)
    return cfg, t


def host(case):
    """(driven, ok) of the host call for a case"""
    cfg, t = configs(case["tracker"], case["vehicle"])
    return api.track_rows(cfg, t, case["rows"], case["layout"], case["start6"], case["n_drive"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def write_cases(path, cases, expected):
    """The cases as tests/cpp/tracker_test.cc reads them (little-endian): "TKCASE01", i32 n; per case i32 layout, i32 K,
    i32 n_drive, i32 has_start, 13 doubles of the tracker configuration (cilqr_tracker_config's order, max_num_iteration as a
    double), 9 doubles of the vehicle (tracker_cases.VEHICLE_FIELDS), rows [K][F], start6 [6] if has_start, i32 ok,
    expected [n_drive][10]."""
    import struct
    with open(path, "wb") as f:
        f.write(b"TKCASE01" + struct.pack("<i", len(cases)))
        for c, (driven, ok) in zip(cases, expected):
            cfg, t = configs(c["tracker"], c["vehicle"])
            K = c["rows"].shape[0]
            D = K if c["n_drive"] is None else c["n_drive"]
            f.write(struct.pack("<4i", c["layout"], K, D, int(c["start6"] is not None)))
            f.write(np.array([getattr(t, k) for k in tc.TRACKER_FIELDS], "<f8").tobytes())
            f.write(np.array([getattr(cfg, k) for k in tc.VEHICLE_FIELDS], "<f8").tobytes())
            f.write(np.ascontiguousarray(c["rows"], "<f8").tobytes())
            if c["start6"] is not None:
                f.write(np.ascontiguousarray(c["start6"], "<f8").tobytes())
            f.write(struct.pack("<i", int(ok)))
            f.write(np.ascontiguousarray(driven, "<f8").tobytes())
