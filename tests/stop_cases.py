"""The case table of the stop rule (include/cilqr.h, "stop"), shared by tests/test_stop.py (host call against the NumPy
statement), tests/test_gpu_stop.py (kernel against host call) and tests/test_gpu_stop_scenes.py.  Not a test module.

A case is dict(name, layout, rows [K,F], profiles [M,2], delta_t, n_out, start_va or None, expect = the status of profile 0
or None where the table does not pin it)."""
import numpy as np

from cilqr_amd import stop
from cilqr_amd.resample import ROWS_COARSE, ROWS_PLAN, ROWS_TRAJ

LAYOUTS = (ROWS_TRAJ, ROWS_PLAN, ROWS_COARSE)
FIELDS = {ROWS_TRAJ: 10, ROWS_PLAN: 11, ROWS_COARSE: 9}


def from_plan(plan, layout):
    """plan rows [K,11] in another layout (a column the layout lacks is dropped)"""
    plan = np.ascontiguousarray(plan, dtype=np.float64)
    out = np.zeros((plan.shape[0], FIELDS[layout]))
    for col, src in enumerate(stop.TO_PLAN[layout]):
        if src is not None:
            out[:, src] = plan[:, col]
    return out


def straight(K, ds, v=8.0, a=-2.0, t0=0.0, dt=0.1):
    """plan rows of a straight path along x, ds between knots: the chord lengths are the station differences exactly"""
    plan = np.zeros((K, 11))
    plan[:, 0] = t0 + dt * np.arange(K)
    plan[:, 1] = ds * np.arange(K)
    plan[:, 2] = plan[:, 1]
    plan[:, 6], plan[:, 7] = v, a
    return plan


def arc(K, ds, kappa, theta0=0.0, v=6.0, a=-1.0, x0=3.0, y0=-2.0, t0=1.5, dt=0.1, seed=0):
    """plan rows of a circular arc with a wobbling steering column; the heading runs through +-pi when theta0 is near it"""
    rng = np.random.default_rng(seed)
    s = ds * np.arange(K)
    theta = theta0 + kappa * s
    plan = np.zeros((K, 11))
    plan[:, 0] = t0 + dt * np.arange(K)
    plan[:, 1] = s + 0.25                    # a station column that does not start at 0
    plan[:, 2] = x0 + (np.sin(theta) - np.sin(theta0)) / kappa
    plan[:, 3] = y0 - (np.cos(theta) - np.cos(theta0)) / kappa
    plan[:, 4] = theta                       # not wrapped: the rule wraps
    plan[:, 5] = kappa + 0.01 * rng.standard_normal(K)
    plan[:, 6], plan[:, 7] = v, a
    plan[:, 8] = np.arctan(2.8 * kappa) + 0.02 * rng.standard_normal(K)
    plan[:, 9:11] = rng.standard_normal((K, 2))
    return plan


GENTLE, FIRM, HARD = (-1.0, -2.0), (-2.0, -4.0), (-6.0, -20.0)


def _case(name, layout, plan, profiles, delta_t, n_out, start_va=None, expect=None):
    return dict(name=name, layout=layout, rows=from_plan(plan, layout), profiles=np.array(profiles, dtype=np.float64).reshape(-1, 2),
                delta_t=delta_t, n_out=n_out, start_va=None if start_va is None else np.array(start_va, dtype=np.float64),
                expect=expect)


def cases():
    out = []
    # ---- dyadic inputs on a straight 40 m path: every step of the rule is exact (tests/test_stop.py holds them to fractions)
    out.append(_case("constant_braking", ROWS_PLAN, straight(41, 1.0), [FIRM], 0.125, 40, expect=stop.STOPPED))
    out.append(_case("stop_inside_a_step", ROWS_PLAN, straight(41, 1.0, v=7.5), [FIRM], 0.5, 12, expect=stop.STOPPED))
    out.append(_case("jerk_ramp", ROWS_PLAN, straight(41, 1.0, a=0.0), [FIRM], 0.125, 64, expect=stop.STOPPED))
    out.append(_case("easing_off", ROWS_PLAN, straight(41, 1.0, a=-4.0), [FIRM], 0.125, 64, expect=stop.STOPPED))
    # ---- every status
    out.append(_case("overrun_short_path", ROWS_PLAN, straight(11, 1.0), [FIRM], 0.125, 40, expect=stop.OVERRUN))
    out.append(_case("moving_n_out_too_small", ROWS_PLAN, straight(41, 1.0), [FIRM], 0.125, 5, expect=stop.MOVING))
    out.append(_case("refused_nan_v0", ROWS_PLAN, straight(41, 1.0, v=np.nan), [FIRM], 0.125, 40, expect=stop.REFUSED))
    out.append(_case("refused_negative_v0", ROWS_PLAN, straight(41, 1.0, v=-0.5), [FIRM], 0.125, 40, expect=stop.REFUSED))
    out.append(_case("refused_inf_a0_start_va", ROWS_PLAN, straight(41, 1.0), [FIRM], 0.125, 40, start_va=(8.0, -np.inf),
                     expect=stop.REFUSED))
    nan_near = arc(51, 0.6, 0.05)
    nan_near[4, 5] = np.nan                  # a NaN curvature inside the stop distance: it reaches an output
    out.append(_case("refused_nan_curvature_reached", ROWS_PLAN, nan_near, [FIRM], 0.1, 51, expect=stop.REFUSED))
    nan_far = arc(51, 0.6, 0.05)
    nan_far[45, 5] = np.nan                  # ... beyond it: carried, never read into a row
    out.append(_case("carried_nan_not_reached", ROWS_PLAN, nan_far, [FIRM], 0.1, 51, expect=stop.STOPPED))
    nan_later = arc(51, 0.6, 0.05)
    nan_later[25, 5] = np.nan                # ... 15 m along: the first rows are finite and have left when a later chunk meets it
    out.append(_case("refused_nan_curvature_in_a_later_chunk", ROWS_TRAJ, nan_later, [GENTLE, FIRM], 0.1, 51, expect=stop.REFUSED))
    out.append(_case("stopped_v0_zero", ROWS_PLAN, straight(41, 1.0, v=0.0, a=0.0), [FIRM], 0.125, 8, expect=stop.STOPPED))
    out.append(_case("stopped_v0_zero_a0_left", ROWS_PLAN, straight(41, 1.0, v=0.0, a=-1.0), [FIRM], 0.125, 8, expect=stop.STOPPED))
    out.append(_case("n_out_one_standing", ROWS_PLAN, straight(41, 1.0, v=0.0), [FIRM], 0.125, 1, expect=stop.STOPPED))
    out.append(_case("n_out_one_moving", ROWS_PLAN, straight(41, 1.0), [FIRM], 0.125, 1, expect=stop.MOVING))
    # ---- a nominal plan with a standing segment: a degenerate station pair inside the stop distance, and at its end
    standing = arc(51, 0.5, -0.04, v=8.0)    # (the gentle profile runs over the end: the clamped station meets the pair there)
    standing[6:9] = standing[6]              # three knots at one station
    standing[6:9, 0] = 1.5 + 0.1 * np.arange(6, 9)
    standing[-3:, 1:9] = standing[-3, 1:9]
    for layout in LAYOUTS:
        out.append(_case(f"standing_segment_layout{layout}", layout, standing, [GENTLE, FIRM, HARD], 0.1, 51))
    # ---- every layout on a curve whose heading wraps, start_va given and absent, several profiles per call
    wrap = arc(51, 0.7, 0.09, theta0=3.0)
    for layout in LAYOUTS:
        out.append(_case(f"wrap_layout{layout}", layout, wrap, [GENTLE, FIRM, HARD], 0.1, 51))
        out.append(_case(f"wrap_start_va_layout{layout}", layout, wrap, [FIRM, HARD], 0.1, 40, start_va=(9.5, 0.75)))
    out.append(_case("eight_profiles", ROWS_TRAJ, arc(51, 0.6, 0.03, seed=3),
                     [(-0.5 * (m + 1), -1.0 - m) for m in range(8)], 0.1, 51))
    # ---- the limits of the shapes
    out.append(_case("two_knots", ROWS_COARSE, arc(2, 30.0, 0.01), [FIRM], 0.1, 51, expect=stop.STOPPED))
    out.append(_case("two_knots_n_out_one", ROWS_TRAJ, arc(2, 30.0, 0.01), [FIRM], 0.1, 1))
    out.append(_case("knots_256_n_out_256", ROWS_TRAJ, arc(256, 0.2, 0.02, v=12.0, seed=5), [GENTLE, HARD], 0.05, 256))
    out.append(_case("accelerating_start", ROWS_PLAN, arc(51, 0.9, 0.02, v=4.0, a=2.0), [GENTLE, FIRM], 0.1, 80))
    out.append(_case("already_beyond_target", ROWS_PLAN, arc(51, 0.9, 0.02, v=9.0, a=-5.0), [GENTLE], 0.1, 80))
    # ---- the first two stations exactly 1e-10 apart (1e-10 - 0.0 is 1e-10): the pair is interpolated (`<`), its heading that
    # of its first row (slerp's own `<=`); knot 0 of every chain is answered by it, and every knot of a standing start
    close = arc(51, 0.6, 0.05)
    close[:, 1] -= 0.25
    close[1, 1] = 1e-10
    for layout in (ROWS_PLAN, ROWS_COARSE):
        out.append(_case(f"stations_exactly_1e-10_apart_layout{layout}", layout, close, [GENTLE, FIRM], 0.1, 51))
    out.append(_case("stations_exactly_1e-10_apart_standing", ROWS_PLAN, close, [FIRM], 0.1, 4, start_va=(0.0, 0.0)))
    # ... and the LAST two (0.0 - -1e-10 is 1e-10): a chain that runs over the end is clamped onto the second key, w = 1, so
    # its rows are the last knot's -- a degenerate pair would give the knot before it
    short = arc(11, 0.6, 0.05)
    short[:, 1] -= short[-1, 1]
    short[-2, 1] = -1e-10
    assert short[-1, 1] == 0.0 and short[-1, 1] - short[-2, 1] == 1e-10
    for layout in (ROWS_PLAN, ROWS_COARSE):
        out.append(_case(f"last_stations_exactly_1e-10_apart_layout{layout}", layout, short, [GENTLE, FIRM], 0.1, 51, expect=stop.OVERRUN))
    # ---- headings more than 2 pi outside [-pi, pi): the library call of NormalizeAngle
    out.append(_case("headings_near_7.5_pi", ROWS_TRAJ, arc(51, 0.7, 0.09, theta0=7.5 * np.pi), [GENTLE, FIRM], 0.1, 51))
    out.append(_case("headings_near_-9.25_pi", ROWS_PLAN, arc(51, 0.7, -0.09, theta0=-9.25 * np.pi), [FIRM, HARD], 0.1, 51))
    return out


KINDS = ("long", "short", "nan_v0", "carried_nan", "short_standing_end", "nan_curvature_near", "standing", "fast",
         "nan_curvature_later")
BATCH_PROFILES = np.array([GENTLE, FIRM, HARD, (-0.5, -1.0), (-3.0, -8.0), (-4.0, -30.0), (0.0, -1.0), (-8.0, -50.0)])


def make_batch(B, K, seed):
    """plan rows [B,K,11], start_va [B,2] and the kind of every trajectory (an index into KINDS, b % 9): long paths that
    every profile stops on, paths of a few centimetres at the most that every chain overruns (one kind with its last two knots at one
    station: the clamped station meets a degenerate pair), start values and curvatures that refuse, a NaN that is carried
    without being read, a vehicle that stands, one too fast to stop in a few seconds, a NaN curvature an eighth along the path,
    which the faster chains reach after finite rows"""
    rng = np.random.default_rng(seed)
    plans, kinds = np.zeros((B, K, 11)), np.arange(B) % len(KINDS)
    start_va = np.stack([rng.uniform(1.0, 9.0, B), rng.uniform(-3.0, 1.0, B)], axis=1)
    for b in range(B):
        kind = KINDS[kinds[b]]
        tiny = kind in ("short", "short_standing_end")
        plan = arc(K, 0.0005 if tiny else (400.0 if kind == "carried_nan" else 120.0) / (K - 1), rng.uniform(0.01, 0.06) * rng.choice([-1.0, 1.0]),
                   theta0=rng.uniform(-3.2, 3.2), v=rng.uniform(4.0, 9.0), a=rng.uniform(-2.5, 1.0), seed=seed + b)
        if kind == "nan_v0":
            plan[0, 6] = np.nan
            start_va[b, 0] = np.nan
        elif kind == "carried_nan":
            plan[K - 1, 5] = np.nan          # the path is 400 m long: no chain gets to its last pair
        elif kind == "short_standing_end":
            plan[K - 1, 1:9] = plan[K - 2, 1:9]
        elif kind == "nan_curvature_near":
            plan[0, 5] = np.nan
        elif kind == "nan_curvature_later":
            plan[max(2, K // 8), 5] = np.nan
            plan[:, 6] = 9.0
            start_va[b] = (9.0, 0.0)
        elif kind == "standing":
            plan[:, 6] = 0.0
            start_va[b, 0] = 0.0
        elif kind == "fast":
            plan[:, 6] = 14.0
            start_va[b] = (14.0, 0.5)
        plans[b] = plan
    return plans, start_va, kinds


def host_batch(api, rows, layout, profiles, delta_t, n_out, start_va):
    """the host call, trajectory by trajectory, stacked profile-major like the batched call's result"""
    per = [api.stop_rows(rows[b], layout, profiles, delta_t, n_out, None if start_va is None else start_va[b])
           for b in range(rows.shape[0])]
    return {k: np.stack([p[k] for p in per], axis=1) for k in ("rows", "status", "stop_knot", "travel")}


def reference(case):
    """the NumPy statement on a case: dict(rows [M,n_out,11], status / stop_knot [M] int32, travel [M])"""
    got = [stop.stop_rows(case["rows"], case["layout"], p, case["delta_t"], case["n_out"], case["start_va"]) for p in case["profiles"]]
    return dict(rows=np.stack([g["rows"] for g in got]), status=np.array([g["status"] for g in got], np.int32),
                stop_knot=np.array([g["stop_knot"] for g in got], np.int32), travel=np.array([g["travel"] for g in got]))


def same_bits(a, b) -> bool:
    """bit for bit, with a NaN matching a NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | both_nan).all())
