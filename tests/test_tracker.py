"""The tracker oracle (oracle/tracker_oracle.cc) against an independent statement of the same operation in long double
(tests/tracker_reference.py), on the crafted table of tests/tracker_cases.py.  No GPU: tests/test_gpu_tracker.py holds the
kernel to the oracle on the same table.

The oracle and the kernel were written from one reading of the reference's tracker (which needs Eigen and cannot be built
here); only the trajectory queries are pinned against the reference's own code (tests/test_reference_pins.py).  What these
tests add: the clock loop, both controllers, the DARE loop with its stopping rule, the clamps and the RK4 step as a second,
differently shaped statement in more precision reads them."""
import numpy as np
import pytest

import tracker_cases as tc
import tracker_reference as ref
from oracle import oracle as orc
from parity_util import traj_err

STAGE_TOL = 1e-9     # the project's stage tolerance (tests/test_gpu_parity.py)
MARGIN = 1e-9        # a DARE stopping test this close (relative) to its tolerance is undecidable: test_tracker_init_guess
LD = np.longdouble
EPS_LD, EPS_64 = float(np.finfo(LD).eps), float(np.finfo(np.float64).eps)


def _cfg(case):
    cfg = dict(zip(orc.TRACKER_CFG_FIELDS, orc.TRACKER_CFG_DEFAULT))
    cfg.update(tc.oracle_overrides(case))
    return cfg


@pytest.fixture(scope="module")
def runs():
    """every case of the table with the stations it was drawn with and with chord-length stations: (case, which, oracle
    result or None, independent result)"""
    out = []
    for case in tc.cases():
        for which, st in (("given", case["station"]), ("chord", orc.chord_stations(case["coarse"]))):
            try:
                o = orc.tracker_init_guess(case["start"], case["coarse"], st, knot_dt=case["knot_dt"], **tc.oracle_overrides(case))
            except ValueError:
                o = None
            out.append((case, which, o, ref.track(case["start"], case["coarse"], st, case["knot_dt"], _cfg(case))))
    return out


def test_table_covers_what_it_promises():
    cs = tc.cases()
    assert {c["n_steps"] for c in cs} >= {1, 2, 3, 5, 50, 100, 280}
    assert {c["knot_dt"] for c in cs} >= {0.05, 0.08, 0.1, 0.2}
    assert {c["tracker"].get("sumulation_dt", 0.01) for c in cs} >= {0.005, 0.01, 0.02, 0.025, 0.05, 0.1}
    assert {c["tracker"].get("tolerance", 0.01) for c in cs} >= {0.01, 1e-8, 0.0}
    assert {c["tracker"].get("max_num_iteration", 150) for c in cs} >= {1, 7, 150}
    assert any(c["tracker"].get("dt") == 0.05 and c["tracker"].get("preview_time") == 0.5 for c in cs)
    assert any(c["vehicle"].get("wheel_base") == 2.8 for c in cs)
    assert len({c["name"] for c in cs}) == len(cs)


def test_oracle_equals_the_independent_statement(runs):
    """X and U of every case within STAGE_TOL (traj_err: per column, relative to the column's largest entry).  A case is left
    out only when the independent statement's own smallest DARE margin is below 1e-9 -- one round more or less changes the
    gains by ~1e-2 --, and at most one case may be.  Measured: worst error 1.3e-11 (U of N280_stops), smallest margin 3.1e-5."""
    left_out, worst, smallest = [], (0.0, None), np.inf
    for case, which, o, r in runs:
        what = (case["name"], which)
        assert r["ok"], what
        assert o is not None, what
        if r["margin"] < MARGIN:
            left_out.append(what)
            continue
        smallest = min(smallest, r["margin"])
        oX, oU, _ = o
        assert np.isfinite(oX).all() and np.isfinite(oU).all(), what
        e = max(traj_err(oX, r["X"].astype(float)), traj_err(oU, r["U"].astype(float)))
        worst = max(worst, (e, what))
        assert e < STAGE_TOL, (what, e)
    print(f"tracker oracle against long double: worst error {worst[0]:.2e} at {worst[1]}, smallest DARE margin {smallest:.2e}, "
          f"left out {left_out}")
    assert len(left_out) <= 1, left_out


def test_census(runs):
    """Every branch the kernel has is taken somewhere in the table (counted in the independent statement; a count is the
    number of simulation steps, or projections, that took it)."""
    total = dict.fromkeys(ref.CENSUS, 0)
    for _, _, _, r in runs:
        for k, n in r["census"].items():
            total[k] += int(n)
    print("tracker branch census:", total)
    assert all(n > 0 for n in total.values()), total


def _models():
    cfg = dict(zip(orc.TRACKER_CFG_FIELDS, orc.TRACKER_CFG_DEFAULT))
    out = [("longitudinal", ref.longitudinal_model(cfg))]
    out += [(f"lateral v={v}", ref.lateral_model(cfg, LD(v))) for v in (0, 1.9, 2, 7, 20)]
    # the oracle sees doubles: round the models once, and hand the SAME numbers to both
    return [(name, tuple(np.asarray(m, float) for m in (A, B, Q)) + (float(R),)) for name, (A, B, Q, R) in out]


@pytest.mark.parametrize("name,model", _models(), ids=[n for n, _ in _models()])
def test_riccati_fixed_point(name, model):
    """SolveLQRProblem with tolerance 0 runs until P stops moving; its gains must be the gains of the discrete algebraic Riccati
    equation's solution, taken from the same iteration run to its fixed point in long double.

    Bound: the long double iteration's own noise at its fixed point (largest relative movement of a gain over its last 10
    rounds, at least one ulp) says how much this map amplifies one rounding; fp64 rounds 2^11 times coarser, and 100 times that
    is allowed.  Measured: noise 0 .. 5.1e-19 (up to 5 ulp of long double), so the bound is 2.2e-14 .. 1.05e-13; the
    oracle's gains are within 1.6e-16 .. 5.1e-16 of the long double ones, after 59 .. 288 rounds."""
    A, B, Q, R = model
    Al, Bl, Ql, Rl = np.asarray(A, LD), np.asarray(B, LD), np.asarray(Q, LD), LD(R)
    P, gains = Ql.copy(), []
    for _ in range(5000):
        P = ref.riccati_step(Al, Bl, Ql, Rl, P)
        gains.append(ref.gain(Al, Bl, Rl, P))
    K = gains[-1]
    noise = max(float(np.abs((g - K) / K).max()) for g in gains[-10:])
    # the fixed point satisfies the equation (in long double, to the same noise)
    residual = float(np.abs(ref.riccati_step(Al, Bl, Ql, Rl, P) - P).max() / np.abs(P).max())
    assert residual <= 100 * EPS_LD, residual
    bound = 100.0 * max(noise, EPS_LD) * (EPS_64 / EPS_LD)
    Ko, rounds, _ = orc.tracker_solve_lqr(A, B, Q, R, 0.0, 1000)
    err = float(np.abs((Ko - K) / K).max())
    print(f"{name}: long double noise {noise:.2e}, residual {residual:.2e}, bound {bound:.2e}; oracle: {rounds} rounds, error {err:.2e}")
    assert rounds < 1000          # it stopped by itself
    assert err <= bound, (err, bound)
    # the default stopping rule: as many rounds as the independent statement runs, and its gains
    Kd, rounds_d, margin_d = orc.tracker_solve_lqr(A, B, Q, R, 0.01, 150)
    Kr, rounds_r, margin_r = ref.dare_gain(A, B, Q, R, 0.01, 150)
    assert margin_r > MARGIN
    assert rounds_d == rounds_r and 1 < rounds_d < 150, (rounds_d, rounds_r)
    assert float(np.abs((Kd - Kr) / Kr).max()) <= bound
    assert margin_d == pytest.approx(margin_r, rel=1e-9)
    # and the cap alone
    for cap in (1, 7):
        Kc, rounds_c, _ = orc.tracker_solve_lqr(A, B, Q, R, 0.0, cap)
        Krc, rounds_rc, _ = ref.dare_gain(A, B, Q, R, 0.0, cap)
        assert rounds_c == rounds_rc == cap
        assert np.allclose(Kc, Krc.astype(float), rtol=bound, atol=0.0)


SIM_DT_PASS, SIM_DT_FAIL = (0.005, 0.02, 0.025, 0.05, 0.1), (0.03, 0.25)


@pytest.mark.parametrize("n_steps,knot_dt", [(50, 0.1), (80, 0.1), (50, 0.08), (3, 0.2)])
def test_time_grid_failure(n_steps, knot_dt):
    """The oracle gives up (-1, "tacker failed") exactly where the clock, replayed in plain doubles, passes fewer than K - 1
    knots -- and nowhere else."""
    K = n_steps + 1
    coarse, station = tc.path(n_steps, knot_dt, 6.0, 0.02)
    seen = set()
    for h in SIM_DT_PASS + SIM_DT_FAIL + (0.01, 0.04, 0.07, 0.2, 0.3, 1.0):
        rounds, passed = ref.clock_passes(K, knot_dt, h)
        try:
            orc.tracker_init_guess(coarse[0, :4], coarse, station, knot_dt=knot_dt, sumulation_dt=h)
            ok = True
        except ValueError:
            ok = False
        assert ok == (passed == K - 1), (h, rounds, passed)
        seen.add(ok)
        if (n_steps, knot_dt) == (50, 0.1):
            if h in SIM_DT_PASS:
                assert ok, h
            if h in SIM_DT_FAIL:
                assert not ok, h
    assert seen == {True, False}
