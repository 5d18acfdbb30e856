"""GPU tests of the tracker init guess (k_init_guess_tracker, CILQR_INIT_TRACKER) through the C-ABI: the crafted table of
tests/tracker_cases.py under every configuration it names, one batch of 65536 distinct problems, whole solves started from
it on both solve loops, submitted solves and a pool, station handling, hostile inputs and the argument checks of
cilqr_set_tracker_config.

The oracle is oracle/tracker_oracle.cc, which tests/test_tracker.py holds to an independent long double statement on the
same table.  Every tolerance is STAGE_TOL or STEP_TOL of the project; a problem is left out of a stage comparison only on
evidence from the oracle itself (a DARE stopping test within 1e-9 of its tolerance, or a result that moves under a 4e-16
perturbation of its inputs), and the number left out is bounded."""
import ctypes as C
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tracker_cases as tc
from cilqr_amd import api, scenario
from oracle import oracle as orc
from parity_util import PERTURB_EPS, N_PERTURB, assert_steps, oracle_cfg_from, traj_err

pytestmark = pytest.mark.gpu
STAGE_TOL = 1e-9     # tests/test_gpu_parity.py
MARGIN = 1e-9        # a DARE stopping test this close (relative) to its tolerance is undecidable (test_tracker_init_guess)
ITER_CAP = 48
CMAX = 16
WORKERS = int(os.environ.get("OMP_NUM_THREADS") or 16)
INT32_MAX = 2 ** 31 - 1

_TAIL = [None]       # which solve loop: None = the product default (the per-problem tail kernel at these sizes), 0 = lockstep


@pytest.fixture(params=["tail", "lockstep"])
def both_paths(request):
    _TAIL[0] = None if request.param == "tail" else 0
    yield request.param
    _TAIL[0] = None


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def lanes():
    sc = scenario.generate("mix11", 1, seed=1)
    return sc["left"], sc["right"]


def _handle(n_steps, capacity, knot_dt=0.1, vehicle=None, tracker=None, cmax=CMAX):
    cfg = api.default_config(n_steps, init_guess=api.INIT_TRACKER, dt=knot_dt, **(vehicle or {}))
    opt = api.BatchIlqrOptimizer(cfg, batch_capacity=capacity, cmax=cmax, max_lane_segments=64)
    if _TAIL[0] is not None:
        opt.set_option(api.OPT_TAIL_THRESHOLD, _TAIL[0])
    if tracker is not None:
        opt.set_tracker_config(**tracker)
    return opt


def _scene(start, coarse, lanes, station=None, cmax=CMAX):
    coarse = np.ascontiguousarray(coarse)
    cor, cnt = tc.box_corridors(coarse, cmax)
    sc = dict(start=np.ascontiguousarray(start), coarse=coarse, corridor=cor, ccount=cnt, left=lanes[0], right=lanes[1],
              n_steps=coarse.shape[1] - 1, cmax=cmax)
    if station is not None:
        sc["coarse_station"] = np.ascontiguousarray(station)
    return sc


def _init_guess(opt, sc):
    opt.stage_load(sc)
    opt.stage_init_guess()
    return opt.read(api.T_X), opt.read(api.T_U)


# ---------------------------------------------------------------------------------------------
# the crafted table
# ---------------------------------------------------------------------------------------------
def _group_id(key, cases):
    n, dt, tr, veh = key
    what = ",".join(f"{k}={v}" for k, v in tr[:3]) + ("..." if len(tr) > 3 else "")
    return f"N{n}-dt{dt}-{what or ('vehicle' if veh else 'defaults')}"


GROUPS = tc.groups()


@pytest.mark.parametrize("key,cases", GROUPS, ids=[_group_id(k, c) for k, c in GROUPS])
def test_table_through_the_stages(key, cases, lanes):
    """stage_load -> set_tracker_config -> stage_init_guess -> read(T_X / T_U) of every case of one configuration against
    orc.tracker_init_guess with the same overrides at STAGE_TOL, with the stations the paths were drawn with and with
    chord-length stations.  Then the same cases repeated to 131 problems in a handle of capacity 200 (256 slots, three
    workgroups, every case at several lanes of several wavefronts), the configuration set BEFORE the load this time: every copy
    equals the first run bit for bit."""
    n_steps, knot_dt, tracker, vehicle = key[0], key[1], dict(key[2]), dict(key[3])
    n = len(cases)
    start = np.stack([c["start"] for c in cases])
    coarse = np.stack([c["coarse"] for c in cases])
    for with_station in (True, False):
        station = np.stack([c["station"] for c in cases]) if with_station else None
        opt = _handle(n_steps, n, knot_dt, vehicle)
        sc = _scene(start, coarse, lanes, station)
        opt.stage_load(sc)
        opt.set_tracker_config(**tracker)               # between the load and the launch: the stations stay
        opt.stage_init_guess()
        X, U = opt.read(api.T_X), opt.read(api.T_U)
        opt.close()
        left_out, worst = [], 0.0
        for b, c in enumerate(cases):
            oX, oU, margin = orc.tracker_init_guess(c["start"], c["coarse"], c["station"] if with_station else None,
                                                    knot_dt=knot_dt, **tc.oracle_overrides(c))
            if margin < MARGIN:
                left_out.append(c["name"])
                continue
            e = max(traj_err(X[b], oX), traj_err(U[b], oU))
            worst = max(worst, e)
            assert e < STAGE_TOL, (c["name"], with_station, e)
        assert len(left_out) <= 1, left_out
        print(f"{_group_id(key, cases)} stations {with_station}: worst stage error {worst:.2e} over {n - len(left_out)} cases, "
              f"left out {left_out}")
        # the same cases across workgroups, in a handle whose capacity is not its batch
        B2 = 131
        pick = np.arange(B2) % n
        opt = _handle(n_steps, 200, knot_dt, vehicle, tracker)
        X2, U2 = _init_guess(opt, _scene(start[pick], coarse[pick], lanes, None if station is None else station[pick]))
        opt.close()
        assert np.array_equal(X2, X[pick]) and np.array_equal(U2, U[pick]), (with_station, "repeats differ")


# ---------------------------------------------------------------------------------------------
# scale
# ---------------------------------------------------------------------------------------------
def _scale_batch(B, seed=4242, share=4):
    """start [B,4] and coarse [B,51,6] of scenario mix11; every `share`-th problem replaced by an arc drawn from a seeded
    generator (speeds 0..14, headings -pi..pi, curvature -0.08..0.08) with the start moved off its first knot by up to
    0.3 m, 0.1 rad and 1 m/s."""
    chunk = 4096
    parts = [scenario.generate("mix11", min(chunk, B - c0), seed=seed, first_problem=c0, workers=min(8, WORKERS)) for c0 in range(0, B, chunk)]
    start = np.concatenate([p["start"] for p in parts])
    coarse = np.concatenate([p["coarse"] for p in parts])
    K, dt = coarse.shape[1], 0.1
    rng = np.random.default_rng(seed)
    idx = np.arange(0, B, share)
    m = len(idx)
    v, th, kap = rng.uniform(0.0, 14.0, m), rng.uniform(-np.pi, np.pi, m), rng.uniform(-0.08, 0.08, m)
    x, y = rng.uniform(-50.0, 50.0, m), rng.uniform(-50.0, 50.0, m)
    arc = np.zeros((m, K, 6))
    for k in range(K):
        arc[:, k, 0], arc[:, k, 1], arc[:, k, 3] = x, y, v
        arc[:, k, 2] = (th + np.pi) % (2.0 * np.pi) - np.pi
        x, y, th = x + v * np.cos(th) * dt, y + v * np.sin(th) * dt, th + v * kap * dt
    coarse[idx] = arc
    s0 = arc[:, 0, :4].copy()
    d = rng.uniform(-1.0, 1.0, (m, 4)) * np.array([0.3, 0.3, 0.1, 1.0])
    s0 += d
    s0[:, 3] = np.maximum(s0[:, 3], 0.0)
    start[idx] = s0
    return np.ascontiguousarray(start), np.ascontiguousarray(coarse)


def test_scale_65536(lanes):
    """One batch of 65536 distinct problems (N = 50, chord stations), every one against the oracle at STAGE_TOL.  A problem
    above it is excused only by the oracle: its smallest DARE margin is below 1e-9, or its own result moves by more than
    STAGE_TOL / 10 under the 4e-16 input perturbation of parity_util (8 samples); at most 0.1 % may be.

    The launch at full size has a limit of its own: the same kernel is timed on the first 4096 problems (64 workgroups: the
    machine is not full, so full size cannot take more than 16 times as long), and the full batch is launched only if 16 times
    that is below 60 s."""
    B = 65536
    start, coarse = _scale_batch(B)
    assert len(np.unique(np.concatenate([start, coarse.reshape(B, -1)], axis=1), axis=0)) == B
    sc = _scene(start, coarse, lanes, cmax=4)
    opt = _handle(50, B, cmax=4)
    small = {k: (v[:4096] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in sc.items()}
    opt.stage_load(small)
    t0 = time.perf_counter()
    opt.stage_init_guess()
    t_small = time.perf_counter() - t0
    Xs = opt.read(api.T_X)
    assert 16.0 * t_small < 60.0, f"4096 problems took {t_small:.3f} s: the full batch is not launched"
    opt.stage_load(sc)
    t0 = time.perf_counter()
    opt.stage_init_guess()
    t_full = time.perf_counter() - t0
    X, U = opt.read(api.T_X), opt.read(api.T_U)
    opt.close()
    assert np.array_equal(X[:4096], Xs)                         # the size of the batch does not change a problem's result
    print(f"k_init_guess_tracker: {t_small * 1e3:.2f} ms for 4096 problems, {t_full * 1e3:.2f} ms for {B} (launch + wait, wall clock)")

    def run(b):
        oX, oU, margin = orc.tracker_init_guess(start[b], coarse[b])
        return max(traj_err(X[b], oX), traj_err(U[b], oU)), margin

    with ThreadPoolExecutor(WORKERS) as pool:
        res = list(pool.map(run, range(B), chunksize=256))
    err = np.array([r[0] for r in res])
    margin = np.array([r[1] for r in res])
    above = np.nonzero(~(err < STAGE_TOL))[0]
    excused, failed = [], []
    rng = np.random.default_rng(99)
    for b in above:
        why = "margin" if margin[b] < MARGIN else None
        if why is None:
            oX, oU, _ = orc.tracker_init_guess(start[b], coarse[b])
            for _ in range(N_PERTURB):
                pX, pU, _ = orc.tracker_init_guess(start[b] * (1.0 + PERTURB_EPS * rng.standard_normal(4)),
                                                   coarse[b] * (1.0 + PERTURB_EPS * rng.standard_normal(coarse[b].shape)))
                if max(traj_err(pX, oX), traj_err(pU, oU)) > STAGE_TOL / 10:
                    why = "oracle moves"
                    break
        (excused if why else failed).append((int(b), float(err[b]), why))
    ok = err < STAGE_TOL
    print(f"scale: worst stage error {err[ok].max():.2e} over {int(ok.sum())} problems, smallest DARE margin {margin.min():.2e}, "
          f"excused {len(excused)} {excused[:8]}, failed {len(failed)}")
    assert not failed, failed[:8]
    assert len(excused) <= B // 1000, excused[:8]


# ---------------------------------------------------------------------------------------------
# whole solves
# ---------------------------------------------------------------------------------------------
def _stations(sc):
    """stations that are NOT the chord lengths: the arc length of a circle through consecutive points would be a few 1e-4
    longer; 2 % longer is plainly another projection"""
    return np.stack([orc.chord_stations(c) for c in sc["coarse"]]) * 1.02


def _tracker_opt(sc, capacity=None):
    cfg = api.default_config(sc["n_steps"], init_guess=api.INIT_TRACKER)
    opt = api.BatchIlqrOptimizer(cfg, batch_capacity=capacity or sc["coarse"].shape[0], cmax=sc["cmax"], max_lane_segments=64)
    if _TAIL[0] is not None:
        opt.set_option(api.OPT_TAIL_THRESHOLD, _TAIL[0])
    return opt


KEYS = ("traj", "cost_hist", "n_cost", "status", "n_iter", "alpha_trace", "iter_trajs", "n_iter_trajs")


@pytest.mark.parametrize("family,B,seed", [("mix11", 120, 311), ("ped6", 120, 312), ("dyn20x", 100, 313)])
def test_whole_solves_from_the_tracker(family, B, seed, both_paths):
    """Solves started from the tracker's init guess on both solve loops: iterate 0 is the staged init guess bit for bit, every
    step replays in the oracle from the device's own iterates (assert_steps, STEP_TOL), and the stations are used."""
    sc = scenario.generate(family, B, seed=seed)
    opt = _tracker_opt(sc)
    X, U = _init_guess(opt, sc)
    for b in range(0, B, 9):
        oX, oU, margin = orc.tracker_init_guess(sc["start"][b], sc["coarse"][b], knot_dt=sc["dt"])
        if margin >= MARGIN:
            assert traj_err(X[b], oX) < STAGE_TOL and traj_err(U[b], oU) < STAGE_TOL, b
    res = opt.plan(sc, max_iter_trajs=ITER_CAP, alpha_trace=True)
    assert ((res["status"] >= 1) & (res["status"] <= 5)).all()
    assert np.array_equal(res["iter_trajs"][:, 0, :, 1:7], X)
    assert np.array_equal(res["iter_trajs"][:, 0, :-1, 8:10], U)
    rep = assert_steps(res, sc, oracle_cfg_from(opt.cfg), what=f"{family} from the tracker ({both_paths})")
    with_st = dict(sc, coarse_station=_stations(sc))
    Xs, _ = _init_guess(opt, with_st)
    assert not np.array_equal(Xs, X)
    res_st = opt.plan(with_st, max_iter_trajs=ITER_CAP, alpha_trace=True)
    assert np.array_equal(res_st["iter_trajs"][:, 0, :, 1:7], Xs)
    print(f"{family} ({both_paths}): steps {rep}")
    opt.close()


def _outputs(opt, B):
    K, M = opt.K, opt.cfg.max_iter
    o = dict(traj=np.full((B, K, 10), -7.0), cost_hist=np.full((B, M + 1, 5), -7.0), n_cost=np.full(B, -1, np.int32),
             status=np.full(B, -1, np.int32), n_iter=np.full(B, -1, np.int32), iter_trajs=np.full((B, ITER_CAP, K, 10), -7.0),
             n_iter_trajs=np.full(B, -1, np.int32), alpha_trace=np.full((B, M), 9, np.int8))
    sol = api.SolutionBatch(api.MEM_HOST, ITER_CAP, *(o[k].ctypes.data for k in ("traj", "cost_hist", "n_cost", "status", "n_iter",
                                                                                "iter_trajs", "n_iter_trajs", "alpha_trace")))
    return o, sol


def _same_solve(got, ref, what):
    """bit for bit, in what a solve defines: rows and iterates beyond the counts belong to nobody"""
    for k in ("n_cost", "status", "n_iter", "n_iter_trajs", "traj", "alpha_trace"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    for b in range(len(ref["n_cost"])):
        assert np.array_equal(got["cost_hist"][b, :ref["n_cost"][b]], ref["cost_hist"][b, :ref["n_cost"][b]]), (what, b)
        n = min(int(ref["n_iter_trajs"][b]), ITER_CAP)
        assert np.array_equal(got["iter_trajs"][b, :n], ref["iter_trajs"][b, :n]), (what, b)


@pytest.mark.parametrize("family,B,seed", [("mix11", 120, 311), ("dyn20x", 100, 313)])
def test_submitted_solves_keep_their_own_stations(family, B, seed, both_paths):
    """Two solves in flight on one handle, one with stations and one without, back to back in both orders, and the same two
    through a pool of two handles: each equals its cilqr_solve_batch result bit for bit.  (have_station is handle state that
    the load of a later solve rewrites: each solve's launch must carry its own.)"""
    plain = scenario.generate(family, B, seed=seed)
    with_st = dict(plain, coarse_station=_stations(plain))
    opt = _tracker_opt(plain)
    ref = {"plain": opt.plan(plain, max_iter_trajs=ITER_CAP, alpha_trace=True),
           "stations": opt.plan(with_st, max_iter_trajs=ITER_CAP, alpha_trace=True)}
    assert not np.array_equal(ref["plain"]["traj"], ref["stations"]["traj"])
    scenes = {"plain": plain, "stations": with_st}
    probs = {k: opt._host_problem(v) for k, v in scenes.items()}
    for order in (("stations", "plain"), ("plain", "stations"), ("stations", "plain", "stations")):
        outs = [_outputs(opt, B) for _ in order]
        for name, (_, sol) in zip(order, outs):
            assert opt.submit_raw(probs[name][0], sol) == api.OK
        for _ in order:
            assert opt.wait() == api.OK
        for name, (o, _) in zip(order, outs):
            _same_solve(o, ref[name], (order, name))
    opt.close()
    pool = api.HandlePool(api.default_config(plain["n_steps"], init_guess=api.INIT_TRACKER), device=0, handles=2, batch_capacity=B,
                          cmax=plain["cmax"], max_lane_segments=64)
    if _TAIL[0] is not None:
        pool.set_option(api.OPT_TAIL_THRESHOLD, _TAIL[0])
    order = ("stations", "plain", "plain", "stations")
    outs = [_outputs(opt, B) for _ in order]
    for name, (_, sol) in zip(order, outs):
        assert pool.submit_raw(probs[name][0], sol) == api.OK
    for _ in order:
        assert pool.wait() == api.OK
    for name, (o, _) in zip(order, outs):
        _same_solve(o, ref[name], ("pool", name))
    pool.close()


# ---------------------------------------------------------------------------------------------
# stations, hostile inputs, arguments
# ---------------------------------------------------------------------------------------------
def _table_scene(lanes, stations=True):
    cases = [c for k, cs in GROUPS if k == (50, 0.1, (), ()) for c in cs]
    assert len(cases) >= 12
    return _scene(np.stack([c["start"] for c in cases]), np.stack([c["coarse"] for c in cases]), lanes,
                  np.stack([c["station"] for c in cases]) if stations else None)


def test_station_handling(lanes):
    with_st, plain = _table_scene(lanes), _table_scene(lanes, stations=False)
    B = with_st["coarse"].shape[0]
    opt = _handle(50, B + 5)
    Xs, Us = _init_guess(opt, with_st)
    Xp, Up = _init_guess(opt, plain)                       # stations, then none: chord lengths are recomputed
    assert not np.array_equal(Xs, Xp)
    chord = dict(plain, coarse_station=np.stack([orc.chord_stations(c) for c in plain["coarse"]]))
    Xc, Uc = _init_guess(opt, chord)                       # none, then stations: the caller's are used
    assert traj_err(Xc, Xp) < STAGE_TOL and traj_err(Uc, Up) < STAGE_TOL   # (chord lengths summed on the host)
    X2, U2 = _init_guess(opt, with_st)
    assert np.array_equal(X2, Xs) and np.array_equal(U2, Us)
    # cilqr_set_tracker_config between the load and the launch leaves the stations alone
    opt.stage_load(with_st)
    opt.set_tracker_config()
    opt.stage_init_guess()
    assert np.array_equal(opt.read(api.T_X), Xs) and np.array_equal(opt.read(api.T_U), Us)
    opt.stage_load(plain)
    opt.set_tracker_config()
    opt.stage_init_guess()
    assert np.array_equal(opt.read(api.T_X), Xp)
    opt.close()


def test_hostile_inputs_stay_in_their_lane(lanes):
    """NaN and +-1e300 in the coarse x / y / theta / v, the stations and the start of a few problems of a batch of 130: the
    call returns, and every other problem's output is bit-identical to a clean batch.

    Read beforehand: every loop of k_init_guess_tracker is bounded by something that is not data.  The chord-length sum and the
    nearest-knot search run K rounds; solve_lqr at most max_num_iteration (a NaN `diff` ends it: `diff > tolerance` is false);
    the clock loop runs on t and sumulation_dt alone (bounded by cilqr_set_tracker_config); the two `while` loops of the time
    lookup move an index between 0 and K - 1 on the clock's time, which the branch before them keeps below the last knot's
    time; normalize_angle and slerp are straight-line code (fmod), lean_sincos / lean_tan reduce with one rint.  Nothing is
    indexed by a value computed from the data except `idx`, which stays the 0 it starts at when no distance compares below
    DBL_MAX."""
    base = _table_scene(lanes)
    n, B = base["coarse"].shape[0], 130
    pick = np.arange(B) % n
    for with_station in (True, False):
        clean = _scene(base["start"][pick], base["coarse"][pick], lanes, base["coarse_station"][pick] if with_station else None)
        opt = _handle(50, B)
        Xc, Uc = _init_guess(opt, clean)
        assert np.isfinite(Xc).all() and np.isfinite(Uc).all()
        bad = dict(clean, start=clean["start"].copy(), coarse=clean["coarse"].copy())
        if with_station:
            bad["coarse_station"] = clean["coarse_station"].copy()
        hit = []
        poison = [np.nan, 1e300, -1e300, np.inf]
        for j, b in enumerate(range(3, B, 11)):
            val = poison[j % len(poison)]
            col = j % 6
            if col < 4:
                bad["coarse"][b, (7 * j) % 51, col] = val
            elif col == 4:
                bad["start"][b, j % 4] = val
            elif with_station:
                bad["coarse_station"][b, (5 * j) % 51] = val
            else:
                bad["coarse"][b, :, 0] = val
            hit.append(b)
        X, U = _init_guess(opt, bad)                      # returns
        keep = np.setdiff1d(np.arange(B), hit)
        assert np.array_equal(X[keep], Xc[keep]) and np.array_equal(U[keep], Uc[keep]), with_station
        X3, U3 = _init_guess(opt, clean)                  # and the handle is as good as before
        assert np.array_equal(X3, Xc) and np.array_equal(U3, Uc)
        opt.close()


def test_set_tracker_config_argument_checks(lanes):
    """Refused without a launch: a null config, non-finite fields, max_num_iteration above CILQR_TRACKER_MAX_ITERATIONS, a
    sumulation_dt that needs more than CILQR_TRACKER_MAX_SIM_STEPS steps, a time grid that misses knots.  The handle keeps the
    configuration it had."""
    sc = _table_scene(lanes)
    B = sc["coarse"].shape[0]
    opt = _handle(50, B)
    default = opt.plan(sc, max_iter_trajs=4)
    opt.set_tracker_config(preview_time=0.5, weight_l=0.4, sumulation_dt=0.02, max_num_iteration=40)
    before = opt.plan(sc, max_iter_trajs=4)
    assert not np.array_equal(before["iter_trajs"][:, 0], default["iter_trajs"][:, 0])
    L = opt.L

    def rc_of(**over):
        c = api.TrackerConfig()
        L.cilqr_default_tracker_config(C.byref(c))
        for k, v in over.items():
            setattr(c, k, v)
        return L.cilqr_set_tracker_config(opt.h, C.byref(c))

    assert L.cilqr_set_tracker_config(opt.h, None) == api.ERR_ARG
    assert L.cilqr_set_tracker_config(None, None) == api.ERR_NULL
    for field, _ in api.TrackerConfig._fields_[:12]:
        for val in (float("nan"), float("inf"), -float("inf")):
            assert rc_of(**{field: val}) == api.ERR_ARG, (field, val)
    for cap in (api.TRACKER_MAX_ITERATIONS + 1, 10 ** 6, INT32_MAX, 0, -1):
        assert rc_of(max_num_iteration=cap) == api.ERR_ARG, cap
    assert rc_of(max_num_iteration=INT32_MAX, tolerance=0.0) == api.ERR_ARG
    smallest = 50 * 0.1 / api.TRACKER_MAX_SIM_STEPS
    for h in (smallest * 0.99, 1e-5, 1e-9, 1e-300, 5e-324, 0.0, -0.01):
        assert rc_of(sumulation_dt=h) == api.ERR_ARG, h
    for h in (0.03, 0.25, 0.07, 7.0):                      # the reference's "tacker failed": the clock misses knots
        assert rc_of(sumulation_dt=h) == api.ERR_ARG, h
    assert rc_of(tolerance=-1e-3) == api.ERR_ARG and rc_of(dt=0.0) == api.ERR_ARG
    with pytest.raises(api.CilqrError):
        opt.set_tracker_config(sumulation_dt=0.03)
    after = opt.plan(sc, max_iter_trajs=4)
    for k in ("traj", "cost_hist", "n_cost", "status", "n_iter", "iter_trajs"):
        assert np.array_equal(after[k], before[k]), k
    # what the limits admit is accepted (and replaced again before anything is launched)
    assert rc_of(max_num_iteration=api.TRACKER_MAX_ITERATIONS) == api.OK
    for h in (0.005, 0.02, 0.025, 0.05, 0.1):
        assert rc_of(sumulation_dt=h) == api.OK, h
    assert rc_of() == api.OK
    again = opt.plan(sc, max_iter_trajs=4)
    assert np.array_equal(again["iter_trajs"], default["iter_trajs"]) and np.array_equal(again["traj"], default["traj"])
    opt.close()
