"""cilqr_track_rows_batch (include/cilqr.h, "track"; kernels_track.hip) on the GPU: pinned to the init-guess kernel it shares
its steps with (bit for bit), held to the host call at STAGE_TOL, the equalities that need no tolerance (n_drive prefix,
layouts, HOST / DEVICE arrays, position in the batch, start6 = NULL), per-problem failure isolation, the argument checks and
the chain plan -> track -> audits -> warm start on rows that stay in device memory.

Tolerance: STAGE_TOL of tests/test_gpu_tracker.py with its measure (parity_util.traj_err).  A trajectory is left out of a
comparison only when the yardstick itself cannot decide it -- the host call's result moves by more than STAGE_TOL when the
start is scaled by 1 + 4e-16 -- at most MAX_EXCLUDED per comparison, each printed with its figures.

No test feeds non-finite or unbounded time axes to the GPU: the bound of the simulation loop is held on the host call
(tests/test_track.py) and by the finite 40 000-step case below.
"""
import ctypes as C

import numpy as np
import pytest

import track_cases as tk
import tracker_cases as tc
from cilqr_amd import api, scenario, scene_io
from parity_util import traj_err

pytestmark = pytest.mark.gpu
STAGE_TOL = 1e-9      # tests/test_gpu_tracker.py
MAX_EXCLUDED = 2
CMAX = 16

_HANDLES = {}


def _opt(tracker=None, vehicle=None, init_guess=api.INIT_IQR, capacity=1):
    """one handle per configuration for the whole module; batch and n_knots of a track call are not tied to it"""
    key = (tuple(sorted((tracker or {}).items())), tuple(sorted((vehicle or {}).items())), init_guess, capacity)
    if key not in _HANDLES:
        cfg = api.default_config(50, init_guess=init_guess, **(vehicle or {}))
        opt = api.BatchIlqrOptimizer(cfg, batch_capacity=capacity, cmax=CMAX, max_lane_segments=64)
        if tracker:
            opt.set_tracker_config(**tracker)
        _HANDLES[key] = opt
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for opt in _HANDLES.values():
        opt.close()
    _HANDLES.clear()


def _host_batch(rows, layout, start6, n_drive, tracker=None, vehicle=None):
    cfg, t = tk.configs(tracker, vehicle)
    out = [api.track_rows(cfg, t, rows[b], layout, None if start6 is None else start6[b], n_drive) for b in range(rows.shape[0])]
    return np.stack([d for d, _ in out]), np.array([ok for _, ok in out])


def _hold(got, ok, rows, layout, start6, n_drive, tracker, vehicle, what):
    """every problem of a batch against the host call at STAGE_TOL"""
    want, want_ok = _host_batch(rows, layout, start6, n_drive, tracker, vehicle)
    assert np.array_equal(ok != 0, want_ok), what
    worst, excluded = 0.0, []
    cfg, t = tk.configs(tracker, vehicle)
    for b in range(rows.shape[0]):
        e = traj_err(got[b], want[b])
        if e < STAGE_TOL:
            worst = max(worst, e)
            continue
        s6 = (rows[b, 0, [tk.COLS[layout][c] for c in range(6)]] if start6 is None else start6[b]) * (1.0 + 4e-16)
        moved = traj_err(api.track_rows(cfg, t, rows[b], layout, s6, n_drive)[0], want[b])
        assert moved > STAGE_TOL, (what, b, e, moved)      # the only evidence that excludes: the yardstick's own
        excluded.append((b, e, moved))
        print(f"{what}: problem {b} excluded: distance {e:.2e}, the host call itself moves by {moved:.2e} under 1 + 4e-16")
    print(f"{what}: {rows.shape[0]} problems, largest distance to the host call {worst:.2e}, excluded {len(excluded)}")
    assert len(excluded) <= MAX_EXCLUDED, (what, excluded)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------
# G1: pinned to k_init_guess_tracker
@pytest.mark.parametrize("with_station", [True, False], ids=["stations", "chord"])
def test_pinned_to_the_init_guess_kernel(with_station):
    B, K = 130, 51
    sc = scenario.generate("mix11", B, seed=5)
    opt = _opt(init_guess=api.INIT_TRACKER, capacity=B)
    coarse = sc["coarse"]
    station = None
    if with_station:   # arc-like stations that are not the chord length
        station = np.ascontiguousarray(np.stack([tk.chord(c) for c in coarse]) * 1.01 + 0.5)
        sc = dict(sc, coarse_station=station)
    opt.stage_load(sc)
    opt.stage_init_guess()
    X, U = opt.read(api.T_X), opt.read(api.T_U)
    assert X.shape == (B, K, 6) and U.shape == (B, K - 1, 2)
    times = np.array([opt.cfg.dt * i for i in range(K)])          # the bits of dt * i as the kernel forms them
    start6 = np.concatenate([sc["start"], np.zeros((B, 2))], axis=1)
    if with_station:
        rows = np.stack([tk.make_rows(api.ROWS_COARSE, times, coarse[b], station[b]) for b in range(B)])
        layout = api.ROWS_COARSE
    else:
        rows = np.stack([tk.make_rows(api.ROWS_TRAJ, times, coarse[b]) for b in range(B)])
        layout = api.ROWS_TRAJ
    driven, ok = opt.track(rows, layout, start6)
    assert ok.all()
    assert np.array_equal(_bits(driven[:, :, tk.STATE]), _bits(X))
    assert np.array_equal(_bits(driven[:, :-1, tk.CONTROLS]), _bits(U))
    assert np.all(driven[:, -1, tk.CONTROLS] == 0.0)


# ---------------------------------------------------------------------------------------------
# G2: the kernel against the host call
def test_crafted_table_against_the_host_call():
    groups = {}
    for c in tk.crafted():
        key = (c["layout"], c["rows"].shape[0], c["n_drive"], c["start6"] is not None, tuple(sorted(c["tracker"].items())),
               tuple(sorted(c["vehicle"].items())))
        groups.setdefault(key, []).append(c)
    for (layout, K, n_drive, has_start, _, _), cases in groups.items():
        pick = [cases[i % len(cases)] for i in range(65)]               # B padded to 65 by repeating cases
        rows = np.stack([c["rows"] for c in pick])
        start6 = np.stack([c["start6"] for c in pick]) if has_start else None
        tracker, vehicle = cases[0]["tracker"], cases[0]["vehicle"]
        driven, ok = _opt(tracker, vehicle).track(rows, layout, start6, n_drive)
        n = len(cases)
        _hold(driven[:n], ok[:n], rows[:n], layout, None if start6 is None else start6[:n], n_drive, tracker, vehicle,
              "crafted " + "/".join(c["name"] for c in cases[:3]))
        for i in range(n, 65):                                          # the repeats are the originals, bit for bit
            assert np.array_equal(_bits(driven[i]), _bits(driven[i % n]))


@pytest.mark.parametrize("name,tracker,vehicle", (("default", {}, {}),) + tk.CONFIGS, ids=lambda v: v if isinstance(v, str) else "")
def test_base_cases_against_the_host_call(name, tracker, vehicle):
    rows, start6 = tk.base_rows()
    driven, ok = _opt(tracker, vehicle).track(rows, api.ROWS_TRAJ, start6)
    _hold(driven, ok, rows, api.ROWS_TRAJ, start6, None, tracker, vehicle, "base " + name)


# ---------------------------------------------------------------------------------------------
# G3: equalities
def _mixed_batch(B, K=51, seed=9):
    """B distinct trajectories in CILQR_ROWS_COARSE with stations, times from 2.0, and six-state starts beside them"""
    rng = np.random.default_rng(seed)
    rows, starts = [], []
    for b in range(B):
        c, s = tc.path(K - 1, 0.1, rng.uniform(3.0, 9.0), rng.uniform(-0.08, 0.08), x0=rng.uniform(-5, 5), y0=rng.uniform(-5, 5),
                       th0=rng.uniform(-3, 3))
        c[:, 4], c[:, 5] = rng.uniform(-1, 1), rng.uniform(-0.2, 0.2)
        rows.append(tk.make_rows(api.ROWS_COARSE, 2.0 + tk.axis(K), c, s))
        starts.append(np.r_[tc._offset(c, rng.uniform(-1, 1), rng.uniform(-0.2, 0.2), v=c[0, 3] + rng.uniform(-1, 1)),
                            rng.uniform(-1, 1), rng.uniform(-0.1, 0.1)])
    return np.stack(rows), np.stack(starts)


def _as_layout(rows_coarse, layout, chord_station=False):
    out = []
    for r in rows_coarse:
        c = np.concatenate([r[:, 2:5], r[:, 6:9]], axis=1)
        out.append(tk.make_rows(layout, r[:, 0], c, tk.chord(c) if chord_station else r[:, 1]))
    return np.stack(out)


@pytest.mark.parametrize("B,K", [(1, 51), (63, 3), (64, 2), (65, 51), (130, 51)])
def test_equalities(B, K):
    import torch
    dev = torch.device("cuda", 0)
    opt = _opt()
    rows, start6 = _mixed_batch(B, K)
    full, ok = opt.track(rows, api.ROWS_COARSE, start6)
    assert ok.all() and full.shape == (B, K, 10)
    # ---- the n_drive prefix (the last row's controls belong to a step the shorter run does not take: zero)
    for nd in sorted({1, 2, min(6, K), K}):
        part, ok_p = opt.track(rows, api.ROWS_COARSE, start6, nd)
        assert ok_p.all() and part.shape == (B, nd, 10)
        assert np.array_equal(_bits(part[:, :nd - 1]), _bits(full[:, :nd - 1]))
        assert np.array_equal(_bits(part[:, nd - 1, :8]), _bits(full[:, nd - 1, :8]))
        assert np.all(part[:, nd - 1, tk.CONTROLS] == 0.0)
    # ---- layouts
    plan, _ = opt.track(_as_layout(rows, api.ROWS_PLAN), api.ROWS_PLAN, start6)
    assert np.array_equal(_bits(plan), _bits(full))
    traj, _ = opt.track(_as_layout(rows, api.ROWS_TRAJ), api.ROWS_TRAJ, start6)
    chord, _ = opt.track(_as_layout(rows, api.ROWS_COARSE, chord_station=True), api.ROWS_COARSE, start6)
    assert np.array_equal(_bits(traj), _bits(chord))
    # ---- HOST arrays = DEVICE arrays (rows one double into a larger block: nothing beyond a double's alignment is assumed)
    block = torch.zeros(rows.size + 1, dtype=torch.float64, device=dev)
    block[1:] = torch.from_numpy(rows.ravel()).to(dev)
    d_rows = block[1:].view(B, K, 9)
    d_start = torch.from_numpy(start6).to(dev)
    d_driven = torch.full((B * K * 10 + 2,), 77.0, dtype=torch.float64, device=dev)
    d_ok = torch.full((B + 2,), 77, dtype=torch.int32, device=dev)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rc, n_failed = opt.track_raw(B, api.ROWS_COARSE, d_rows.data_ptr(), K, d_start.data_ptr(), K, d_driven.data_ptr() + 8,
                                 d_ok.data_ptr() + 4, api.MEM_DEVICE)
    torch.cuda.synchronize()
    opt.set_stream(0)
    assert rc == api.OK and n_failed == 0
    got, got_ok = d_driven.cpu().numpy(), d_ok.cpu().numpy()
    assert got[0] == 77.0 and got[-1] == 77.0 and got_ok[0] == 77 and got_ok[-1] == 77     # nothing beside the outputs
    assert np.array_equal(_bits(got[1:-1].reshape(B, K, 10)), _bits(full)) and np.all(got_ok[1:-1] == 1)
    t_driven, t_ok = opt.track(d_rows.contiguous(), api.ROWS_COARSE, d_start)
    assert np.array_equal(_bits(t_driven.cpu().numpy()), _bits(full)) and t_ok.dtype == torch.int32
    # ---- start6 = NULL is the start gathered from row 0
    from_row0, _ = opt.track(rows, api.ROWS_COARSE, None)
    gathered, _ = opt.track(rows, api.ROWS_COARSE, np.ascontiguousarray(rows[:, 0, [2, 3, 4, 6, 7, 8]]))
    assert np.array_equal(_bits(from_row0), _bits(gathered))
    assert not np.array_equal(_bits(from_row0), _bits(full))


def test_a_problem_does_not_depend_on_its_batch():
    opt = _opt()
    rows, start6 = _mixed_batch(130)
    probe_rows, probe_start = _mixed_batch(1, seed=77)
    alone, ok = opt.track(probe_rows, api.ROWS_COARSE, probe_start)
    assert ok.all()
    for at in (0, 63, 64, 129):
        r, s = rows.copy(), start6.copy()
        r[at], s[at] = probe_rows[0], probe_start[0]
        driven, ok = opt.track(r, api.ROWS_COARSE, s)
        assert ok.all() and np.array_equal(_bits(driven[at]), _bits(alone[0])), at


# ---------------------------------------------------------------------------------------------
# G4: failures stay in their problem
def test_failures_are_isolated():
    opt = _opt(dict(sumulation_dt=0.01, max_num_iteration=1))
    rows, start6 = _mixed_batch(65, K=2, seed=12)
    good, ok = opt.track(rows, api.ROWS_COARSE, start6)
    assert ok.all()
    bad = rows.copy()
    bad[7, :, 0] = 0.0, 0.001        # the 10 ms clock ends before it has passed the second knot
    bad[40, :, 0] = 0.0, 400.0       # 40 000 steps: beyond CILQR_TRACKER_MAX_SIM_STEPS
    d_ok = np.zeros(65, np.int32)
    driven = np.full((65, 2, 10), 7.0)
    rc, n_failed = opt.track_raw(65, api.ROWS_COARSE, bad.ctypes.data, 2, start6.ctypes.data, 2, driven.ctypes.data,
                                 d_ok.ctypes.data, api.MEM_HOST)
    assert rc == api.OK and n_failed == 2
    others = np.ones(65, bool)
    others[[7, 40]] = False
    assert np.all(d_ok[others] == 1) and np.all(d_ok[~others] == 0)
    assert np.all(driven[~others] == 0.0)
    assert np.array_equal(_bits(driven[others]), _bits(good[others]))
    # the host call agrees about both
    cfg, t = tk.configs(dict(sumulation_dt=0.01, max_num_iteration=1))
    for b in (7, 40):
        d, ok_b = api.track_rows(cfg, t, bad[b], api.ROWS_COARSE, start6[b])
        assert not ok_b and np.all(d == 0.0)


# ---------------------------------------------------------------------------------------------
# G5: argument checks
def test_argument_checks():
    opt = _opt(capacity=8)
    L = api.lib()
    rows, start6 = _mixed_batch(4, K=3)
    driven, ok = np.zeros((4, 3, 10)), np.zeros(4, np.int32)
    n = C.c_int32(-1)

    def call(h=opt.h, B=4, layout=api.ROWS_COARSE, rows_=rows.ctypes.data, K=3, start=start6.ctypes.data, D=3, out=driven.ctypes.data,
             ok_=ok.ctypes.data, n_=C.byref(n), memory=api.MEM_HOST):
        return L.cilqr_track_rows_batch(h, B, layout, rows_, K, start, D, out, ok_, n_, memory)

    assert call() == api.OK and n.value == 0
    assert call(start=None) == api.OK and call(n_=None) == api.OK
    assert call(h=None) == api.ERR_NULL and call(rows_=None) == api.ERR_NULL
    assert call(out=None) == api.ERR_NULL and call(ok_=None) == api.ERR_NULL
    assert call(B=0) == api.ERR_ARG and call(B=-3) == api.ERR_ARG
    for layout in (-1, api.ROWS_CONTROLS, api.ROWS_POINTS, 7):
        assert call(layout=layout) == api.ERR_ARG
    assert call(K=1, D=1) == api.ERR_ARG
    assert call(D=0) == api.ERR_ARG and call(D=4) == api.ERR_ARG
    assert call(memory=2) == api.ERR_ARG and call(memory=-1) == api.ERR_ARG
    # ---- CILQR_ERR_STATE while a solve is submitted; the handle works after the wait
    sc = scenario.generate("mix11", 8, seed=3)
    ticket = opt.submit(sc)
    assert call() == api.ERR_STATE
    opt.collect(ticket)
    before = driven.copy()
    assert call() == api.OK
    assert np.array_equal(_bits(before), _bits(driven))


# ---------------------------------------------------------------------------------------------
# G6: the chain on rows that stay on the device
def test_chain_plan_track_audit_warm_start():
    import os
    import torch
    dev = torch.device("cuda", 0)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sf = scene_io.load(os.path.join(here, "scenes_mix11_4.cqs"))
    sc = scenario.generate("mix11", 4, seed=71, obstacle_points=True, scenarios=True)     # what the file was made from
    B, K = 4, sc["coarse"].shape[1]
    opt = _opt(capacity=4)
    M = opt.cfg.max_iter
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    dp_cfg, cor_cfg = api.default_dp_config(tf=opt.N * opt.cfg.dt, delta_t=opt.cfg.dt), api.default_corridor_config()
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    start = torch.from_numpy(np.ascontiguousarray(sc["start"])).to(dev)
    traj = torch.zeros((B, K, 10), dtype=torch.float64, device=dev)
    hist = torch.zeros((B, M + 1, 5), dtype=torch.float64, device=dev)
    plan = torch.zeros((B, K, api.PLAN_FIELDS), dtype=torch.float64, device=dev)
    n_cost, status, n_iter, outcome = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                            n_iter.data_ptr(), None, None, None)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    try:
        rc, _, _ = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb, start.data_ptr(), K, sol, plan.data_ptr(), None, outcome.data_ptr())
        assert rc == api.OK
        # ---- track the plan from a displaced start
        s6 = np.concatenate([sc["start"] + np.array([0.3, -0.4, 0.05, 0.5]), np.zeros((B, 2))], axis=1)
        d_s6 = torch.from_numpy(np.ascontiguousarray(s6)).to(dev)
        driven = torch.zeros((B, K, 10), dtype=torch.float64, device=dev)
        d_ok = torch.zeros(B, dtype=torch.int32, device=dev)
        rc, n_failed = opt.track_raw(B, api.ROWS_PLAN, plan.data_ptr(), K, d_s6.data_ptr(), K, driven.data_ptr(), d_ok.data_ptr(),
                                     api.MEM_DEVICE)
        assert rc == api.OK and n_failed == 0 and bool((d_ok == 1).all())
        # ---- the audits on the driven rows where they lie
        mask = torch.zeros((B, K), dtype=torch.uint8, device=dev)
        first, n_hit = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        rc, _ = opt.check_collisions_raw(dp_cfg, sb, api.ROWS_TRAJ, driven.data_ptr(), K, 0.0, mask.data_ptr(), first.data_ptr(),
                                         n_hit.data_ptr())
        assert rc == api.OK
        lowest, knot = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        rc, _ = opt.clearance_raw(dp_cfg, sb, api.ROWS_TRAJ, driven.data_ptr(), K, None, None, lowest.data_ptr(), knot.data_ptr(), 0.0)
        assert rc == api.OK
        prob, keep = api.margin_problem(sc, B, K)
        d_cor, d_cnt = torch.from_numpy(keep["corridor"]).to(dev), torch.from_numpy(keep["ccount"]).to(dev)
        prob.memory, prob.corridor, prob.corridor_count = api.MEM_DEVICE, d_cor.data_ptr(), d_cnt.data_ptr()
        mm, mk = torch.zeros((B, 8), dtype=torch.float64, device=dev), torch.zeros((B, 8), dtype=torch.int32, device=dev)
        violated = torch.zeros(B, dtype=torch.int32, device=dev)
        rc, _ = opt.constraint_margins_raw(prob, api.ROWS_TRAJ, driven.data_ptr(), None, None, mm.data_ptr(), mk.data_ptr(), None,
                                           violated.data_ptr())
        assert rc == api.OK
        # ---- a warm-started solve from the driven rows
        left, right = np.ascontiguousarray(sc["left"]), np.ascontiguousarray(sc["right"])
        d_coarse = torch.from_numpy(np.ascontiguousarray(sc["coarse"])).to(dev)
        problem = api.ProblemBatch(B, K, sc["cmax"], api.MEM_DEVICE, start.data_ptr(), d_coarse.data_ptr(), d_cor.data_ptr(),
                                   d_cnt.data_ptr(), left.shape[0], right.shape[0], left.ctypes.data, right.ctypes.data)
        it = torch.zeros((B, 1, K, 10), dtype=torch.float64, device=dev)
        n_it = torch.zeros(B, dtype=torch.int32, device=dev)
        sol2 = api.SolutionBatch(api.MEM_DEVICE, 1, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                                 n_iter.data_ptr(), it.data_ptr(), n_it.data_ptr(), None)
        warm, alive = api.make_warm((driven, None, api.ROWS_TRAJ))
        rc = opt.solve_raw(problem, sol2, warm)
        torch.cuda.synchronize()
        assert rc == api.OK
        h_driven, h_it = driven.cpu().numpy(), it.cpu().numpy()
        assert np.array_equal(_bits(h_it[:, 0, :-1, 8:10]), _bits(h_driven[:, :-1, 8:10]))
        assert np.abs(h_driven[:, :-1, 8:10]).max() > 0.0
    finally:
        opt.set_stream(0)
