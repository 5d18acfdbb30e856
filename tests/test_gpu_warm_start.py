"""Warm start on the GPU (cilqr_*_warm, include/cilqr.h; kernels_warm.hip): the first iterate against the NumPy statement of the
gather rule and the library's / the oracle's open-loop rollout, the fixed point of a re-solve, every step of warm solves
against the oracle, one result by every road into the library, hostile rows, the argument checks and the C++ adapter.

Scenes: scenario.generate("mix11", B, seed=3), N = 50, cmax 16.  The oracle of a warm-started solve is the oracle as it
stands: parity_util.check_steps replays every step from iter_trajs[0] onwards, whatever produced that iterate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import parity_util as pu
from cilqr_amd import api, scenario, warm
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, K = 50, 51
I32_MAX = 2 ** 31 - 1
ITER_CAP = 48
FIELDS = ("traj", "cost_hist", "n_cost", "status", "n_iter", "alpha_trace", "n_iter_trajs")
SHIFT_LIST = [-1, 0, 1, 7, N - 1, N, N + 1, I32_MAX]


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _take(sc, idx):
    """the listed problems of a scene dict (lane tables and sizes shared)"""
    B = sc["coarse"].shape[0]
    return {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.shape[:1] == (B,) and k not in ("left", "right") else v)
            for k, v in sc.items()}


def _sub(g, idx):
    """the listed problems of a result dict"""
    return {k: v[idx] for k, v in g.items() if isinstance(v, np.ndarray)}


def _tightened(sc, by=0.05):
    """every corridor plane moved inwards by `by` metres: c -= by * hypot(a, b)"""
    cor = sc["corridor"].copy()
    cor[..., 2] -= by * np.hypot(cor[..., 0], cor[..., 1])
    return dict(sc, corridor=cor)


def _assert_same_solution(g, ref, what, idx=None, cap=None):
    """every output of two solves, bit for bit (iterates: the ones both hold; idx: only these problems of g, against ref[idx])"""
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    for k in FIELDS:
        if ref.get(k) is None or g.get(k) is None:
            continue
        assert _same_bits(g[k], pick(ref[k])), (what, k)
    if g.get("iter_trajs") is not None and ref.get("iter_trajs") is not None:
        n = np.minimum(g["n_iter_trajs"], cap if cap is not None else g["iter_trajs"].shape[1])
        rit = pick(ref["iter_trajs"])
        for b in range(len(n)):
            assert _same_bits(g["iter_trajs"][b, :n[b]], rit[b, :n[b]]), (what, "iter_trajs", b)


# ---------------------------------------------------------------------------------------------
# device-resident problems and solutions (torch tensors), for the raw interface
# ---------------------------------------------------------------------------------------------
class _Dev:
    """a scene's per-problem arrays on the device + what a solve writes, as torch tensors"""

    def __init__(self, sc, cap=ITER_CAP, max_iter=200):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        self.sc = sc
        self.B = B = sc["coarse"].shape[0]
        self.t = {k: torch.from_numpy(np.ascontiguousarray(sc[k], dtype=(np.int32 if k == "ccount" else np.float64))).to(dev)
                  for k in ("start", "coarse", "corridor", "ccount")}
        self.left, self.right = np.ascontiguousarray(sc["left"], np.float64), np.ascontiguousarray(sc["right"], np.float64)
        M = max_iter
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.o = dict(traj=z((B, K, 10), torch.float64), cost_hist=z((B, M + 1, 5), torch.float64), n_cost=z(B, torch.int32),
                      status=z(B, torch.int32), n_iter=z(B, torch.int32), iter_trajs=z((B, cap, K, 10), torch.float64),
                      n_iter_trajs=z(B, torch.int32), alpha_trace=torch.full((B, M), -3, dtype=torch.int8, device=dev))
        self.cap = cap
        self.warm_keep = None
        torch.cuda.synchronize()

    def problem(self):
        t = self.t
        return api.ProblemBatch(self.B, K, self.sc["cmax"], api.MEM_DEVICE, t["start"].data_ptr(), t["coarse"].data_ptr(),
                                t["corridor"].data_ptr(), t["ccount"].data_ptr(), self.left.shape[0], self.right.shape[0],
                                self.left.ctypes.data, self.right.ctypes.data)

    def solution(self):
        o = self.o
        return api.SolutionBatch(api.MEM_DEVICE, self.cap, o["traj"].data_ptr(), o["cost_hist"].data_ptr(), o["n_cost"].data_ptr(),
                                 o["status"].data_ptr(), o["n_iter"].data_ptr(), o["iter_trajs"].data_ptr(),
                                 o["n_iter_trajs"].data_ptr(), o["alpha_trace"].data_ptr())

    def warm(self, rows, shift, layout):
        torch = self.torch
        dev = torch.device("cuda", 0)
        r = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).to(dev)
        s = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift, np.int32)).to(dev)
        torch.cuda.synchronize()
        w, keep = api.make_warm((r, s, layout))
        self.warm_keep = keep
        assert w.memory == api.MEM_DEVICE
        return w

    def result(self):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.o.items()}


def _host_warm_solve(opt, sc, warm_arg, cap=ITER_CAP):
    return opt.plan(sc, max_iter_trajs=cap, alpha_trace=True, warm=warm_arg)


# ---------------------------------------------------------------------------------------------
# 1. the first iterate
# ---------------------------------------------------------------------------------------------
_SCENE130 = {}
_OPTS = {}


def _scene130():
    if not _SCENE130:
        _SCENE130["sc"] = scenario.generate("mix11", 130, seed=3)
    return _SCENE130["sc"]


def _stage_opt(init):
    """one handle per init guess for all the cases of test 1 (closed with the module)"""
    if init not in _OPTS:
        cfg = api.default_config(N, init_guess=init)
        _OPTS[init] = api.BatchIlqrOptimizer(cfg, batch_capacity=130, cmax=16)
    return _OPTS[init]


@pytest.fixture(scope="module", autouse=True)
def _close_stage_opts():
    yield
    for o in _OPTS.values():
        o.close()
    _OPTS.clear()


def _random_rows(layout, B, rng):
    """finite rows with every column filled; the controls in the range test_open_loop_rollout uses (its tolerance is for them)"""
    stride, col = warm.CONTROL_COLUMNS[layout]
    rows = rng.normal(size=(B, warm.rows_per_problem(layout, N), stride)) * 3.0
    rows[:, :, col] = rng.uniform(-10, 10, rows.shape[:2])
    rows[:, :, col + 1] = rng.uniform(-0.23, 0.23, rows.shape[:2])
    return rows


@pytest.mark.parametrize("init", [api.INIT_IQR, api.INIT_TRACKER], ids=["iqr", "tracker"])
@pytest.mark.parametrize("memory", [api.MEM_HOST, api.MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("layout", [api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_CONTROLS], ids=["traj", "plan", "controls"])
@pytest.mark.parametrize("B", [130, 1, 64])
def test_first_iterate(B, layout, memory, init):
    """stage_load(warm) + stage_init_guess: U is the gather rule's, X the open-loop rollout from goals_[0]; the problems with
    shift -1 hold the configured init guess.  130 = two full wavefronts and a tail of two."""
    sc = _take(_scene130(), np.arange(B))
    rng = np.random.default_rng(100 * B + 10 * layout + memory)
    rows = _random_rows(layout, B, rng)
    opt = _stage_opt(init)
    # the cold first iterate of the same load
    opt.stage_load(sc)
    opt.stage_init_guess()
    Xc, Uc = opt.read(api.T_X), opt.read(api.T_U)
    x0 = np.concatenate([sc["start"], np.zeros((B, 2))], axis=1)          # goals_[0]: the start state with a = delta = 0
    o = orc.Oracle(n_steps=N)
    # the shift list repeated over the batch; a batch of one takes every entry in turn
    shifts = [np.resize(np.asarray(SHIFT_LIST, np.int32), B)] if B > 1 else [np.asarray([v], np.int32) for v in SHIFT_LIST]
    for shift in shifts:
        if memory == api.MEM_HOST:
            opt.stage_load(sc, warm=(rows, shift, layout))
        else:
            d = _Dev(sc, cap=1)
            assert opt.stage_load_raw(d.problem(), d.warm(rows, shift, layout)) == api.OK
        opt.stage_init_guess()
        X, U = opt.read(api.T_X), opt.read(api.T_U)
        want_u = warm.warm_controls(rows, shift, layout, N)
        hot = shift >= 0
        assert _same_bits(U[hot], want_u[hot])
        assert _same_bits(X[hot], opt.open_loop_rollout(x0, want_u)[hot])
        for b in np.nonzero(hot)[0]:
            assert pu.rel_err(X[b], o.open_loop_rollout(x0[b], want_u[b])) < 1e-11, b
        assert _same_bits(X[~hot], Xc[~hot]) and _same_bits(U[~hot], Uc[~hot])
        if hot.any():
            assert not _same_bits(X[hot], Xc[hot])                        # (the warm problems did change)
    # without a shift array every problem is warm-started with shift 0
    if memory == api.MEM_HOST:
        opt.stage_load(sc, warm=(rows, None, layout))
    else:
        d = _Dev(sc, cap=1)
        assert opt.stage_load_raw(d.problem(), d.warm(rows, None, layout)) == api.OK
    opt.stage_init_guess()
    U0 = opt.read(api.T_U)
    assert _same_bits(U0, warm.warm_controls(rows, None, layout, N))
    assert _same_bits(opt.read(api.T_X), opt.open_loop_rollout(x0, U0))
    # a plain load afterwards is cold again
    opt.stage_load(sc)
    opt.stage_init_guess()
    assert _same_bits(opt.read(api.T_X), Xc) and _same_bits(opt.read(api.T_U), Uc)


# ---------------------------------------------------------------------------------------------
# shared solves of tests 2, 4 and 5: 200 scenes, their cold solution
# ---------------------------------------------------------------------------------------------
_S200 = {}


def _solved200():
    if not _S200:
        sc = scenario.generate("mix11", 200, seed=3)
        opt = api.BatchIlqrOptimizer(api.default_config(N), batch_capacity=1300, cmax=16)
        cold = opt.plan(sc, max_iter_trajs=ITER_CAP, alpha_trace=True)
        _S200.update(sc=sc, opt=opt, cold=cold)
    return _S200["sc"], _S200["opt"], _S200["cold"]


@pytest.fixture(scope="module", autouse=True)
def _close_s200():
    yield
    if _S200:
        _S200["opt"].close()
        _S200.clear()


# ---------------------------------------------------------------------------------------------
# 2. fixed point
# ---------------------------------------------------------------------------------------------
def test_resolve_from_own_solution_starts_at_it():
    """The open-loop rollout of a returned trajectory's controls reproduces its states, and TotalCost of the pair its last
    Cost row (both bit for bit, in the oracle and here): a solve warm-started from its own result begins exactly there."""
    sc, opt, cold = _solved200()
    g = _host_warm_solve(opt, sc, (cold["traj"], None, api.ROWS_TRAJ))
    assert _same_bits(g["iter_trajs"][:, 0], cold["traj"])                    # all ten columns
    last = cold["cost_hist"][np.arange(200), cold["n_cost"] - 1]
    assert _same_bits(g["cost_hist"][:, 0], last)
    final = g["cost_hist"][np.arange(200), g["n_cost"] - 1, 0]
    assert np.all(final <= g["cost_hist"][:, 0, 0])                           # accepted steps need dcost > 0
    assert np.all((g["status"] >= 1) & (g["status"] <= 5))


# ---------------------------------------------------------------------------------------------
# 3. every step against the oracle
# ---------------------------------------------------------------------------------------------
def test_every_step_of_warm_solves_against_the_oracle():
    """The 5 cm-tightened variant of 64 scenes, warm from the untightened problems' cold solutions, with shift 0 and with
    shift 5 (on an unadvanced problem a poor guess: a source of long step chains)."""
    sc = scenario.generate("mix11", 64, seed=3)
    tight = _tightened(sc)
    opt = api.BatchIlqrOptimizer(api.default_config(N), batch_capacity=64, cmax=16)
    ocfg = pu.oracle_cfg_from(opt.cfg)
    base = opt.plan(sc)
    cold = opt.plan(tight)
    g0 = _host_warm_solve(opt, tight, (base["traj"], np.zeros(64, np.int32), api.ROWS_TRAJ))
    g5 = _host_warm_solve(opt, tight, (base["traj"], np.full(64, 5, np.int32), api.ROWS_TRAJ))
    opt.close()
    want = warm.warm_controls(base["traj"], np.full(64, 5, np.int32), api.ROWS_TRAJ, N)
    assert _same_bits(g5["iter_trajs"][:, 0, :N, 8:10], want)
    assert _same_bits(g0["iter_trajs"][:, 0, :N, 8:10], base["traj"][:, :N, 8:10])
    rep0 = pu.assert_steps(g0, tight, ocfg, what="warm, shift 0")
    rep5 = pu.assert_steps(g5, tight, ocfg, what="warm, shift 5")
    print(f"warm steps: shift 0 {rep0}; shift 5 {rep5}; n_iter cold {int(cold['n_iter'].sum())} "
          f"warm {int(g0['n_iter'].sum())} shifted {int(g5['n_iter'].sum())}")
    assert rep5["steps"] >= 3 * 64
    assert 2 * int(g0["n_iter"].sum()) <= int(cold["n_iter"].sum())


# ---------------------------------------------------------------------------------------------
# 4. one result by every road
# ---------------------------------------------------------------------------------------------
def _raw(handle, d, w):
    rc = handle.solve_raw(d.problem(), d.solution(), w)
    assert rc == api.OK, rc
    return d.result()


@pytest.mark.parametrize("B", [200, 1300])
def test_one_result_by_every_road(B):
    """1300 = the 200 scenes tiled, above the tail threshold of the synchronous call: lockstep iterations, re-packing and the
    hand-over to the finishing arena all see warm-started problems; the host arrays of such a batch travel array by array, and
    on a submitted solve through the transfer thread."""
    sc200, opt, cold200 = _solved200()
    idx = np.resize(np.arange(200), B)
    sc = _take(sc200, idx)
    cap = 4
    rows_a = np.ascontiguousarray(cold200["traj"][idx])
    shift_a = np.resize(np.asarray([0, -1, 3, 0, N + 1, 1, 0, -1, 0, 12, 0], np.int32), B)      # differing shifts, a quarter cold
    rows_b = rows_a.copy()
    rows_b[:, :, 8:10] *= 0.5                                                                     # another warm start altogether
    shift_b = np.resize(np.asarray([0, 0, -1, 2], np.int32), B)
    warm_a, warm_b = (rows_a, shift_a, api.ROWS_TRAJ), (rows_b, shift_b, api.ROWS_TRAJ)

    # the synchronous call on device arrays is the reference; plain solve for the cold problems
    da, db = _Dev(sc, cap), _Dev(sc, cap)
    ref_a = _raw(opt, da, da.warm(*warm_a))
    ref_b = _raw(opt, db, db.warm(*warm_b))
    plain = opt.plan(sc, max_iter_trajs=cap, alpha_trace=True)
    assert not _same_bits(ref_a["traj"], ref_b["traj"])
    cold_a = np.nonzero(shift_a < 0)[0]
    _assert_same_solution(_sub(ref_a, cold_a), plain, "shift < 0 in a mixed batch", idx=cold_a, cap=cap)
    hot = shift_a >= 0
    assert not _same_bits(ref_a["iter_trajs"][hot, 0], plain["iter_trajs"][hot, 0])

    # warm = NULL and an all-negative shift are the plain call
    dn = _Dev(sc, cap)
    _assert_same_solution(_raw(opt, dn, None), plain, "warm NULL", cap=cap)
    L = api.lib()
    assert L.cilqr_solve_batch_warm(opt.h, C.byref(dn.problem()), None, C.byref(dn.solution())) == api.OK
    _assert_same_solution(dn.result(), plain, "cilqr_solve_batch_warm(NULL)", cap=cap)
    _assert_same_solution(_raw(opt, dn, dn.warm(rows_a, np.full(B, -1, np.int32), api.ROWS_TRAJ)), plain, "all shifts negative", cap=cap)

    # HOST arrays, synchronous
    _assert_same_solution(_host_warm_solve(opt, sc, warm_a, cap), ref_a, "host arrays", cap=cap)
    _assert_same_solution(_host_warm_solve(opt, sc, warm_b, cap), ref_b, "host arrays (b)", cap=cap)
    # ... and the other layouts carry the same controls
    plan_rows = np.zeros((B, K, 11))
    plan_rows[:, :, 9:11] = rows_a[:, :, 8:10]
    _assert_same_solution(_host_warm_solve(opt, sc, (plan_rows, shift_a, api.ROWS_PLAN), cap), ref_a, "plan rows", cap=cap)
    ctl = np.ascontiguousarray(rows_a[:, :N, 8:10])
    _assert_same_solution(_host_warm_solve(opt, sc, (ctl, shift_a, api.ROWS_CONTROLS), cap), ref_a, "control rows", cap=cap)

    # two submitted solves in flight with different warm arrays: device arrays, then host arrays
    da2, db2 = _Dev(sc, cap), _Dev(sc, cap)
    assert opt.submit_raw(da2.problem(), da2.solution(), da2.warm(*warm_a)) == api.OK
    assert opt.submit_raw(db2.problem(), db2.solution(), db2.warm(*warm_b)) == api.OK
    assert opt.wait() == api.OK and opt.wait() == api.OK
    _assert_same_solution(da2.result(), ref_a, "submitted, device (a)", cap=cap)
    _assert_same_solution(db2.result(), ref_b, "submitted, device (b)", cap=cap)
    ta = opt.submit(sc, max_iter_trajs=cap, alpha_trace=True, warm=warm_a)
    tb = opt.submit(sc, max_iter_trajs=cap, alpha_trace=True, warm=warm_b)
    _assert_same_solution(opt.collect(ta), ref_a, "submitted, host (a)", cap=cap)
    _assert_same_solution(opt.collect(tb), ref_b, "submitted, host (b)", cap=cap)

    # a pool of two
    with api.HandlePool(api.default_config(N), handles=2, batch_capacity=B, cmax=16) as pool:
        tickets = [pool.submit(sc, max_iter_trajs=cap, alpha_trace=True, warm=w) for w in (warm_a, warm_b, warm_a)]
        for t, ref, what in zip(tickets, (ref_a, ref_b, ref_a), ("pool 0", "pool 1", "pool 2")):
            _assert_same_solution(pool.collect(t), ref, what, cap=cap)
        dp = _Dev(sc, cap)
        assert pool.submit_raw(dp.problem(), dp.solution(), dp.warm(*warm_b)) == api.OK
        assert pool.wait() == api.OK
        _assert_same_solution(dp.result(), ref_b, "pool, device arrays", cap=cap)

    # one process, device 0 listed twice: the warm arrays are cut into the shards
    with api.MultiDeviceOptimizer(api.default_config(N), devices=(0, 0), batch_capacity=B, cmax=16) as m:
        _assert_same_solution(m.plan(sc, max_iter_trajs=cap, alpha_trace=True, warm=warm_a), ref_a, "multi (a)", cap=cap)
        _assert_same_solution(m.plan(sc, max_iter_trajs=cap, alpha_trace=True, warm=warm_b), ref_b, "multi (b)", cap=cap)
        _assert_same_solution(m.plan(sc, max_iter_trajs=cap, alpha_trace=True), plain, "multi, plain", cap=cap)

    # 8 sampled problems as batches of one
    for b in np.random.default_rng(B).choice(B, 8, replace=False):
        one = _host_warm_solve(opt, _take(sc, [b]), (rows_a[[b]], shift_a[[b]], api.ROWS_TRAJ), cap)
        _assert_same_solution(one, ref_a, f"problem {b} alone", idx=[b], cap=cap)


def test_warm_start_with_lane_groups():
    """problems grouped by lane table are solved group by group: the warm arrays are sliced with them"""
    sc200, opt, cold = _solved200()
    sc = _take(sc200, np.arange(60))
    shift = np.resize(np.asarray([0, -1, 2], np.int32), 60)
    w = (np.ascontiguousarray(cold["traj"][:60]), shift, api.ROWS_TRAJ)
    ref = _host_warm_solve(opt, sc, w)
    nl, nr = len(sc["left"]), len(sc["right"])
    grouped = dict(sc, lane_groups=[(0, nl, nr), (23, nl, nr)], left=np.concatenate([sc["left"], sc["left"]]),
                   right=np.concatenate([sc["right"], sc["right"]]))
    _assert_same_solution(_host_warm_solve(opt, grouped, w), ref, "lane groups")


# ---------------------------------------------------------------------------------------------
# 5. hostile rows
# ---------------------------------------------------------------------------------------------
def test_hostile_rows_stay_inside_their_problems():
    sc, opt, cold = _solved200()
    rows = cold["traj"].copy()
    clean = _host_warm_solve(opt, sc, (rows, None, api.ROWS_TRAJ))
    bad = [17, 64, 199]                                    # mid-wave, first lane of a wave, last problem
    rows[17, 10, 9] = np.nan
    rows[64, 0, 8] = np.inf
    rows[199, 3, 8], rows[199, 30, 9] = -np.inf, np.nan
    g = _host_warm_solve(opt, sc, (rows, None, api.ROWS_TRAJ))
    others = np.setdiff1d(np.arange(200), bad)
    _assert_same_solution(_sub(g, others), clean, "beside hostile rows", idx=others)
    o = orc.Oracle(pu.oracle_cfg_from(opt.cfg))
    for b in bad:
        assert _same_bits(g["iter_trajs"][b, 0, :N, 8:10], rows[b, :N, 8:10])      # the bits went in as they were
        assert o.set_problem(sc["start"][b], sc["coarse"][b], sc["corridor"][b], sc["ccount"][b], sc["left"], sc["right"]) == 0
        X, U = g["iter_trajs"][b, 0, :, 1:7], g["iter_trajs"][b, 0, :N, 8:10]
        r = o.replay(np.ascontiguousarray(X), np.ascontiguousarray(U), 1.0, 1.0, 0)
        assert r["status"] != 0 and r["cost1"] is None, "the oracle accepted a step from a non-finite iterate"
        assert int(g["status"][b]) == r["status"], b
        assert int(g["n_iter"][b]) == r["n_iter"] == len(r["decisions"]), b
        assert np.array_equal(g["alpha_trace"][b, :r["n_iter"]], r["decisions"]), b
        assert int(g["n_cost"][b]) == 1 and int(g["n_iter_trajs"][b]) == 1, b


# ---------------------------------------------------------------------------------------------
# 6. argument checks
# ---------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_handle_usable():
    sc200, opt, cold = _solved200()
    sc = _take(sc200, np.arange(40))
    rows = np.ascontiguousarray(cold["traj"][:40])
    prob, keep = opt._host_problem(sc)
    sol, res = opt._plan_solution(40, 0, False)
    L = api.lib()
    good = api.WarmStart(api.MEM_HOST, api.ROWS_TRAJ, rows.ctypes.data, None)
    cases = [(api.WarmStart(api.MEM_HOST, api.ROWS_TRAJ, None, None), api.ERR_NULL),              # no rows
             (api.WarmStart(api.MEM_HOST, api.ROWS_COARSE, rows.ctypes.data, None), api.ERR_ARG),  # carries no controls
             (api.WarmStart(api.MEM_HOST, 4, rows.ctypes.data, None), api.ERR_ARG),                # unknown layouts
             (api.WarmStart(api.MEM_HOST, -1, rows.ctypes.data, None), api.ERR_ARG),
             (api.WarmStart(2, api.ROWS_TRAJ, rows.ctypes.data, None), api.ERR_ARG),               # no such memory
             (api.WarmStart(api.MEM_DEVICE, api.ROWS_TRAJ, rows.ctypes.data, None), api.ERR_ARG)]  # not the problem's memory
    pool = api.HandlePool(api.default_config(N), handles=1, batch_capacity=40, cmax=16)
    multi = api.MultiDeviceOptimizer(api.default_config(N), devices=(0, 0), batch_capacity=40, cmax=16)
    for w, code in cases:
        assert L.cilqr_solve_batch_warm(opt.h, C.byref(prob), C.byref(w), C.byref(sol)) == code
        assert L.cilqr_submit_warm(opt.h, C.byref(prob), C.byref(w), C.byref(sol)) == code
        assert opt.wait() == api.ERR_STATE                                                         # nothing was accepted
        assert L.cilqr_stage_load_warm(opt.h, C.byref(prob), C.byref(w)) == code
        assert L.cilqr_pool_submit_warm(pool.h, C.byref(prob), C.byref(w), C.byref(sol)) == code
        assert pool.wait() == api.ERR_STATE
        assert L.cilqr_multi_solve_warm(multi.h, C.byref(prob), C.byref(w), C.byref(sol)) == code
    assert L.cilqr_solve_batch_warm(opt.h, None, C.byref(good), C.byref(sol)) == api.ERR_NULL
    assert L.cilqr_solve_batch_warm(opt.h, C.byref(prob), C.byref(good), None) == api.ERR_NULL
    # a good call on the same handles
    ref = _host_warm_solve(opt, sc, (rows, None, api.ROWS_TRAJ), cap=2)
    assert _same_bits(ref["iter_trajs"][:, 0], rows)
    assert L.cilqr_solve_batch_warm(opt.h, C.byref(prob), C.byref(good), C.byref(sol)) == api.OK
    _assert_same_solution(dict(res), ref, "after the rejected calls")
    _assert_same_solution(pool.collect(pool.submit(sc, max_iter_trajs=2, alpha_trace=True, warm=(rows, None))), ref, "pool after", cap=2)
    _assert_same_solution(multi.plan(sc, max_iter_trajs=2, alpha_trace=True, warm=(rows, None)), ref, "multi after", cap=2)
    opt.stage_load(sc, warm=(rows, None))
    opt.stage_init_guess()
    assert _same_bits(opt.read(api.T_U), rows[:, :N, 8:10])
    pool.close()
    multi.close()
    del keep


# ---------------------------------------------------------------------------------------------
# 7. the C++ adapter
# ---------------------------------------------------------------------------------------------
def test_cpp_adapter_warm_start(tmp_path):
    """IlqrOptimizer::WarmStart(previous): the next Plan starts from `previous`, the one after it is cold again."""
    from test_host import build_cpp_test
    exe = build_cpp_test("warm_start_test", tmp_path, "stand-ins")
    g = np.load(os.path.join(HERE, "golden", "mix11_n50.npz"))
    b = 1
    Kg, cmax = g["coarse"].shape[1], int(g["cmax"])
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as f:
        np.array([Kg, cmax, g["left"].shape[0], g["right"].shape[0]], np.int32).tofile(f)
        for a in (g["start"][b], g["coarse"][b]):
            np.ascontiguousarray(a, np.float64).tofile(f)
        np.ascontiguousarray(g["ccount"][b], np.int32).tofile(f)
        for a in (g["corridor"][b], g["left"], g["right"]):
            np.ascontiguousarray(a, np.float64).tofile(f)
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(scene), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, np.uint8)
    ok, n1, n2, n3 = np.frombuffer(raw[:16].tobytes(), np.int32)
    assert ok == 1
    first, second_it0, second, third, first_it0, third_it0 = np.frombuffer(raw[16:].tobytes(), np.float64).reshape(6, Kg, 10)
    assert n1 >= 1 and n2 >= 1 and second.shape == first.shape
    assert _same_bits(second_it0, first)                   # the warm Plan's first iterate is the first Plan's result
    assert _same_bits(third, first) and n3 == n1           # armed for one Plan only: the third equals the first
    assert _same_bits(third_it0, first_it0) and not _same_bits(first_it0, first)
