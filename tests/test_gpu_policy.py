"""cilqr_policy_gains_batch and cilqr_policy_rollout_batch (include/cilqr.h, "policy"; kernels_policy.hip) on the GPU.

  gains    = the stage chain load -> set_trajectory -> quadratize -> backward -> read, as int64 views
  rollout  = k_forward (cilqr_stage_forward) bit for bit from goals[0], at horizons 1, 2, 5, 50 and on the crafted table's
             unwrapped headings; a solver's own trajectory is a fixed point; perturbed starts against the oracle's Forward and
             the long-double statement at STAGE_TOL; a chain's bits do not depend on its batch, its samples or its neighbours;
             clamp, n_out and the optional outputs against cilqr_amd/policy.py; HOST = DEVICE arrays; every refusal.
Batches of 1, 63, 65, 130 and samples of 1, 3, 8, 65, 256 straddle a wavefront, the 64-lane and the 256-lane workgroup."""
import numpy as np
import pytest

import policy_cases as pc
import riccati_cases as rc
import riccati_reference as rr
import stage_cases as sc
from parity_util import oracle_cfg_from
from cilqr_amd import api, policy, scenario
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
STAGE_TOL = rc.STAGE_TOL
bits = pc.bits
ALPHAS = (1.0, 0.5012, 0.0010, 0.0)


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _first(scene, B):
    n = scene["coarse"].shape[0]
    return {k: (np.ascontiguousarray(v[:B]) if isinstance(v, np.ndarray) and v.shape[:1] == (n,) and k not in ("left", "right") else v)
            for k, v in scene.items()}


@pytest.fixture(scope="module")
def solved():
    """130 mix11 scenes of the generator's horizon, solved once: (scene, traj [130, 51, 10], handle of capacity 130)"""
    scene = scenario.generate("mix11", 130, seed=pc.REF_SEED)
    opt = api.BatchIlqrOptimizer(n_steps=scene["n_steps"], batch_capacity=130, cmax=scene["cmax"])
    g = opt.plan(scene)
    yield scene, np.ascontiguousarray(g["traj"]), opt
    opt.close()


@pytest.fixture(scope="module")
def gains(solved):
    """gains of the solved trajectories at lambda = 1 (pc.REF_LAMBDA): dict(Kfb, kff, dV, ok)"""
    scene, traj, opt = solved
    return opt.policy_gains(scene, traj, api.ROWS_TRAJ, lam=pc.REF_LAMBDA)


def _plan_rows(traj):
    """the same trajectories in CILQR_ROWS_PLAN, NaN in the columns the policy calls do not read"""
    return pc.rows_of(traj[:, :, 1:7], traj[:, :-1, 8:10], api.ROWS_PLAN)


# ---------------------------------------------------------------------------------------------
# 1. gains = stage chain
def _chain(opt, scene, X, U, lam):
    opt.stage_load(scene)
    opt.stage_set_trajectory(X, U)
    opt.stage_quadratize()
    opt.stage_backward(lam)
    return opt.read(api.T_KFB), opt.read(api.T_KFF), opt.read(api.T_DV)


@pytest.mark.parametrize("B", [1, 65, 130])
def test_gains_are_the_stage_chain(solved, B):
    scene, traj, opt = solved
    sub = _first(scene, B)
    X, U = np.ascontiguousarray(traj[:B, :, 1:7]), np.ascontiguousarray(traj[:B, :-1, 8:10])
    mix = np.array([rc.HORIZON_LAMBDAS[b % len(rc.HORIZON_LAMBDAS)] for b in range(B)])
    for lam in (None, 1.0, mix):
        want = _chain(opt, sub, X, U, lam)
        for layout in (api.ROWS_TRAJ, api.ROWS_PLAN):
            got = opt.policy_gains(sub, pc.rows_of(X, U, layout), layout, lam=lam)
            for name, w in zip(("Kfb", "kff", "dV"), want):
                assert np.array_equal(bits(got[name]), bits(w)), (B, layout, name, lam is None)
            assert np.all(got["ok"] == 1)
            # the handle is in the chain's staged state
            assert np.array_equal(bits(opt.read(api.T_KFB)), bits(want[0]))
            assert np.array_equal(bits(opt.read(api.T_X)), bits(X))


def test_gains_at_a_short_horizon():
    scene = rc.horizon_scene("mix11", 5, 9, seed=rc.HORIZON_SEED + 1050)
    opt = api.BatchIlqrOptimizer(api.default_config(5), batch_capacity=16, cmax=scene["cmax"])
    opt.stage_load(scene)
    opt.stage_init_guess()
    X, U = opt.read(api.T_X), opt.read(api.T_U)
    want = _chain(opt, scene, X, U, 1.0)
    got = opt.policy_gains(scene, pc.rows_of(X, U, api.ROWS_PLAN), api.ROWS_PLAN, lam=1.0)
    for name, w in zip(("Kfb", "kff", "dV"), want):
        assert np.array_equal(bits(got[name]), bits(w)), name
    opt.close()


def test_gains_of_a_problem_without_corridor(solved):
    """one negative corridor_count: ok = 0 and zeros for that problem; a NaN row poisons its own problem; the neighbours of both
    keep the bits of the clean call"""
    scene, traj, opt = solved
    B, dead, nan = 65, 7, 40
    sub = _first(scene, B)
    clean = opt.policy_gains(sub, traj[:B], api.ROWS_TRAJ, lam=1.0)
    sub["ccount"] = sub["ccount"].copy()
    sub["ccount"][dead, 11] = -1
    rows = traj[:B].copy()
    rows[nan, 20, 1] = np.nan
    got = opt.policy_gains(sub, rows, api.ROWS_TRAJ, lam=1.0)
    others = np.ones(B, bool)
    others[[dead, nan]] = False
    assert got["ok"][dead] == 0 and np.all(got["ok"][others] == 1) and got["ok"][nan] == 1
    for name in ("Kfb", "kff", "dV"):
        assert np.all(bits(got[name][dead]) == 0), name
        assert np.array_equal(bits(got[name][others]), bits(clean[name][others])), name
    assert not np.isfinite(got["Kfb"][nan]).all()


def test_gains_refusals(solved):
    scene, traj, opt = solved
    B = 8
    sub = _first(scene, B)
    rows = np.ascontiguousarray(traj[:B])
    nl, nr = scene["left"].shape[0], scene["right"].shape[0]
    grouped = dict(sub, left=np.concatenate([scene["left"]] * 2), right=np.concatenate([scene["right"]] * 2),
                   lane_groups=[(0, nl, nr), (3, nl, nr)])
    prob, keep = opt._host_problem(sub)
    out = dict(K=np.zeros((B, opt.N, 2, 6)), k=np.zeros((B, opt.N, 2)))
    call = lambda p, layout, r=rows, K=out["K"], k=out["k"]: opt.policy_gains_raw(p, layout, api._ptr(r), None, api._ptr(K), api._ptr(k))  # noqa: E731
    good = lambda: opt.policy_gains(sub, rows, api.ROWS_TRAJ)   # noqa: E731
    gprob, gkeep = opt._host_problem(grouped)
    assert call(gprob, api.ROWS_TRAJ) == api.ERR_ARG             # two lane groups
    good()
    for layout in (api.ROWS_COARSE, api.ROWS_CONTROLS, api.ROWS_POINTS, 9, -1):
        assert call(prob, layout) == api.ERR_ARG, layout
    good()
    assert call(None, api.ROWS_TRAJ) == api.ERR_NULL
    assert call(prob, api.ROWS_TRAJ, r=None) == api.ERR_NULL and call(prob, api.ROWS_TRAJ, K=None) == api.ERR_NULL
    assert call(prob, api.ROWS_TRAJ, k=None) == api.ERR_NULL
    short, skeep = opt._host_problem(dict(sub, coarse=sub["coarse"][:, :-1], corridor=sub["corridor"][:, :-1], ccount=sub["ccount"][:, :-1]))
    assert call(short, api.ROWS_TRAJ) == api.ERR_KNOTS
    good()
    # while a solve is submitted
    ticket = opt.submit(sub)
    assert call(prob, api.ROWS_TRAJ) == api.ERR_STATE
    opt.collect(ticket)
    assert call(prob, api.ROWS_TRAJ) == api.OK


# ---------------------------------------------------------------------------------------------
# 2. rollout = k_forward
def _hold_k_forward(opt, X, U, what):
    """after cilqr_stage_quadratize: for lambda 0 and 1, every alpha -- out_rows against XCAND / UCAND of cilqr_stage_forward"""
    B, K = X.shape[:2]
    N = K - 1
    goals = opt.read(api.T_GOALS)
    start = np.ascontiguousarray(goals[None, :, 0])
    dt, wb = opt.cfg.dt, opt.cfg.wheel_base
    for lam in rc.FORWARD_LAMBDAS:
        opt.stage_backward(np.full(B, lam))
        Kfb, kff = opt.read(api.T_KFB), opt.read(api.T_KFF)
        for layout in (api.ROWS_TRAJ, api.ROWS_PLAN):
            rows = pc.rows_of(X, U, layout)
            for alpha in ALPHAS:
                opt.stage_forward(alpha)
                Xc, Uc = opt.read(api.T_XCAND), opt.read(api.T_UCAND)
                got = opt.policy_rollout(rows, layout, Kfb, start, kff=kff, alpha=alpha)
                r = got["rows"][0]
                assert np.array_equal(bits(r[:, :, 1:7]), bits(Xc)), (what, lam, layout, alpha, "states")
                assert np.array_equal(bits(r[:, :N, 8:10]), bits(Uc)), (what, lam, layout, alpha, "controls")
                assert np.all(bits(r[:, N, 8:10]) == 0), (what, "last row's controls")
                assert np.array_equal(r[:, :, 0], np.broadcast_to(np.arange(K) * dt, (B, K))), (what, "time")
                kappa = np.tan(Xc[:, :, 5]) / wb       # write_traj_point's expression; the device's tan is within 2 ulp of libm's
                ok = np.isfinite(kappa)
                assert np.all(np.abs(r[:, :, 7] - kappa)[ok] <= 4e-16 * np.abs(kappa[ok])), (what, "kappa")
                assert np.all(got["n_clamped"] == 0)


@pytest.mark.parametrize("n_steps,B", [(1, 65), (2, 9), (5, 65), (50, 63)])
def test_rollout_is_k_forward(n_steps, B):
    scene = rc.horizon_scene("mix11", n_steps, B, seed=rc.HORIZON_SEED + 1000 + 10 * n_steps + (4 if n_steps == 50 else 0))
    opt = api.BatchIlqrOptimizer(api.default_config(n_steps), batch_capacity=80, cmax=scene["cmax"])
    opt.stage_load(scene)
    opt.stage_init_guess()
    X, U = opt.read(api.T_X), opt.read(api.T_U)
    opt.stage_quadratize()
    _hold_k_forward(opt, X, U, f"mix11 N {n_steps} B {B}")
    opt.close()


def test_rollout_is_k_forward_on_unwrapped_headings():
    """the crafted table of tests/stage_cases.py: nominal headings of 3, 7, 40 and -25 rad, so the rare path of the wraps runs"""
    g = sc.evaluate("default", True, 1)[sc.MAIN_CMAX]
    B = g["X"].shape[0]
    assert np.abs(g["X"][:, :, 2]).max() > 9.4      # beyond the short paths of NormalizeAngle
    opt = api.BatchIlqrOptimizer(api.default_config(sc.N_STEPS, **sc.CONFIGS["default"]), batch_capacity=B, cmax=sc.MAIN_CMAX)
    opt.set_option(api.OPT_EXACT_LANE_TIES, 1)
    opt.stage_load(g["scene"])
    opt.stage_set_trajectory(g["X"], g["U"])
    opt.stage_quadratize()
    _hold_k_forward(opt, g["X"], g["U"], "table default")
    opt.close()


# ---------------------------------------------------------------------------------------------
# 3. fixed point
@pytest.mark.parametrize("S,B", [(1, 130), (3, 65), (256, 9)])
def test_a_solvers_trajectory_is_a_fixed_point(solved, gains, S, B):
    """from its own start under the feedback alone: every sample's rows are the nominal rows' state and control columns bit for
    bit -- time and kappa too, which are write_traj_point's own (the nominal IS its output) -- and max_dev == 0"""
    scene, traj, opt = solved
    traj = np.ascontiguousarray(traj[-B:])
    start = np.ascontiguousarray(np.broadcast_to(traj[None, :, 0, 1:7], (S, B, 6)))
    got = opt.policy_rollout(traj, api.ROWS_TRAJ, gains["Kfb"][-B:], start)
    for s in range(S):
        assert np.array_equal(bits(got["rows"][s]), bits(traj)), s
    assert np.all(bits(got["max_dev"]) == 0) and np.all(bits(got["end_dev"]) == 0) and np.all(got["n_clamped"] == 0)


# ---------------------------------------------------------------------------------------------
# 4. perturbed starts against the references
def test_perturbed_starts_against_the_oracle_and_the_statement(solved, gains):
    """The first pc.REF_B solved mix11 scenes whose nominal trajectory is tame itself, gains at lambda = 1, the eight offsets of tests/policy_cases.py, alpha 1 and 0.
      (a) offsets of x, y, theta, v: the oracle's Forward, its problem set with the perturbed start, fed the device's gains
          and the nominal X, U -- STAGE_TOL where rc.tame holds;
      (b) all eight offsets (a and delta too): rr.forward with that x0 -- STAGE_TOL on tame rollouts.
    Rollouts that are not tame are excluded, at most rc.wild_cap of them.  Counted on the CPU with oracle-side gains
    (Oracle.backward at lambda 1 on the oracle's quadratisation of its own solve, no kernel involved), same scenes and offsets:
    scenes 0 and 25 are skipped (their own plan steers beyond 0.7 rad); 4 of the 256 rollouts of (a) and 8 of the 512 of (b)
    are not tame -- all of scene 22 at alpha = 1, a plan that steers to 0.44 rad and whose last feed-forward step is large --
    against caps of 7 and 15; on the tame rollouts of (a) the oracle (double) and the statement (long double) part by at most
    3.6e-12, none beyond STAGE_TOL / 4."""
    scene, traj, opt = solved
    B, K = pc.REF_B, traj.shape[1]
    N = K - 1
    off = pc.offsets()
    S = off.shape[0]
    idx = pc.reference_scenes(traj[:, :, 1:7])
    scene = {k: (v[idx] if k in ("start", "coarse", "corridor", "ccount") else v) for k, v in scene.items()}
    nominal = np.ascontiguousarray(traj[idx])
    X, U = nominal[:, :, 1:7], nominal[:, :-1, 8:10]
    Kfb, kff = np.ascontiguousarray(gains["Kfb"][idx]), np.ascontiguousarray(gains["kff"][idx])
    start = X[None, :, 0] + off[:, None, :]
    ocfg = oracle_cfg_from(opt.cfg)
    worst = dict(oracle=0.0, statement=0.0)
    total = dict(oracle=0, statement=0)
    wild = dict(oracle=0, statement=0)
    for alpha in pc.REF_ALPHAS:
        got = opt.policy_rollout(nominal, api.ROWS_TRAJ, Kfb, start, kff=kff, alpha=alpha)["rows"]
        for s in range(S):
            sX, sU = rr.forward(alpha, start[s], X, U, Kfb, kff, ocfg)
            for b in range(B):
                mine = (got[s, b, :, 1:7], got[s, b, :N, 8:10])
                total["statement"] += 1
                if rc.tame(sX[b]):
                    d = rc.forward_distance(mine, (sX[b], sU[b]))
                    worst["statement"] = max(worst["statement"], d)
                    assert d < STAGE_TOL, ("statement", alpha, s, b, d)
                else:
                    wild["statement"] += 1
                if np.all(off[s, 4:] == 0):
                    o = orc.Oracle(ocfg)
                    assert o.set_problem(scene["start"][b] + off[s, :4], scene["coarse"][b], scene["corridor"][b], scene["ccount"][b],
                                         scene["left"], scene["right"]) == 0
                    oX, oU = o.forward(alpha, X[b], U[b], Kfb[b], kff[b])
                    total["oracle"] += 1
                    if rc.tame(oX):
                        d = rc.forward_distance(mine, (oX, oU))
                        worst["oracle"] = max(worst["oracle"], d)
                        assert d < STAGE_TOL, ("oracle", alpha, s, b, d)
                    else:
                        wild["oracle"] += 1
    print(f"perturbed starts: kernel vs oracle {worst['oracle']:.2e} ({wild['oracle']} of {total['oracle']} not tame), "
          f"kernel vs statement {worst['statement']:.2e} ({wild['statement']} of {total['statement']} not tame)")
    for k in total:
        assert wild[k] <= rc.wild_cap(N, total[k]), (k, wild[k], total[k])


# ---------------------------------------------------------------------------------------------
# 5. independence
def test_a_chain_does_not_depend_on_its_batch_or_samples(solved, gains):
    scene, traj, opt = solved
    off = pc.offsets()
    b, o = 37, 6
    rows1, K1 = np.ascontiguousarray(traj[b:b + 1]), np.ascontiguousarray(gains["Kfb"][b:b + 1])
    k1 = np.ascontiguousarray(gains["kff"][b:b + 1])
    x0 = traj[b, 0, 1:7] + off[o]
    alone = opt.policy_rollout(rows1, api.ROWS_TRAJ, K1, x0[None, None], kff=k1, alpha=0.5012, clamp=True)
    names = ("rows", "max_dev", "end_dev")

    def same(got, s, p, what):
        for n in names:
            assert np.array_equal(bits(got[n][s, p]), bits(alone[n][0, 0])), (what, n)
        assert got["n_clamped"][s, p] == alone["n_clamped"][0, 0], what
    # the same problem at several places of a batch of 130 (among other neighbours), the same start at several samples of 8
    for place in (0, 63, 64, 129):
        order = np.arange(130)
        order[[place, b]] = order[[b, place]]
        rows, Kfb, kff = traj[order], gains["Kfb"][order], gains["kff"][order]
        start = rows[None, :, 0, 1:7] + off[:, None, :]                    # [8, 130, 6]
        for smp in (0, 5, 7):
            st = start.copy()
            st[[smp, o]] = st[[o, smp]]
            got = opt.policy_rollout(rows, api.ROWS_TRAJ, Kfb, st, kff=kff, alpha=0.5012, clamp=True)
            same(got, smp, place, (place, smp))
    # ... and among 256 samples of a batch of 3 (one workgroup per problem)
    sel = [b - 1, b, b + 1]
    st = traj[None, sel, 0, 1:7] + np.resize(off, (256, 6))[:, None, :] * np.linspace(-1, 1, 256)[:, None, None]
    st[200, 1] = x0
    got = opt.policy_rollout(traj[sel], api.ROWS_TRAJ, gains["Kfb"][sel], st, kff=gains["kff"][sel], alpha=0.5012, clamp=True)
    same(got, 200, 1, "S = 256")
    # a non-finite start in one sample leaves every other chain as it was
    st2 = st.copy()
    st2[17, 1, 2] = np.nan
    st2[64, 0, 0] = np.inf
    got2 = opt.policy_rollout(traj[sel], api.ROWS_TRAJ, gains["Kfb"][sel], st2, kff=gains["kff"][sel], alpha=0.5012, clamp=True)
    keep = np.ones((256, 3), bool)
    keep[17, 1] = keep[64, 0] = False
    for n in names + ("n_clamped",):
        a, c = got[n][keep], got2[n][keep]
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, c.view(np.int64) if c.dtype == np.float64 else c), n
    assert np.isnan(got2["max_dev"][17, 1]) and not np.isfinite(got2["rows"][64, 0]).all()


def test_sample_slices_are_ordinary_batches():
    """out_rows stays on the device; slice s of it, where it lies, gives check_collisions and constraint_margins the bits the
    same rows give when copied out into a batch of their own"""
    import os
    import torch
    from cilqr_amd import scene_io
    dev = torch.device("cuda", 0)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sf = scene_io.load(os.path.join(here, "scenes_mix11_4.cqs"))
    scn = scenario.generate("mix11", 4, seed=71, obstacle_points=True, scenarios=True)      # what the file was made from
    B, K, S = 4, scn["coarse"].shape[1], 3
    opt = api.BatchIlqrOptimizer(n_steps=scn["n_steps"], batch_capacity=B, cmax=scn["cmax"])
    traj = np.ascontiguousarray(opt.plan(scn)["traj"])
    g = opt.policy_gains(scn, traj, api.ROWS_TRAJ, lam=1.0)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    dp_cfg = api.default_dp_config(tf=opt.N * opt.cfg.dt, delta_t=opt.cfg.dt)
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    start = traj[None, :, 0, 1:7] + pc.offsets()[[0, 3, 7]][:, None, :]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    try:
        got = opt.policy_rollout(to(traj), api.ROWS_TRAJ, to(g["Kfb"]), to(start))
        rows = got["rows"]
        assert tuple(rows.shape) == (S, B, K, 10)
        prob, keep = api.margin_problem(scn, B, K)
        d_cor, d_cnt = to(keep["corridor"]), to(keep["ccount"])
        prob.memory, prob.corridor, prob.corridor_count = api.MEM_DEVICE, d_cor.data_ptr(), d_cnt.data_ptr()

        def audits(ptr):
            mask = torch.zeros((B, K), dtype=torch.uint8, device=dev)
            first, n_hit = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            rc_, _ = opt.check_collisions_raw(dp_cfg, sb, api.ROWS_TRAJ, ptr, K, 0.0, mask.data_ptr(), first.data_ptr(), n_hit.data_ptr())
            assert rc_ == api.OK
            mm, mk = torch.zeros((B, 8), dtype=torch.float64, device=dev), torch.zeros((B, 8), dtype=torch.int32, device=dev)
            violated = torch.zeros(B, dtype=torch.int32, device=dev)
            rc_, _ = opt.constraint_margins_raw(prob, api.ROWS_TRAJ, ptr, None, None, mm.data_ptr(), mk.data_ptr(), None,
                                                violated.data_ptr())
            assert rc_ == api.OK
            torch.cuda.synchronize()
            return [v.cpu().numpy() for v in (mask, first, mm, mk, violated)]
        for s in range(S):
            where_it_lies = audits(rows.data_ptr() + s * B * K * 10 * 8)
            own = rows[s].clone()
            copied = audits(own.data_ptr())
            for a, c in zip(where_it_lies, copied):
                assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, c.view(np.int64) if c.dtype == np.float64 else c), s
        host = opt.policy_rollout(traj, api.ROWS_TRAJ, g["Kfb"], start)
        assert np.array_equal(bits(rows.cpu().numpy()), bits(host["rows"]))
    finally:
        opt.set_stream(0)
        opt.close()


# ---------------------------------------------------------------------------------------------
# 6. clamp, n_out, optional outputs
def _recorded_step(rows):
    """the device's own rows as the dynamics: step i of chain (s, b) leads where the device went"""
    return lambda i, x, u: rows[:, :, i + 1, 1:7]


@pytest.mark.parametrize("B,S", [(63, 8), (130, 3)])
def test_clamp_against_the_statement(solved, gains, B, S):
    """starts 3 to 6 m and 0.3 rad off, alpha = 1: controls and n_clamped of cilqr_amd/policy.py, fed the device's states,
    are the device's, exactly; both bounds of both controls are met"""
    scene, traj, opt = solved
    cfg = opt.cfg
    r = np.random.default_rng(5)
    far = np.array([6.0, 3.0, 0.3, 2.0, 0.5, 0.05])
    start = traj[None, :B, 0, 1:7] + r.uniform(-1, 1, (S, B, 6)) * far
    got = opt.policy_rollout(traj[:B], api.ROWS_TRAJ, gains["Kfb"][:B], start, kff=gains["kff"][:B], alpha=1.0, clamp=True)
    bounds = (cfg.jerk_min, cfg.jerk_max, cfg.delta_rate_min, cfg.delta_rate_max)
    want = policy.rollout(traj[:B], api.ROWS_TRAJ, gains["Kfb"][:B], start, _recorded_step(got["rows"]), cfg.dt, cfg.wheel_base,
                          kff=gains["kff"][:B], alpha=1.0, bounds=bounds)
    assert np.array_equal(bits(got["rows"][..., 8:10]), bits(want["rows"][..., 8:10]))
    assert np.array_equal(got["n_clamped"], want["n_clamped"])
    assert np.array_equal(bits(got["rows"][..., 0]), bits(want["rows"][..., 0]))
    assert np.array_equal(bits(got["max_dev"]), bits(want["max_dev"])) and np.array_equal(bits(got["end_dev"]), bits(want["end_dev"]))
    u = got["rows"][..., :-1, 8:10]
    wrap = lambda v: float(policy.normalize_angle(np.float64(v)))    # noqa: E731
    assert u[..., 0].min() == cfg.jerk_min and u[..., 0].max() == cfg.jerk_max
    assert u[..., 1].min() == wrap(cfg.delta_rate_min) and u[..., 1].max() == wrap(cfg.delta_rate_max)
    assert got["n_clamped"].max() > 0 and got["n_clamped"].min() >= 0 and got["n_clamped"].max() <= traj.shape[1] - 1
    # without the clamp: the same bits for the chains no limit was applied to, other rows for every chain one was applied to
    free = opt.policy_rollout(traj[:B], api.ROWS_TRAJ, gains["Kfb"][:B], start, kff=gains["kff"][:B], alpha=1.0)
    assert np.all(free["n_clamped"] == 0)
    same = (bits(free["rows"]) == bits(got["rows"])).all(axis=(2, 3))
    assert np.array_equal(same, got["n_clamped"] == 0)


@pytest.mark.parametrize("B,S", [(65, 3), (3, 65)])
def test_n_out_and_optional_outputs(solved, gains, B, S):
    scene, traj, opt = solved
    K = traj.shape[1]
    off = np.resize(pc.offsets(), (S, 6))
    start = np.ascontiguousarray(traj[None, :B, 0, 1:7] + off[:, None, :])
    args = (traj[:B], api.ROWS_PLAN if S == 3 else api.ROWS_TRAJ)
    rows = _plan_rows(traj[:B]) if S == 3 else traj[:B]
    kw = dict(kff=gains["kff"][:B], alpha=0.5012, clamp=True)
    full = opt.policy_rollout(rows, args[1], gains["Kfb"][:B], start, **kw)
    for n_out in (1, 2, 6, K - 1):
        part = opt.policy_rollout(rows, args[1], gains["Kfb"][:B], start, n_out=n_out, **kw)
        assert part["rows"].shape == (S, B, n_out, 10)
        assert np.array_equal(bits(part["rows"][:, :, :n_out - 1]), bits(full["rows"][:, :, :n_out - 1])), n_out
        last = part["rows"][:, :, n_out - 1]
        assert np.array_equal(bits(last[..., :8]), bits(full["rows"][:, :, n_out - 1, :8])) and np.all(bits(last[..., 8:]) == 0), n_out
        d = np.hypot(part["rows"][..., 1] - traj[None, :B, :n_out, 1], part["rows"][..., 2] - traj[None, :B, :n_out, 2])
        dx, dy = part["rows"][..., 1] - traj[None, :B, :n_out, 1], part["rows"][..., 2] - traj[None, :B, :n_out, 2]
        d = np.sqrt(dx * dx + dy * dy)
        assert np.array_equal(bits(part["max_dev"]), bits(d.max(axis=-1))) and np.array_equal(bits(part["end_dev"]), bits(d[..., -1])), n_out
        if n_out == 1:
            assert np.array_equal(bits(part["rows"][:, :, 0, 1:7]), bits(start)) and np.all(part["n_clamped"] == 0)
    # summaries only, rows only: the bits of the full run
    p = api._ptr
    mx, en, nc = np.empty((S, B)), np.empty((S, B)), np.empty((S, B), np.int32)
    a = [np.ascontiguousarray(v) for v in (rows, gains["Kfb"][:B], gains["kff"][:B])]
    raw = lambda out, m, e, n: opt.policy_rollout_raw(B, args[1], p(a[0]), K, p(a[1]), p(a[2]), 0.5012, S, p(start), True, K,  # noqa: E731
                                                      p(out), p(m), p(e), p(n), api.MEM_HOST)
    assert raw(None, mx, en, nc) == api.OK
    assert np.array_equal(bits(mx), bits(full["max_dev"])) and np.array_equal(bits(en), bits(full["end_dev"]))
    assert np.array_equal(nc, full["n_clamped"])
    only = np.empty((S, B, K, 10))
    assert raw(only, None, None, None) == api.OK
    assert np.array_equal(bits(only), bits(full["rows"]))
    one = np.empty((S, B))
    assert raw(None, None, one, None) == api.OK and np.array_equal(bits(one), bits(full["end_dev"]))
    assert opt.policy_rollout(rows, args[1], gains["Kfb"][:B], start, rows_out=False, **kw)["rows"] is None


# ---------------------------------------------------------------------------------------------
# 7. host arrays = device arrays
@pytest.mark.parametrize("B,S", [(130, 8), (1, 1)])
def test_host_arrays_give_the_bits_of_device_arrays(solved, gains, B, S):
    import torch
    scene, traj, opt = solved
    dev = torch.device("cuda", 0)
    off = np.resize(pc.offsets(), (S, 6))
    start = np.ascontiguousarray(traj[None, :B, 0, 1:7] + off[:, None, :])
    rows = _plan_rows(traj[:B])
    host = opt.policy_rollout(rows, api.ROWS_PLAN, gains["Kfb"][:B], start, kff=gains["kff"][:B], alpha=1.0, clamp=True, n_out=7)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    try:
        d = opt.policy_rollout(to(rows), api.ROWS_PLAN, to(gains["Kfb"][:B]), to(start), kff=to(gains["kff"][:B]), alpha=1.0,
                               clamp=True, n_out=7)
        torch.cuda.synchronize()
        for n in ("rows", "max_dev", "end_dev"):
            assert np.array_equal(bits(d[n].cpu().numpy()), bits(host[n])), n
        assert np.array_equal(d["n_clamped"].cpu().numpy(), host["n_clamped"])
        # the gains call on device arrays
        sub = _first(scene, B)
        prob, keep = opt._host_problem(sub)
        t = dict(start=to(keep["start"]), coarse=to(keep["coarse"]), corridor=to(keep["corridor"]), ccount=to(keep["ccount"]))
        prob.memory = api.MEM_DEVICE
        prob.start, prob.coarse = t["start"].data_ptr(), t["coarse"].data_ptr()
        prob.corridor, prob.corridor_count = t["corridor"].data_ptr(), t["ccount"].data_ptr()
        N = opt.N
        dK, dk = torch.zeros((B, N, 2, 6), dtype=torch.float64, device=dev), torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
        ddV, dok = torch.zeros((B, 2), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        lam = to(np.full(B, pc.REF_LAMBDA))
        rc_ = opt.policy_gains_raw(prob, api.ROWS_PLAN, to(rows).data_ptr(), lam.data_ptr(), dK.data_ptr(), dk.data_ptr(),
                                   ddV.data_ptr(), dok.data_ptr())
        torch.cuda.synchronize()
        assert rc_ == api.OK
        for n, v in (("Kfb", dK), ("kff", dk), ("dV", ddV)):
            assert np.array_equal(bits(v.cpu().numpy()), bits(gains[n][:B])), n
        assert bool((dok == 1).all())
    finally:
        opt.set_stream(0)


# ---------------------------------------------------------------------------------------------
# 8. argument checks
def test_rollout_refusals(solved, gains):
    scene, traj, opt = solved
    B, S, K = 5, 2, traj.shape[1]
    a = dict(rows=np.ascontiguousarray(traj[:B]), K=np.ascontiguousarray(gains["Kfb"][:B]), k=np.ascontiguousarray(gains["kff"][:B]),
             start=np.ascontiguousarray(np.broadcast_to(traj[None, :B, 0, 1:7], (S, B, 6))), out=np.empty((S, B, K, 10)),
             mx=np.empty((S, B)))
    p = api._ptr

    def call(h=True, batch=B, layout=api.ROWS_TRAJ, rows="rows", n_knots=K, Kfb="K", kff="k", alpha=1.0, S_=S, start="start",
             n_out=K, out="out", mx="mx", memory=api.MEM_HOST):
        g = lambda n: None if n is None else p(a[n])    # noqa: E731
        return opt.L.cilqr_policy_rollout_batch(opt.h if h else None, batch, layout, g(rows), n_knots, g(Kfb), g(kff),
                                                api.C.c_double(alpha), S_, g(start), 0, n_out, g(out), g(mx), None, None, memory)
    refusals = [
        (dict(h=False), api.ERR_NULL), (dict(rows=None), api.ERR_NULL), (dict(Kfb=None), api.ERR_NULL),
        (dict(start=None), api.ERR_NULL), (dict(out=None, mx=None), api.ERR_NULL),
        (dict(memory=2), api.ERR_ARG), (dict(memory=-1), api.ERR_ARG),
        (dict(layout=api.ROWS_COARSE), api.ERR_ARG), (dict(layout=api.ROWS_CONTROLS), api.ERR_ARG),
        (dict(layout=api.ROWS_POINTS), api.ERR_ARG), (dict(layout=7), api.ERR_ARG),
        (dict(n_out=0), api.ERR_ARG), (dict(n_out=K + 1), api.ERR_ARG), (dict(n_out=-3), api.ERR_ARG),
        (dict(S_=0), api.ERR_ARG), (dict(S_=api.POLICY_MAX_SAMPLES + 1), api.ERR_ARG),
        (dict(alpha=float("nan")), api.ERR_ARG), (dict(alpha=float("inf")), api.ERR_ARG),
        (dict(n_knots=1, n_out=1), api.ERR_ARG), (dict(batch=0), api.ERR_ARG),
    ]
    assert call() == api.OK
    clean = a["out"].copy()
    for kw, code in refusals:
        assert call(**kw) == code, kw
        a["out"][:] = 0.0
        assert call() == api.OK, ("after", kw)
        assert np.array_equal(bits(a["out"]), bits(clean)), ("after", kw)
    assert call(kff=None, alpha=float("nan")) == api.OK          # alpha is not read without kff
    ticket = opt.submit(_first(scene, B))
    assert call() == api.ERR_STATE
    opt.collect(ticket)
    assert call() == api.OK
