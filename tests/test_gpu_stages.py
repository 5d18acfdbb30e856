"""The cost and quadratise kernels (quad_core.hpp, kernels_quad.hip, the barrier and lane code of dev_model.hpp) run through
the stage API at CRAFTED states -- cilqr_stage_set_trajectory puts the table of tests/stage_cases.py on the device -- and held
against the double-precision oracle and against the long-double statement of tests/stage_reference.py, entry by entry at
STAGE_TOL = 1e-9 (parity_util.entry_err).  Shapes are the table's: up to 300 problems of N = 7.

cmax = 70: a handle with 70 planes per knot is created as asked (cilqr_create accepts any cmax >= 1; the load kernel tiles
its transpose)."""
import numpy as np
import pytest

import stage_cases as sc
import stage_reference as sr
from parity_util import REL_TOL, entry_err, rel_err
from cilqr_amd import api
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
STAGE_TOL = 1e-9
TENSORS = dict(A=api.T_A, B=api.T_B, lx=api.T_LX, lu=api.T_LU, lxx=api.T_LXX, luu=api.T_LUU)
KNOT_TENSORS = ("lx", "lxx")              # have a terminal row; the others end at the last step
BIG = 320                                 # capacity of the handle that is larger than every batch


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _handle(name, cmax, capacity, exact):
    cfg = api.default_config(sc.N_STEPS, **sc.CONFIGS[name])
    opt = api.BatchIlqrOptimizer(cfg, batch_capacity=capacity, cmax=cmax)
    opt.set_option(api.OPT_EXACT_LANE_TIES, int(exact))
    return opt


def _first(scene, B):
    n = scene["coarse"].shape[0]
    return {k: (np.ascontiguousarray(v[:B]) if isinstance(v, np.ndarray) and v.shape[:1] == (n,) and k not in ("left", "right") else v)
            for k, v in scene.items()}


def _stages(opt, scene, X, U):
    """load, set the crafted trajectory, cost, quadratise: everything the device reports"""
    opt.stage_load(scene)
    opt.stage_set_trajectory(X, U)
    out = dict(goals=opt.read(api.T_GOALS), cor=opt.read(api.T_CORRIDOR), lanes=opt.read(api.T_LANES),
               X=opt.read(api.T_X), U=opt.read(api.T_U), cost=opt.stage_total_cost())
    opt.stage_quadratize()
    for k, t in TENSORS.items():
        out[k] = opt.read(t)
    return out


_DEVICE = {}


def _device(name, exact, cmax, capacity, B):
    """One run of the stages per (configuration, tie rule, group, layout), shared by the tests and left unchanged."""
    key = (name, exact, cmax, capacity, B)
    if key not in _DEVICE:
        g = sc.evaluate(name, exact, int(exact))[cmax]
        opt = _handle(name, cmax, capacity, exact)
        _DEVICE[key] = _stages(opt, _first(g["scene"], B), g["X"][:B], g["U"][:B])
        opt.close()
    return _DEVICE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _errors(got, ref, B):
    out = {"cost": entry_err(got["cost"], np.asarray(ref["cost"][:B], np.float64))}
    for k in TENSORS:
        g, r = np.asarray(got[k]), np.asarray(ref[k][:B], np.float64)
        out[k] = entry_err(g.reshape((-1,) + g.shape[2:]), r.reshape((-1,) + r.shape[2:]))
    return out


def _long_double_for(g, dev, B):
    """The long-double statement on the stage inputs the DEVICE holds: the cached one where they are the oracle's bit for bit."""
    nl = g["left"][0].shape[0]
    live = np.arange(g["cor"].shape[2])[None, None, :] < g["scene"]["ccount"][:B, :, None]
    same = (np.array_equal(dev["goals"][:, :, :3], g["goals"][:B, :, :3]) and np.array_equal(dev["cor"][live], g["cor"][:B][live])
            and np.array_equal(dev["lanes"][:nl], g["left"][0]) and np.array_equal(dev["lanes"][nl:], g["right"][0]))
    if same:
        return g["ld"], True
    left, right = (dev["lanes"][:nl], g["left"][1]), (dev["lanes"][nl:], g["right"][1])
    return sr.problems(g["X"][:B], g["U"][:B], dev["goals"], dev["cor"], g["scene"]["ccount"][:B], left, right, g["cfg"]), False


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", ["batch", BIG])
def test_set_trajectory_and_read_return_the_same_bits(capacity):
    """cilqr_stage_set_trajectory then read(T_X), read(T_U): the bits that went in, for batches that end inside a wave, on
    its border, inside a 256-thread block and beyond it, with the slot stride equal to and larger than the batch."""
    g = sc.evaluate("default")[sc.MAIN_CMAX]
    for B in (1, 63, 64, 65, 257, 300):
        opt = _handle("default", sc.MAIN_CMAX, B if capacity == "batch" else BIG, True)
        opt.stage_load(_first(g["scene"], B))
        X, U = g["X"][:B].copy(), g["U"][:B].copy()
        X[0, 0, 4], U[0, 0, 1] = -0.0, np.nextafter(0.0, 1.0)           # a signed zero and a denormal travel unchanged too
        opt.stage_set_trajectory(X, U)
        assert np.array_equal(_bits(opt.read(api.T_X)), _bits(X)), B
        assert np.array_equal(_bits(opt.read(api.T_U)), _bits(U)), B
        # a second set replaces the first completely
        opt.stage_set_trajectory(X[::-1], U[::-1])
        assert np.array_equal(_bits(opt.read(api.T_X)), _bits(X[::-1])) and np.array_equal(_bits(opt.read(api.T_U)), _bits(U[::-1])), B
        opt.close()


@pytest.mark.parametrize("exact", [False, True], ids=["ties_off", "ties_on"])
@pytest.mark.parametrize("name", list(sc.CONFIGS))
def test_cost_and_quadratize_on_the_crafted_table(name, exact):
    """Every group of the table (cmax 1, 2, 5, 16, 70), capacity = batch and capacity 320 (main group: B = 300 and 257):
    five cost components and A, B, lx, lu, lxx, luu per entry against the oracle and the long-double statement; the layouts
    agree bit for bit; a case placed at two slots gives the same bits."""
    groups = sc.evaluate(name, exact, int(exact))
    worst = {}
    for cmax, g in groups.items():
        n_all = g["X"].shape[0]
        layouts = [(n_all, n_all), (BIG, n_all)] + ([(BIG, 257)] if cmax == sc.MAIN_CMAX else [])
        runs = []
        for capacity, B in layouts:
            dev = _device(name, exact, cmax, capacity, B)
            runs.append((B, dev))
            assert np.array_equal(_bits(dev["X"]), _bits(g["X"][:B])) and np.array_equal(_bits(dev["U"]), _bits(g["U"][:B]))
            ld, cached = _long_double_for(g, dev, B)
            note = "" if cached else " (the device's stage inputs are not the oracle's bit for bit)"
            for against, ref in (("oracle", g["oracle"]), ("long double", ld)):
                for k, (e, where) in _errors(dev, ref, B).items():
                    worst[(against, k)] = max(worst.get((against, k), 0.0), e)
                    print(f"[{name} ties {int(exact)} cmax {cmax} cap {capacity} B {B}] {k} vs {against}: {e:.3e} at {where}{note}")
            for against, ref in (("oracle", g["oracle"]), ("long double", ld)):
                for k, (e, where) in _errors(dev, ref, B).items():
                    assert e < STAGE_TOL, (name, exact, cmax, capacity, B, against, k, e, where)
        # the layouts, problem by problem
        B0, d0 = runs[0]
        for B, d in runs[1:]:
            for k in ("cost",) + tuple(TENSORS):
                assert np.array_equal(_bits(d[k]), _bits(d0[k][:B])), (name, cmax, B, k)
        # the same case at two slots: interior knots against interior, terminal against terminal
        which = g["which"]
        first_at = {}
        pairs = 0
        for b in range(n_all):
            for i in range(sc.K):
                kind = (int(which[b, i]), i == sc.K - 1)
                if kind not in first_at:
                    first_at[kind] = (b, i)
                    continue
                b1, i1 = first_at[kind]
                pairs += 1
                for k in (KNOT_TENSORS if i == sc.K - 1 else tuple(TENSORS)):
                    assert np.array_equal(_bits(d0[k][b, i]), _bits(d0[k][b1, i1])), (name, cmax, k, (b, i), (b1, i1), g["cases"][which[b, i]]["name"])
        assert pairs > 0 or n_all == len(g["cases"])
    print(f"[{name} ties {int(exact)}] worst: " + ", ".join(f"{a} {k} {v:.2e}" for (a, k), v in sorted(worst.items())))


@pytest.mark.parametrize("name", ["default", "barrier", "dyadic_eps"])
def test_bounds_exactly_on_the_edge_take_the_side_the_double_g_selects(name):
    """The bound cases at g = -eps (or the nearest double beside it) and at the neighbour on the log side: the diagonal Hessian
    entry of the bound's own component equals the long-double value of the branch the double g selects.  The two sides
    differ by the factor 1 / eps, so STAGE_TOL decides."""
    g = sc.evaluate(name, True, 1)[sc.MAIN_CMAX]
    B = g["X"].shape[0]
    dev = _device(name, True, sc.MAIN_CMAX, B, B)
    ld, _ = _long_double_for(g, dev, B)
    eps = float(g["cfg"].barrier_eps)
    comp = dict(v=3, a=4, delta=5, jerk=0, rate=1)
    checked = {}
    for b in range(B):
        for i in range(sc.K):
            c = g["cases"][g["which"][b, i]]
            if c["cls"] != "bound" or ":edge" not in c["name"]:
                continue
            what = c["name"].split("_")[0]
            if what in ("jerk", "rate"):
                if i == sc.K - 1:
                    continue
                got, want = dev["luu"][b, i, comp[what], comp[what]], ld["luu"][b, i, comp[what], comp[what]]
            else:
                got, want = dev["lxx"][b, i, comp[what], comp[what]], ld["lxx"][b, i, comp[what], comp[what]]
            err = abs(got - float(want)) / abs(float(want))
            checked.setdefault(c["name"], []).append((float(want), err))
            assert err < STAGE_TOL, (name, c["name"], (b, i), got, float(want))
    assert len(checked) == 20, sorted(checked)                      # ten bounds, the edge and its neighbour
    for bound in {n.split(":")[0] for n in checked}:
        on = [n for n in checked if n.startswith(bound + ":edge_exact") or n.startswith(bound + ":edge_nearest")][0]
        ratio = checked[bound + ":edge_log_neighbour"][0][0] / checked[on][0][0]
        print(f"[{name}] {on}: Hessian entry {checked[on][0][0]:.6g}, log-side neighbour {ratio:.4g} times that; worst error "
              f"{max(e for _, e in checked[on] + checked[bound + ':edge_log_neighbour']):.2e}")
        assert ratio > 0.4 / eps                                        # (the opposite bound's own term is in both)


def test_backward_and_forward_from_the_crafted_quadratisation():
    """cilqr_stage_backward with a lambda per problem on the crafted quadratisation (relaxed terms of 1e4 beside entries of 1):
    the one-lane, team and wave kernels agree bit for bit and with the oracle's Backward fed the device's own q; then
    cilqr_stage_forward at the largest, a middle and the smallest step of the line search against the oracle's Forward, with
    test_stage_parity's rule (tight where the oracle's rollout stays physical).
    (lambda 0 .. 1e11, every configuration, the horizons 1 .. 5 and 64 .. 130, all eleven step sizes and the long-double
    statement of these stages: tests/test_gpu_riccati.py.)"""
    g = sc.evaluate("default", True, 1)[sc.MAIN_CMAX]
    B = g["X"].shape[0]
    opt = _handle("default", sc.MAIN_CMAX, B, True)
    opt.stage_load(g["scene"])
    opt.stage_set_trajectory(g["X"], g["U"])
    opt.stage_quadratize()
    q = {k: opt.read(t) for k, t in TENSORS.items()}
    lam = np.linspace(0.5, 3.0, B)
    outs = []
    for team, wave in ((0, 0), (4096, 0), (0, 4096)):
        opt.set_option(api.OPT_TEAM_THRESHOLD, team)
        opt.set_option(api.OPT_WAVE_THRESHOLD, wave)
        opt.stage_backward(lam)
        outs.append([opt.read(t) for t in (api.T_KFB, api.T_KFF, api.T_DV, api.T_GNORM)])
    for other in outs[1:]:
        for a, b_ in zip(outs[0], other):
            assert np.array_equal(_bits(a), _bits(b_))
    Kfb, kff, dV, gn = outs[0]
    o = orc.Oracle(g["cfg"])
    worst = np.zeros(3)
    ref = []
    for b in range(B):
        assert o.set_problem(g["scene"]["start"][b], g["scene"]["coarse"][b], g["scene"]["corridor"][b], g["scene"]["ccount"][b],
                             g["scene"]["left"], g["scene"]["right"]) == 0
        ref.append(o.backward(float(lam[b]), {k: q[k][b] for k in q}))
        worst = np.maximum(worst, [rel_err(Kfb[b], ref[b][0], 1e-6), rel_err(kff[b], ref[b][1], 1e-6), rel_err(dV[b], ref[b][2], 1e-6)])
    print(f"backward vs oracle, worst rel_err: K {worst[0]:.3e}, k {worst[1]:.3e}, dV {worst[2]:.3e}; largest |lxx| {np.abs(q['lxx']).max():.3g}")
    for b in range(B):
        oK, ok_, odV = ref[b]
        assert rel_err(Kfb[b], oK, 1e-6) < STAGE_TOL and rel_err(kff[b], ok_, 1e-6) < STAGE_TOL, b
        assert rel_err(dV[b], odV, 1e-6) < STAGE_TOL, b
        assert gn[b] == pytest.approx(o.grad_norm(kff[b], g["U"][b]), rel=1e-12)
    for alpha in (1.0, 0.2512, 0.0010):
        opt.stage_forward(alpha)
        Xc, Uc = opt.read(api.T_XCAND), opt.read(api.T_UCAND)
        figures = []
        for b in range(B):
            assert o.set_problem(g["scene"]["start"][b], g["scene"]["coarse"][b], g["scene"]["corridor"][b], g["scene"]["ccount"][b],
                                 g["scene"]["left"], g["scene"]["right"]) == 0
            oXn, oUn = o.forward(alpha, g["X"][b], g["U"][b], Kfb[b], kff[b])
            tame = np.all(np.abs(oXn[:, 5]) < 0.7) and np.all(np.abs(oXn[:, 3]) < 30.0)
            figures.append((bool(tame), rel_err(Xc[b], oXn), rel_err(Uc[b], oUn, 1e-3)))
        f = np.array(figures)
        print(f"forward alpha {alpha}: {int(f[:, 0].sum())} of {B} rollouts tame; worst error tame "
              f"{f[f[:, 0] == 1, 1:].max() if f[:, 0].any() else 0.0:.3e}, others {f[f[:, 0] == 0, 1:].max() if (f[:, 0] == 0).any() else 0.0:.3e}")
        for b, (tame, ex, eu) in enumerate(figures):
            ftol = STAGE_TOL if tame else REL_TOL
            assert ex < ftol and eu < ftol, (alpha, b, tame, ex, eu)
    opt.close()


def test_first_cost_row_of_a_solve_from_crafted_controls():
    """The crafted controls as a warm start with shift 0: jerk and steering rate beyond their bounds, so that the rollout leaves
    the velocity, acceleration and steering bounds too.  The first Cost row is the same bits from the tail kernel and from the
    lockstep loop, and equals the long-double total cost of the device's own first iterate."""
    g = sc.evaluate("default")[sc.MAIN_CMAX]
    B = g["X"].shape[0]
    cfg = g["cfg"]
    scene = dict(g["scene"])
    scene["start"] = g["scene"]["start"].copy()
    scene["start"][:, 3] = np.linspace(17.0, 19.9, B)                    # close under max_velocity: the rollout crosses it
    rows = np.zeros((B, sc.N_STEPS, 2))
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    rows[:, :, 0] = (sign * (cfg.jerk_max + 0.5 + 6.0 * (np.arange(B) % 5) / 4.0))[:, None]
    rows[:, :, 1] = (np.roll(sign, 1) * (cfg.delta_rate_max + 0.9 + 0.1 * (np.arange(B) % 7)))[:, None]
    rows[::9, 3:, :] *= -1.0                                                # some change side half-way
    out = {}
    for loop, tail in (("tail", None), ("lockstep", 0)):
        opt = api.BatchIlqrOptimizer(api.default_config(sc.N_STEPS, max_iter=2), batch_capacity=B, cmax=sc.MAIN_CMAX)
        if tail is not None:
            opt.set_option(api.OPT_TAIL_THRESHOLD, tail)
        out[loop] = opt.plan(scene, max_iter_trajs=1, warm=(rows, None, api.ROWS_CONTROLS))
        opt.close()
    a, b_ = out["tail"], out["lockstep"]
    assert np.array_equal(_bits(a["iter_trajs"][:, 0]), _bits(b_["iter_trajs"][:, 0]))
    assert np.array_equal(_bits(a["cost_hist"][:, 0]), _bits(b_["cost_hist"][:, 0]))
    X = np.ascontiguousarray(a["iter_trajs"][:, 0, :, 1:7])
    U = np.ascontiguousarray(a["iter_trajs"][:, 0, :-1, 8:10])
    assert np.array_equal(_bits(U[:, :, 0]), _bits(rows[:, :, 0]))      # the jerk rows as given (the rate is wrapped by the rollout)
    assert (X[:, :, 3].max(axis=1) > cfg.max_velocity).any() and (np.abs(X[:, :, 4]).max(axis=1) > cfg.max_acceleration).mean() > 0.8
    assert (np.abs(X[:, :, 5]).max(axis=1) > cfg.delta_max).mean() > 0.8
    ld = sr.problems(X, U, g["goals"], g["cor"], scene["ccount"], g["left"], g["right"], cfg)
    # (goals[0] is the start state: its v differs from the table's, and the target cost does not read v)
    e, where = entry_err(a["cost_hist"][:, 0], np.asarray(ld["cost"], np.float64))
    print(f"first Cost row vs long double: {e:.3e} at {where}; bounds component between {a['cost_hist'][:, 0, 2].min():.4g} and "
          f"{a['cost_hist'][:, 0, 2].max():.4g}")
    assert e < STAGE_TOL, (e, where)
