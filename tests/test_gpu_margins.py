"""Constraint margins on the GPU (cilqr_constraint_margins_batch, kernels_margins.hip) against the host call
(cilqr_constraint_margins, which tests/test_margins.py holds to the NumPy statement bit for bit, to the crafted table and
to long double).

THE BOUND.  Both sides shrink and normalise every plane with the same operations on the same bits, so (a_n, b_n, c_n) and
hypot(a_n, b_n) are equal; the bound columns are one subtraction on the same bits: equal.  The sides differ by lean_sincos
against the C library's cos / sin for the heading, that is by the disc centres, and by how the last five operations round
on centres that differ.  Unit u = 2^-52 * M, M as in tests/test_margins.py (the largest of the coordinates, the offsets and
the live planes' distances from the origin |c_n| / hypot(a_n, b_n)); a rounded operation on a value <= 2 M costs at most 1 u:
  disc centre, per coordinate   cos / sin: the C library's below 1 ulp of a value <= 1 (0.5 u after the offset <= M),
                                lean_sincos about 1 ulp -- taken as 2 (1 u): 1.5 u; the product, rounded on either side:
                                1 u; the sum likewise: 1 u.  3.5 u per coordinate, two coordinates: 3.5 sqrt 2 < 5 u
  Lipschitz                     m is 1-Lipschitz in the centre: 5 u
  g and the division            two products, a sum, a difference, the division: 5 operations on either side: 10 u
5 + 10 = 15; BOUND_C = 2 * 15 = 30 (the count doubled).  The largest difference measured against the host call is printed
by every test (at most 0.03 of the bound).  Where the host's value is infinite the kernel's must be the same infinity.

`which`, min_knot and the bits of `violated` are compared only where DECIDED by the host's own numbers: the runner-up
among the candidates of a minimum (the NumPy statement's candidates, which equal the host call's bits) is more than twice
the bound above the best; a bit's |min_margin + tol| exceeds the bound; a disc's nearest lane segment is ahead of every
segment measured to another point by more than twice the bound (segments measured to the same end point tie in any
arithmetic: the first wins on both sides).  A lane value is compared where every disc of its knot has a decided segment.
At most 1 % of a test's entries may be undecided: a condition on the inputs, checked here with the host call alone and met by
the seeds below (none to a handful of entries per test; the generated rows keep the discs some decimetres from the strips
along the joints' normals).  The crafted table has heading 0 and dyadic geometry: it is held bit for bit inside a batch."""
import math

import numpy as np
import pytest

import margins_cases as mc
from cilqr_amd import api, margins, scenario

pytestmark = pytest.mark.gpu

UNDECIDED_SHARE = 0.01
BOUND_C = 30.0
U = 2.0 ** -52
INF = math.inf
HANDLE_CMAX = 24


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=192, cmax=HANDLE_CMAX, max_lane_segments=64) as o:
        yield o


@pytest.fixture(scope="module")
def dyadic():
    with api.BatchIlqrOptimizer(cfg=mc.dyadic_config(), batch_capacity=8, cmax=HANDLE_CMAX, max_lane_segments=8) as o:
        yield o


@pytest.fixture(scope="module")
def scenes():
    return scenario.generate("mix11", 192, seed=33)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _scale(cfg, rows, layout, corridor, count):
    F, cx, cy = margins.COLUMNS[layout][:3]
    v = np.abs(rows[..., [cx, cy]])
    veh = margins.vehicle(cfg)
    m = [float(v[np.isfinite(v)].max(initial=0.0)) + float(np.abs(veh["off"]).max())]
    cmax = corridor.shape[2]
    live = np.arange(cmax)[None, None, :] < np.clip(count, 0, cmax)[..., None]
    pa, pb, pc = margins.shrink_normalise(corridor[..., 0], corridor[..., 1], corridor[..., 2], veh["shrink_corridor"], True)
    with np.errstate(all="ignore"):
        d = np.abs(pc) / np.hypot(pa, pb)
    d = d[live & np.isfinite(d)]
    m.append(float(d.max(initial=0.0)))
    return max(m)


def _shape_problem(sc, B, K, cmax, first=0):
    """B problems of K knots and cmax stored planes out of the generated scenes (knots repeat cyclically beyond the scenario's;
    planes are cut -- the counts stay, so they are clamped -- or padded with planes no one may read)"""
    K0, c0 = sc["corridor"].shape[1:3]
    idx = np.arange(K) % K0
    cor = sc["corridor"][first:first + B][:, idx]
    cor = cor[:, :, :cmax] if cmax <= c0 else np.concatenate([cor, np.full((B, K, cmax - c0, 3), 9e9)], axis=2)
    part = {k: sc[k][first:first + B] for k in ("coarse",)}
    return dict(corridor=np.ascontiguousarray(cor), ccount=np.ascontiguousarray(sc["ccount"][first:first + B][:, idx]),
                left=sc["left"], right=sc["right"], **part)


def _device_call(opt, prob_dict, rows, layout, tol=None, per_knot=True, offset=3):
    """cilqr_constraint_margins_batch with every array resident on the device; the outputs are views `offset` elements into
    larger arrays of guard values, which must come back untouched."""
    import torch
    dev = torch.device("cuda", 0)
    B, K = rows.shape[:2]
    prob, keep = api.margin_problem(prob_dict, B, K)
    t_cor = torch.from_numpy(keep["corridor"]).to(dev)
    t_cnt = torch.from_numpy(keep["ccount"]).to(dev)
    t_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    prob.memory, prob.corridor, prob.corridor_count = api.MEM_DEVICE, t_cor.data_ptr(), t_cnt.data_ptr()
    sizes = dict(margins=(B * K * 8, torch.float64), which=(B * K * 6, torch.int32), min_margin=(B * 8, torch.float64),
                 min_knot=(B * 8, torch.int32), violated=(B, torch.int32))
    t = {k: torch.full((offset + n + 1,), 77, dtype=dt, device=dev) for k, (n, dt) in sizes.items()}
    ptr = lambda k: t[k].data_ptr() + offset * t[k].element_size()
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tol = None if tol is None else np.ascontiguousarray(tol, np.float64)
    rc, n = opt.constraint_margins_raw(prob, layout, t_rows.data_ptr(), ptr("margins") if per_knot else None,
                                       ptr("which") if per_knot else None, ptr("min_margin"), ptr("min_knot"), api._ptr(tol),
                                       ptr("violated"))
    torch.cuda.synchronize()
    opt.set_stream(0)
    assert rc == api.OK, rc
    out = {}
    for k, (cnt, dt) in sizes.items():
        a = t[k].cpu().numpy()
        assert (a[:offset] == 77).all() and a[offset + cnt] == 77, k
        if not per_knot and k in ("margins", "which"):
            assert (a == 77).all(), k
            continue
        out[k] = a[offset:offset + cnt]
    shapes = dict(margins=(B, K, 8), which=(B, K, 6), min_margin=(B, 8), min_knot=(B, 8), violated=(B,))
    out = {k: v.reshape(shapes[k]) for k, v in out.items()}
    out["violated"] = out["violated"].astype(np.uint32)
    out["n_violating"] = n
    return out


def _second(a, axis=-1):
    """the second smallest along an axis (+inf with fewer than two entries)"""
    if a.shape[axis] < 2:
        return np.full(np.delete(a.shape, axis), INF)
    return np.take(np.partition(a, 1, axis=axis), 1, axis=axis)


def _compare(cfg, prob, rows, layout, exact_ties, dev, tol=None, what=""):
    """the kernel's result `dev` against the host call on the same inputs, by the module text"""
    h = api.constraint_margins(cfg, prob, rows, layout, tol=tol, exact_ties=exact_ties)
    n = margins.constraint_margins(cfg, rows, layout, prob["corridor"], prob["ccount"], prob["left"], prob["right"], exact_ties,
                                   candidates=True)
    for k in ("margins", "which", "min_margin", "min_knot"):          # the candidates below are the host call's
        assert np.array_equal(_bits(h[k]), _bits(n[k])), k
    B, K = rows.shape[:2]
    bound = BOUND_C * U * _scale(cfg, rows, layout, prob["corridor"], prob["ccount"])
    hm, dm = h["margins"], dev["margins"]
    # ---- the bound families: the same subtraction on the same bits
    assert np.array_equal(_bits(hm[..., 3:]), _bits(dm[..., 3:])), what
    assert np.array_equal(_bits(h["min_margin"][:, 3:]), _bits(dev["min_margin"][:, 3:])), what
    assert np.array_equal(h["min_knot"][:, 3:], dev["min_knot"][:, 3:]), what
    # ---- decided?
    lane_decided = (n["lane_gaps"] > 2 * bound).all(axis=-1)                               # [2, B, K]: every disc's segment
    value_ok = np.ones((B, K, 3), bool)
    value_ok[..., 1], value_ok[..., 2] = lane_decided[0], lane_decided[1]
    with np.errstate(invalid="ignore"):
        cor_gap = _second(n["corridor_candidates"]) - hm[..., 0]
        lane_gap = [_second(n["lane_candidates"][s]) - hm[..., 1 + s] for s in range(2)]
    which_ok = np.zeros((B, K, 6), bool)
    which_ok[..., 0] = which_ok[..., 1] = np.isfinite(hm[..., 0]) & (cor_gap > 2 * bound)
    for s in range(2):
        which_ok[..., 2 + 2 * s] = which_ok[..., 3 + 2 * s] = lane_decided[s] & np.isfinite(hm[..., 1 + s]) & (lane_gap[s] > 2 * bound)
    which_ok |= (h["which"] == -1) & np.isposinf(np.repeat(hm[..., :3], 2, axis=-1))      # nothing to decide: +inf, -1
    # ---- per knot
    fin = np.isfinite(hm[..., :3])
    assert np.array_equal(np.where(value_ok & ~fin, hm[..., :3], 0), np.where(value_ok & ~fin, dm[..., :3], 0)), what
    err = np.where(value_ok & fin, np.abs(np.where(fin, dm[..., :3], 0) - np.where(fin, hm[..., :3], 0)), 0.0)
    assert np.array_equal(np.where(which_ok, dev["which"], 0), np.where(which_ok, h["which"], 0)), \
        (what, np.argwhere(which_ok & (dev["which"] != h["which"]))[:5])
    # ---- per problem: a column is comparable where all its knots are; its knot where the runner-up knot is far enough
    col_ok = value_ok.all(axis=1)                                                          # [B, 3]
    hmin, dmin = h["min_margin"][:, :3], dev["min_margin"][:, :3]
    fmin = np.isfinite(hmin)
    assert np.array_equal(np.where(col_ok & ~fmin, hmin, 0), np.where(col_ok & ~fmin, dmin, 0)), what
    err_min = np.where(col_ok & fmin, np.abs(np.where(fmin, dmin, 0) - np.where(fmin, hmin, 0)), 0.0)
    with np.errstate(invalid="ignore"):
        knot_gap = _second(hm[..., :3], axis=1) - hmin
    knot_ok = col_ok & ((fmin & (knot_gap > 2 * bound)) | np.isposinf(hmin))
    assert np.array_equal(np.where(knot_ok, dev["min_knot"][:, :3], 0), np.where(knot_ok, h["min_knot"][:, :3], 0)), what
    t3 = np.zeros(3) if tol is None else np.asarray(tol, np.float64)[:3]
    with np.errstate(invalid="ignore"):
        bit_ok = col_ok & (~fmin | (np.abs(hmin + t3) > bound))
    bits = lambda v: (v[:, None] >> np.arange(3, dtype=np.uint32)) & 1
    assert np.array_equal(np.where(bit_ok, bits(dev["violated"]), 0), np.where(bit_ok, bits(h["violated"]), 0)), what
    assert np.array_equal(dev["violated"] >> 3, h["violated"] >> 3), what
    if bit_ok.all():
        assert dev["n_violating"] == h["n_violating"] == int((margins.violated(h["min_margin"], tol) != 0).sum()), what
    assert dev["n_violating"] == int((dev["violated"] != 0).sum()), what
    undecided = [1.0 - value_ok.mean(), 1.0 - which_ok.mean(), 1.0 - knot_ok.mean(), 1.0 - bit_ok.mean()]
    print(f"{what}: bound {bound:.3g}, largest difference / bound {max(err.max(), err_min.max()) / bound:.4f}, "
          f"undecided values / which / knots / bits {undecided}")
    assert max(undecided) <= UNDECIDED_SHARE, (what, undecided)
    assert err.max() <= bound and err_min.max() <= bound, (what, err.max(), err_min.max(), bound)
    return h


# ---------------------------------------------------------------- the crafted table inside a batch, bit for bit
@pytest.mark.parametrize("exact_ties", (1, 0))
@pytest.mark.parametrize("layout,cmax,memory", [(api.ROWS_TRAJ, mc.CMAX, "host"), (api.ROWS_PLAN, HANDLE_CMAX, "device"),
                                                (api.ROWS_COARSE, 16, "host")])
def test_crafted_table_inside_a_batch_bit_for_bit(dyadic, layout, cmax, memory, exact_ties):
    cases = mc.crafted_table()
    order = cases + cases[::-1] + cases[7:20]          # every case at several places of the batch, among other neighbours
    prob, state = mc.problem(order, cmax)
    rows = mc.rows_in_layout(layout, state)
    dyadic.set_option(api.OPT_EXACT_LANE_TIES, exact_ties)
    try:
        d = _device_call(dyadic, prob, rows, layout) if memory == "device" else dyadic.constraint_margins(prob, rows, layout)
    finally:
        dyadic.set_option(api.OPT_EXACT_LANE_TIES, 1)
    h = api.constraint_margins(dyadic.cfg, prob, rows, layout, exact_ties=bool(exact_ties))
    for k in ("margins", "which", "min_margin", "min_knot", "violated"):
        assert np.array_equal(_bits(d[k]), _bits(h[k])), (k, np.argwhere(_bits(d[k]) != _bits(h[k]))[:5])
    assert d["n_violating"] == h["n_violating"] == int((h["violated"] != 0).sum())
    # a problem's result does not depend on its place: the first and the mirrored copy agree
    n = len(cases)
    for k in ("margins", "which", "min_margin", "min_knot", "violated"):
        assert np.array_equal(_bits(d[k][:n]), _bits(d[k][n:2 * n][::-1])), k


# ---------------------------------------------------------------- generated problems
SHAPES = [   # batch, knots, stored planes, layout, memory, exact lane ties
    (1, 51, 16, api.ROWS_TRAJ, "host", 1),
    (3, 1, 1, api.ROWS_COARSE, "device", 1),
    (64, 2, 24, api.ROWS_PLAN, "host", 0),
    (65, 65, 16, api.ROWS_TRAJ, "device", 1),
    (3, 256, 16, api.ROWS_PLAN, "device", 0),
    (192, 51, 1, api.ROWS_COARSE, "host", 1),
]


@pytest.mark.parametrize("B,K,cmax,layout,memory,exact_ties", SHAPES)
def test_kernel_against_host_call_on_generated_rows(opt, scenes, B, K, cmax, layout, memory, exact_ties):
    prob = _shape_problem(scenes, B, K, cmax, first=5 if B < 100 else 0)
    rows, _ = mc.generated_rows(prob, layout, seed=B + K, K=K)
    tol = np.array([1e-3, 0.25, 0.0, 0.0, 1e-3, 0.0, 2.0, 0.0])
    opt.set_option(api.OPT_EXACT_LANE_TIES, exact_ties)
    try:
        d = _device_call(opt, prob, rows, layout, tol) if memory == "device" else opt.constraint_margins(prob, rows, layout, tol=tol)
    finally:
        opt.set_option(api.OPT_EXACT_LANE_TIES, 1)
    _compare(opt.cfg, prob, rows, layout, bool(exact_ties), d, tol, f"generated {B}x{K}x{cmax}")


@pytest.fixture(scope="module")
def solved(opt, scenes):
    """one solve of 192 problems (the scenario's 16 planes per knot, on the handle made for 24), shared by the tests below"""
    g = opt.plan(scenes)
    assert np.all((g["status"] >= 1) & (g["status"] <= 5))
    return g["traj"]


def _plan_rows(traj):
    """the `plan` rows of a trajectory: time s x y theta kappa velocity a delta jerk delta_rate, s the running chord length"""
    B, K = traj.shape[:2]
    plan = np.zeros((B, K, api.PLAN_FIELDS))
    plan[..., 0] = traj[..., 0]
    step = np.hypot(np.diff(traj[..., 1], axis=1), np.diff(traj[..., 2], axis=1))
    plan[:, 1:, 1] = np.cumsum(step, axis=1)
    plan[..., 2:5] = traj[..., 1:4]
    plan[..., 5] = traj[..., 7]
    plan[..., 6:9] = traj[..., 4:7]
    plan[..., 9:11] = traj[..., 8:10]
    return plan


@pytest.mark.parametrize("layout,memory", [(api.ROWS_TRAJ, "device"), (api.ROWS_PLAN, "host")])
def test_kernel_against_host_call_on_a_solve(opt, scenes, solved, layout, memory):
    rows = solved if layout == api.ROWS_TRAJ else _plan_rows(solved)
    d = _device_call(opt, scenes, rows, layout) if memory == "device" else opt.constraint_margins(scenes, rows, layout)
    h = _compare(opt.cfg, scenes, rows, layout, True, d, None, f"solve {memory}")
    assert h["n_violating"] > 0          # relaxed barriers: converged trajectories do sit beyond constraints


def test_per_knot_outputs_are_optional_and_two_lane_groups(opt, scenes, solved):
    B = 65
    prob = {k: scenes[k][:B] if k in ("corridor", "ccount", "coarse") else scenes[k] for k in ("corridor", "ccount", "coarse", "left", "right")}
    rows = np.ascontiguousarray(solved[:B])
    full = opt.constraint_margins(prob, rows, api.ROWS_TRAJ)
    lean = _device_call(opt, prob, rows, api.ROWS_TRAJ, per_knot=False)
    for k in ("min_margin", "min_knot", "violated"):
        assert np.array_equal(_bits(full[k]), _bits(lean[k])), k
    assert full["n_violating"] == lean["n_violating"]
    # two groups with different tables: each part is the call with its own table, bit for bit (one kernel, the same inputs)
    cut = 22
    other_l, other_r = scenes["left"][3:].copy(), scenes["right"][:-4].copy()
    grouped = dict(prob, left=np.concatenate([scenes["left"], other_l]), right=np.concatenate([scenes["right"], other_r]),
                   lane_groups=[(0, len(scenes["left"]), len(scenes["right"])), (cut, len(other_l), len(other_r))])
    g = opt.constraint_margins(grouped, rows, api.ROWS_TRAJ)
    second = opt.constraint_margins(dict(corridor=prob["corridor"][cut:], ccount=prob["ccount"][cut:], left=other_l, right=other_r),
                                    rows[cut:], api.ROWS_TRAJ)
    for k in ("margins", "which", "min_margin", "min_knot", "violated"):
        assert np.array_equal(_bits(g[k][:cut]), _bits(full[k][:cut])), k
        assert np.array_equal(_bits(g[k][cut:]), _bits(second[k])), k
    assert (g["which"][cut:] != full["which"][cut:]).any()
    assert g["n_violating"] == int((g["violated"] != 0).sum())
    _compare(opt.cfg, dict(corridor=prob["corridor"][cut:], ccount=prob["ccount"][cut:], left=other_l, right=other_r), rows[cut:],
             api.ROWS_TRAJ, True, second, None, "second lane group")


# ---------------------------------------------------------------- the solver's own planes, and its state
def test_margins_from_the_planes_the_solver_uses(scenes, solved):
    """cilqr_stage_load + cilqr_stage_read give the shrunk, normalised planes of kernels_load.hip; margins rebuilt from them
    in NumPy (the host's disc centres) agree with the kernel's within the bound: the new copy of the arithmetic is the solver's."""
    B = 64
    sub = {k: scenes[k][:B] if k in ("start", "coarse", "corridor", "ccount") else scenes[k] for k in scenes if isinstance(scenes[k], np.ndarray)}
    rows = np.ascontiguousarray(solved[:B])
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=B, cmax=16, max_lane_segments=64) as o:
        o.stage_load(sub)
        cor, lanes = o.read(api.T_CORRIDOR), o.read(api.T_LANES)        # [B, K, 16, 3], [nl + nr, 3]
        d = o.constraint_margins(sub, rows, api.ROWS_TRAJ)
        cfg = o.cfg
    n = margins.constraint_margins(cfg, rows, api.ROWS_TRAJ, sub["corridor"], sub["ccount"], sub["left"], sub["right"], candidates=True)
    # the solver's planes are, bit for bit, the NumPy statement's (and so the host call's and the kernel's)
    veh = margins.vehicle(cfg)
    pa, pb, pc = margins.shrink_normalise(sub["corridor"][..., 0], sub["corridor"][..., 1], sub["corridor"][..., 2], veh["shrink_corridor"], True)
    live = np.arange(16)[None, None, :] < np.clip(sub["ccount"], 0, 16)[..., None]
    for got, want in zip((cor[..., 0], cor[..., 1], cor[..., 2]), (pa, pb, pc)):
        assert np.array_equal(_bits(got)[live], _bits(want)[live])
    nl = len(sub["left"])
    for tab, got in ((margins.prepare_lane(sub["left"], veh["shrink_lane"]), lanes[:nl]), (margins.prepare_lane(sub["right"], veh["shrink_lane"]), lanes[nl:])):
        assert np.array_equal(_bits(np.stack([tab["pa"], tab["pb"], tab["pc"]], axis=1)), _bits(got))
    # margins rebuilt from the solver's planes and the rows
    x, y, th = rows[..., 1], rows[..., 2], rows[..., 3]
    px = x[..., None] + veh["off"] * margins._elementwise("cos", th)[..., None]
    py = y[..., None] + veh["off"] * margins._elementwise("sin", th)[..., None]
    m = margins.plane_margin(cor[:, :, None, :, 0], cor[:, :, None, :, 1], cor[:, :, None, :, 2], px[..., None], py[..., None])
    rebuilt = np.where(live[:, :, None, :], m, INF).reshape(B, 51, -1).min(axis=-1)
    bound = BOUND_C * U * _scale(cfg, rows, api.ROWS_TRAJ, sub["corridor"], sub["ccount"])
    assert np.array_equal(np.isfinite(rebuilt), np.isfinite(d["margins"][..., 0]))
    fin = np.isfinite(rebuilt)
    assert np.abs(np.where(fin, rebuilt - np.where(fin, d["margins"][..., 0], 0), 0)).max() <= bound
    for s in range(2):
        seg = n["lane_segments"][s]
        p = lanes[:nl] if s == 0 else lanes[nl:]
        lane = margins.plane_margin(p[seg, 0], p[seg, 1], p[seg, 2], px, py).min(axis=-1)
        ok = (n["lane_gaps"][s] > 2 * bound).all(axis=-1)
        assert ok.mean() >= 1.0 - UNDECIDED_SHARE
        assert np.abs(np.where(ok, lane - d["margins"][..., 1 + s], 0)).max() <= bound


def test_staged_state_is_untouched(scenes, solved):
    B = 64
    sub = {k: scenes[k][:B] if k in ("start", "coarse", "corridor", "ccount") else scenes[k] for k in scenes if isinstance(scenes[k], np.ndarray)}
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=B, cmax=16, max_lane_segments=64) as o:
        o.stage_load(sub)
        o.stage_init_guess()
        before = o.stage_total_cost()
        x_before = o.read(api.T_X)
        # another batch size, another knot count, other lane tables: nothing of it may reach the staged problem
        prob = _shape_problem(scenes, 100, 65, 16, first=64)
        prob["left"], prob["right"] = scenes["left"][2:], scenes["right"][1:]
        rows, _ = mc.generated_rows(prob, api.ROWS_PLAN, seed=3, K=65)
        o.constraint_margins(prob, rows, api.ROWS_PLAN)
        after = o.stage_total_cost()                     # no CILQR_ERR_STATE: the stage flags are as they were
        assert np.array_equal(_bits(before), _bits(after)) and np.array_equal(_bits(x_before), _bits(o.read(api.T_X)))
        assert np.array_equal(_bits(o.read(api.T_LANES)), _bits(np.concatenate([
            np.stack([t["pa"], t["pb"], t["pc"]], axis=1) for t in (margins.prepare_lane(sub[s], margins.vehicle(o.cfg)["shrink_lane"]) for s in ("left", "right"))])))
        o.stage_quadratize()                             # ... and the sequence goes on


# ---------------------------------------------------------------- argument checks
def test_argument_checks_leave_the_outputs_unwritten(opt, scenes):
    B, K = 4, 51
    prob_dict = _shape_problem(scenes, B, K, 16)
    rows, _ = mc.generated_rows(prob_dict, api.ROWS_TRAJ, seed=1)

    def refused(code, change=None, layout=api.ROWS_TRAJ, tol=None, drop=None, no_rows=False, the_dict=prob_dict):
        prob, keep = api.margin_problem(the_dict, B, K)
        if change:
            for f, v in change.items():
                setattr(prob, f, v)
        out = dict(margins=np.full((B, K, 8), 77.0), which=np.full((B, K, 6), 77, np.int32), min_margin=np.full((B, 8), 77.0),
                   min_knot=np.full((B, 8), 77, np.int32), violated=np.full(B, 77, np.uint32))
        p = {k: (None if k == drop else api._ptr(v)) for k, v in out.items()}
        rc, n = opt.constraint_margins_raw(prob, layout, None if no_rows else api._ptr(rows), p["margins"], p["which"], p["min_margin"],
                                           p["min_knot"], api._ptr(tol), p["violated"])
        assert rc == code, (rc, code)
        assert n == 0 and all((v == 77).all() for v in out.values())

    refused(api.ERR_NULL, no_rows=True)
    for drop in ("min_margin", "min_knot", "violated"):
        refused(api.ERR_NULL, drop=drop)
    for layout in (api.ROWS_POINTS, api.ROWS_CONTROLS, -1):
        refused(api.ERR_ARG, layout=layout)
    refused(api.ERR_ARG, dict(n_knots=0))
    refused(api.ERR_ARG, dict(batch=0))
    refused(api.ERR_ARG, dict(memory=3))
    for bad in (-1.0, math.nan, math.inf):
        tol = np.zeros(8)
        tol[0] = bad
        refused(api.ERR_ARG, tol=tol)
    refused(api.ERR_CONSTRAINTS, dict(corridor=None))
    refused(api.ERR_CONSTRAINTS, dict(n_right=0))
    refused(api.ERR_CAPACITY, dict(cmax=HANDLE_CMAX + 1))
    long_table = np.tile(prob_dict["left"], (3, 1))[:65]
    refused(api.ERR_CAPACITY, the_dict=dict(prob_dict, left=long_table))
    assert api.lib().cilqr_constraint_margins_batch(None, None, 0, None, None, None, None, None, None, None, None) == api.ERR_NULL
    # while a solve is submitted the handle is busy
    ticket = opt.submit({k: (scenes[k][:8] if k in ("start", "coarse", "corridor", "ccount") else scenes[k]) for k in scenes if isinstance(scenes[k], np.ndarray)})
    try:
        refused(api.ERR_STATE)
    finally:
        opt.collect(ticket)
    opt.constraint_margins(prob_dict, rows, api.ROWS_TRAJ)      # ... and usable again
