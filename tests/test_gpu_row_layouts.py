"""Where a row layout keeps what a rule names, held on the GPU.  Host and device take their column numbers from ONE table
(include/cilqr/row_layouts.hpp), so a wrong table agrees with itself and the comparisons of a kernel with its host call no
longer see it.  What still does, and is asserted here on one small fixed batch (3 trajectories of 6 rows, one pair of equal
times):

  (a) every call that reads rows -- check_collisions, clearance, constraint_margins, carry, track, frenet, warm rows --
      gets the SAME trajectory written in CILQR_ROWS_TRAJ, _PLAN and _COARSE by the literal column numbers below (this
      file's own statement of include/cilqr.h), once clean and once with a NaN in every column the rule does not read
      according to the "columns read" lines of include/cilqr.h.  The poisoned result must equal the clean one bit for
      bit, and both the result of the host call; and what the layouts share must agree between the layouts, which is
      what shows two columns that are both read changing places.
  (b) resample writes every column: by time the columns the three layouts share agree bit for bit, by station those of
      CILQR_ROWS_PLAN and _COARSE.

The trajectories run straight along x with heading 0 at dyadic coordinates, so that the sines, cosines and chord lengths
on both sides are exact and a kernel's row can be held to its host call's by bits.  The test is about behaviour, not about
the header: it passes on a library from before the table."""
import numpy as np
import pytest

import collision_cases as cc
import margins_cases as mc
from cilqr_amd import api, scenario, scene_io
from resample_cases import same_rows

B, K, M, N_DRIVE = 3, 6, 7, 3
NAMES = ("time", "station", "x", "y", "theta", "kappa", "v", "a", "delta", "jerk", "rate")
# include/cilqr.h, written out here a second time: the column of every name, per layout
COLUMNS = {
    api.ROWS_TRAJ: dict(time=0, x=1, y=2, theta=3, v=4, a=5, delta=6, kappa=7, jerk=8, rate=9),
    api.ROWS_PLAN: dict(time=0, station=1, x=2, y=3, theta=4, kappa=5, v=6, a=7, delta=8, jerk=9, rate=10),
    api.ROWS_COARSE: dict(time=0, station=1, x=2, y=3, theta=4, kappa=5, v=6, a=7, delta=8),
}
LAYOUTS = (api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE)
# the "columns read" of include/cilqr.h, by name (track: a and delta of row 0 only, the start state)
READS = dict(audit=("time", "x", "y", "theta"), margins=("x", "y", "theta", "v", "a", "delta", "jerk", "rate"),
             carry=("time", "x", "y", "theta", "kappa", "v", "a", "delta"), track=("time", "station", "x", "y", "theta", "v"),
             frenet=("x", "y"), warm=("jerk", "rate"))


def _fields():
    """name -> [B, K]: three straight runs along x, heading 0; rows 2 and 3 share their time"""
    k = np.arange(K, dtype=np.float64)
    b = np.arange(B, dtype=np.float64)[:, None]
    x = 2.0 + 4.0 * b + np.array([0.0, 1.0, 2.0, 2.25, 3.0, 4.0])
    f = dict(time=np.broadcast_to(np.array([0.0, 0.5, 1.0, 1.0, 1.5, 2.0]) + 0.0 * b, (B, K)), x=x, y=0.5 * b - 0.5 + 0.0 * k,
             theta=np.zeros((B, K)), kappa=0.015625 * k + 0.0 * b, v=2.0 + 0.25 * k + 0.125 * b, a=0.25 - 0.125 * k + 0.0 * b,
             delta=0.03125 * k + 0.0 * b, jerk=0.125 * (k + 1.0) + 0.5 * b, rate=0.0625 - 0.03125 * k + 0.0 * b)
    f["station"] = x - x[:, :1]   # the chord length of a straight run, exact
    return {n: np.ascontiguousarray(v) for n, v in f.items()}


def _rows(layout, keep=None, row0=()):
    """[B, K, F] rows of `layout`; keep: the names whose columns stay, NaN in every other one (row0: kept in row 0 only)"""
    f = _fields()
    cols = COLUMNS[layout]
    rows = np.full((B, K, api.ROWS_FIELDS[layout]), np.nan)
    for name, c in cols.items():
        if keep is None or name in keep:
            rows[:, :, c] = f[name]
        elif name in row0:
            rows[:, 0, c] = f[name][:, 0]
    return np.ascontiguousarray(rows)


def _pair(layout, rule, row0=()):
    return _rows(layout), _rows(layout, READS[rule], row0)


def _same(a, b):
    if isinstance(a, dict):
        return all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return same_rows(np.asarray(a), np.asarray(b))


# ---- the scene of the audits: a square beside the second run, a moving square that meets the first run
def _scenes():
    center = cc.straight_center(length=30.0)
    square = lambda cx, cy, h: np.array([[cx + h, cy + h], [cx + h, cy - h], [cx - h, cy - h], [cx - h, cy + h]])
    traj = np.array([[0.0, 9.0, -0.5, 0.0], [2.0, 3.0, -0.5, 0.0]])   # time x y theta: towards the first run
    scene = scene_io.Scene(np.zeros(4), np.zeros((1, 6)), [square(9.0, 2.25, 0.5)], [scene_io.DynamicObstacle(square(0.0, 0.0, 0.5), traj)])
    return center, [scene] * B


def _margin_problem():
    corridor = np.full((B, K, 4, 3), 9e9)
    corridor[:, :, 0] = (0.0, 1.0, 3.0)     # y <= 3
    corridor[:, :, 1] = (0.0, -1.0, 3.0)    # y >= -3
    corridor[:, :, 2] = (1.0, 0.0, 16.0)    # x <= 16
    left, right = mc.tables()
    return dict(corridor=corridor, ccount=np.full((B, K), 3, np.int32), left=left, right=right)


ADVANCE = np.array([0.25, 0.5, 1.0])
CARRY = dict(max_advance=1.5, n_knots=5, delta_t=0.25)


def _host(rule, layout, rows, cfg):
    """the host call of `rule` on [B, K, F] rows: one comparable object"""
    if rule in ("collisions", "clearance"):
        center, scenes = _scenes()
        flat = [scene_io.flatten_scene(center, s) for s in scenes]
        if rule == "collisions":
            r = [api.check_collisions(flat[b], rows[b], layout, buffer=0.25) for b in range(B)]
            return dict(mask=np.stack([v[0] for v in r]), first_hit=np.array([v[1] for v in r]), n_hit=np.array([v[2] for v in r]))
        r = [api.clearance_rows(flat[b], rows[b], layout) for b in range(B)]
        return dict(clearance=np.stack([v[0] for v in r]), nearest=np.stack([v[1] for v in r]),
                    min_clearance=np.array([v[2] for v in r]), min_knot=np.array([v[3] for v in r]))
    if rule == "margins":
        r = api.constraint_margins(cfg, _margin_problem(), rows, layout)
        return {k: r[k] for k in ("margins", "which", "min_margin", "min_knot", "violated")}
    if rule == "carry":
        r = [api.carry_rows(rows[b], layout, float(ADVANCE[b]), **CARRY) for b in range(B)]
        return {k: np.stack([np.asarray(v[k]) for v in r]) for k in ("coarse9", "coarse6", "knots3", "station", "state")}
    if rule == "track":
        r = [api.track_rows(cfg, None, rows[b], layout, None, N_DRIVE) for b in range(B)]
        return dict(driven=np.stack([v[0] for v in r]), ok=np.array([int(v[1]) for v in r]))
    if rule == "frenet":
        center, _ = _scenes()
        return dict(frenet=np.stack([api.frenet_rows(center, rows[b], layout) for b in range(B)]))
    raise KeyError(rule)


def _device(opt, rule, layout, rows):
    if rule in ("collisions", "clearance"):
        center, scenes = _scenes()
        packed = scene_io.pack_scene_batch(center, scenes)
        if rule == "collisions":
            r = opt.check_collisions(packed, rows, layout, buffer=0.25)
            return {k: r[k] for k in ("mask", "first_hit", "n_hit")}
        r = opt.clearance(packed, rows, layout)
        return {k: r[k] for k in ("clearance", "nearest", "min_clearance", "min_knot")}
    if rule == "margins":
        r = opt.constraint_margins(_margin_problem(), rows, layout)
        return {k: r[k] for k in ("margins", "which", "min_margin", "min_knot", "violated")}
    if rule == "carry":
        r = opt.carry(rows, layout, ADVANCE, **CARRY)
        return {k: r[k] for k in ("coarse9", "coarse6", "knots3", "station", "state")}
    if rule == "track":
        driven, ok = opt.track(rows, layout, None, N_DRIVE)
        return dict(driven=driven, ok=ok)
    if rule == "frenet":
        center, _ = _scenes()
        return dict(frenet=opt.frenet(center, rows, layout))
    raise KeyError(rule)


# rule -> (the names it reads, those it reads in row 0 only)
RULES = dict(collisions=("audit", ()), clearance=("audit", ()), margins=("margins", ()), carry=("carry", ()),
             track=("track", ("a", "delta")), frenet=("frenet", ()))


def _shared(rule, r):
    """what the three layouts must agree on: everything, but for the margins of the controls CILQR_ROWS_COARSE does not have"""
    if rule != "margins":
        return r
    return dict(margins=r["margins"][..., :6], min_margin=r["min_margin"][..., :6], min_knot=r["min_knot"][..., :6])


@pytest.fixture(scope="module")
def cfg():
    return mc.dyadic_config(50)


@pytest.mark.parametrize("rule", sorted(RULES))
def test_host_calls_ignore_the_columns_they_do_not_read(built, cfg, rule):
    """the host call alone, no GPU: invariant under the poison, and the layouts agree"""
    reads, row0 = RULES[rule]
    results = []
    for layout in LAYOUTS:
        clean, poisoned = _pair(layout, reads, row0)
        want = _host(rule, layout, clean, cfg)
        assert _same(_host(rule, layout, poisoned, cfg), want), (rule, layout)
        results.append(_shared(rule, want))
    assert _same(results[1], results[0]) and _same(results[2], results[0]), rule


@pytest.fixture(scope="module")
def opt(built, cfg):
    with api.BatchIlqrOptimizer(cfg, batch_capacity=4, cmax=4, max_lane_segments=64) as o:
        yield o


@pytest.mark.gpu
@pytest.mark.parametrize("rule", sorted(RULES))
def test_kernels_read_the_columns_of_the_rule_and_no_others(opt, cfg, rule):
    reads, row0 = RULES[rule]
    results = []
    for layout in LAYOUTS:
        clean, poisoned = _pair(layout, reads, row0)
        got = _device(opt, rule, layout, clean)
        assert _same(_device(opt, rule, layout, poisoned), got), (rule, layout, "poisoned against clean")
        host = _host(rule, layout, clean, cfg)
        print(rule, layout, {k: (np.asarray(got[k], np.float64) - np.asarray(host[k], np.float64)).tolist() for k in got
                             if not _same(got[k], host[k])})
        assert _same(got, host), (rule, layout, "against the host call")
        results.append(_shared(rule, got))
    assert _same(results[1], results[0]) and _same(results[2], results[0]), (rule, "between the layouts")
    if rule == "collisions":
        assert (results[0]["first_hit"] >= 0).any() and (results[0]["first_hit"] < 0).any()   # the scene decides something
    if rule == "carry":
        assert (results[0]["state"] == 0).all()


@pytest.mark.gpu
def test_warm_rows_read_the_two_controls_and_no_others(built):
    """stage_load with warm rows + init guess: U is the rows' control columns whatever else the rows hold, in every layout"""
    sc = scenario.generate("mix11", B, seed=12)
    N = sc["n_steps"]
    k = np.arange(N + 1, dtype=np.float64)
    jerk = 0.125 * np.cos(k)[None, :] + 0.25 * np.arange(B)[:, None]
    rate = 0.015625 * np.sin(k)[None, :] - 0.0078125 * np.arange(B)[:, None]
    got = []
    with api.BatchIlqrOptimizer(n_steps=N, batch_capacity=B, cmax=sc["cmax"]) as o:
        for layout, width, cols in ((api.ROWS_TRAJ, 10, (8, 9)), (api.ROWS_PLAN, 11, (9, 10)), (api.ROWS_CONTROLS, 2, (0, 1))):
            n_rows = N if layout == api.ROWS_CONTROLS else N + 1
            for fill in (7.0, np.nan):
                rows = np.full((B, n_rows, width), fill)
                rows[:, :, cols[0]], rows[:, :, cols[1]] = jerk[:, :n_rows], rate[:, :n_rows]
                o.stage_load(sc, warm=(rows, None, layout))
                o.stage_init_guess()
                got.append(o.read(api.T_U))
    want = np.stack([jerk[:, :N], rate[:, :N]], axis=2)
    for u in got:
        assert same_rows(u, want)


@pytest.mark.gpu
def test_resample_writes_the_same_values_in_every_layout(opt):
    """(b): every column is written, so the layouts are held to each other, and to the host call"""
    f = _fields()
    t = f["time"][0]
    # before the first key, on a knot, between knots, inside the equal pair, past the last
    by_time = np.array([-0.25, 0.5, 0.75, 1.0, 1.25, 2.0, 2.5])
    assert len(by_time) == M and t[2] == t[3]
    out = {}
    for layout in LAYOUTS:
        rows = _rows(layout)
        out[layout] = opt.resample(rows, layout, by_time, api.KEY_TIME)
        host = np.stack([api.resample_rows(rows[b], layout, by_time, api.KEY_TIME) for b in range(B)])
        assert same_rows(out[layout], host), layout
    for layout in (api.ROWS_PLAN, api.ROWS_COARSE):
        for name, c in COLUMNS[layout].items():
            if name in COLUMNS[api.ROWS_TRAJ]:
                assert same_rows(out[layout][..., c], out[api.ROWS_TRAJ][..., COLUMNS[api.ROWS_TRAJ][name]]), (layout, name)
    assert same_rows(out[api.ROWS_COARSE], out[api.ROWS_PLAN][..., :9])
    assert same_rows(out[api.ROWS_TRAJ][:, 2, 7], 0.5 * (f["kappa"][:, 1] + f["kappa"][:, 2]))    # kappa is linear ...
    assert same_rows(out[api.ROWS_TRAJ][:, 2, 8:10], np.stack([f["jerk"][:, 1], f["rate"][:, 1]], axis=1))   # ... a control holds
    by_station = np.array([-0.5, 1.0, 1.5, 2.125, 2.25, 4.0, 4.5])
    plan = opt.resample(_rows(api.ROWS_PLAN), api.ROWS_PLAN, by_station, api.KEY_STATION)
    coarse = opt.resample(_rows(api.ROWS_COARSE), api.ROWS_COARSE, by_station, api.KEY_STATION)
    assert same_rows(coarse, plan[..., :9])
    host = np.stack([api.resample_rows(_rows(api.ROWS_PLAN)[b], api.ROWS_PLAN, by_station, api.KEY_STATION) for b in range(B)])
    assert same_rows(plan, host)
    assert same_rows(plan[:, 2, 6], 0.5 * (f["v"][:, 1] + f["v"][:, 2]))   # v, not a, half way between rows 1 and 2
