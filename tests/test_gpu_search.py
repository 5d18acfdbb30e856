"""What follows the five stages of an iteration -- the acceptance test (cc:252-261; four copies: k_search_round, k_spec_pick,
k_round_pick of kernels_search.hip and the pick loop of kernels_tail.hip), the four line-search schedules with their pending
lists, and update_state (search_core.hpp: the lambda / dlambda schedule and every exit) -- held to the statement of
tests/search_reference.py, BIT FOR BIT, on the table of tests/search_cases.py.

The search state of a solve is chosen through the test door cilqr_set_search_seed (cost_old, lambda, dlambda, iteration count),
its first iterate through a warm start.  For every iterate of the table the DEVICE'S OWN eleven candidate totals, delta_V_ and
gradient norm come from the stage doors (held at 1e-9 and bit for bit across forms by test_gpu_stages.py / test_gpu_riccati.py);
the seeds are then laid around every threshold as adjacent doubles with opposite verdicts under the statement.

PREMISE (test_premise_...): wherever a seeded solve accepts, its recorded cost row is the stage door's five columns for that step
size and its next iterate the stage door's candidate, bit for bit -- on every schedule.  Measured figures: DESIGN.md, section 5.

One-iteration solves (iter = max_iter - 1) of the whole table run through every path of PATHS; three-iteration chains
(iter = max_iter - 3) make lambda' and dlambda' visible: a numpy loop over the stage doors and the statement's decisions
reproduces them.  The tables: iterates harvested from zero-tolerance solves at N = 7 and N = 50, the crafted N = 7 table of
stage_cases.py as warm controls, and the N = 7 table under abs_cost_tol = 2^-6 (dcost exactly on the tolerance).  A census is
asserted per path (MIN_PER_BRANCH, MIN_FLIPS; the CPU table of tests/test_search_reference.py must have twice as much): its
branch counters name the branches on which the path was held to the statement, its flip counts come from the device's outputs."""
import numpy as np
import pytest

import search_cases as cs
import search_reference as sr
from parity_util import oracle_cfg_from
from cilqr_amd import api
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
MIN_PER_BRANCH, MIN_FLIPS = 1, 1
SCENES = {7: 12, 50: 8}
TAGGED_ROWS = 16
DYADIC = 2.0 ** -6
SEED = 5100
REPLAY_TOL = 1e-8        # the project's replay rule (parity_util.STEP_TOL)

S, Q, G, T, C, F = api.OPT_SPEC_THRESHOLD, api.OPT_SEQ_ROUNDS, api.OPT_ROUND_GROUP, api.OPT_TAIL_THRESHOLD, api.OPT_COMPACTION, \
    api.OPT_FINISH_THRESHOLD
PATHS = {"defaults": {}, "round by round": {S: 0, Q: 11, T: 0}, "open speculative": {S: 8192, T: 0}, "tail 8192": {T: 8192},
         "tail 0": {T: 0}, "compaction off": {C: 0, T: 0, S: 0}, "compaction on": {C: 1, T: 0, S: 0},
         "finish 0": {F: 0, T: 0}, "finish 3000": {F: 3000, T: 0}}
PATHS.update({f"rounds {r} group {g}": {S: 0, Q: r, G: g, T: 0} for r in (1, 2, 4, 5, 6) for g in (1, 2, 4)})
CHAIN_PATHS = ("defaults", "open speculative", "round by round", "rounds 4 group 2", "rounds 5 group 4", "compaction off", "finish 3000")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _handle(cfg, capacity, cmax, options=None):
    opt = api.BatchIlqrOptimizer(cfg, batch_capacity=capacity, cmax=cmax)
    for k, v in (options or {}).items():
        opt.set_option(k, v)
    return opt


# ---------------------------------------------------------------------------------------------
# the table, from the device's own stage results
# ---------------------------------------------------------------------------------------------
_TABLES = {}


def _rows(key):
    """(n_steps, scene, U) of a table's rows: iterates harvested from zero-tolerance solves on the device (key 7, 50), or the
    N = 7 table of stage_cases.py with its controls as warm controls ("crafted")"""
    if key == "crafted":
        scene, U = cs.crafted_rows()
        return cs.CRAFTED_N, scene, U
    n_scenes = SCENES[key]
    scene = cs.zero_tolerance_scene(key, n_scenes, SEED + key)
    zero = api.default_config(key, abs_cost_tol=0.0, rel_cost_tol=0.0)
    with _handle(zero, n_scenes, scene["cmax"]) as opt:
        g = opt.plan(scene, max_iter_trajs=zero.max_iter + 1)
    U = np.concatenate([cs.pick_iterates(g["iter_trajs"][b], g["n_iter_trajs"][b], g["traj"][b], key) for b in range(n_scenes)])
    return key, cs.take_rows(scene, np.repeat(np.arange(n_scenes), 4)), U


def table(key):
    """key 7, 50, "crafted": a table laid on the device's stage results; "dyadic": the N = 7 table's stage results under
    abs_cost_tol = 2^-6, the cases around and exactly on that tolerance"""
    if key not in _TABLES:
        if key == "dyadic":
            base = table(7)
            cfg = api.default_config(7, abs_cost_tol=DYADIC)
            tol = dict(base["tol"], abs=DYADIC)
            scene_e, stage, entries = base["scene"], base["stage"], base["entries"]
            cases = [c for c in cs.lay_table(stage, entries, tol) if c.threshold == "abs_cost_tol" or c.kind == "dcost == abs_cost_tol"]
        else:
            n_steps, scene, U = _rows(key)
            cfg = api.default_config(n_steps)
            tol = dict(abs=cfg.abs_cost_tol, rel=cfg.rel_cost_tol, max_iter=cfg.max_iter)
            entries = cs.entries_for(U.shape[0], tagged_rows=TAGGED_ROWS)
            rows = [e[0] for e in entries]
            scene_e, U_e = cs.take_rows(scene, rows), np.ascontiguousarray(U[rows])
            with _handle(cfg, len(entries), scene["cmax"]) as a, _handle(cfg, len(entries), scene["cmax"]) as b:
                stage = cs.device_stage(a, b, scene_e, None, U_e, np.array([e[1] for e in entries]))
            cases = cs.lay_table(stage, entries, tol)
        results, census = cs.run_statement(cases, stage, tol)
        _TABLES[key] = dict(cfg=cfg, tol=tol, scene=scene_e, stage=stage, entries=entries, cases=cases, results=results, census=census,
                            batches=_batches(len(cases)))
        print(f"[table {key}] {len(entries)} entries, {len(cases)} cases; {census.report()}")
    return _TABLES[key]


def _batches(n):
    """index ranges of the cases: batches of 1, 9, 65 and 257 first, 300 from there on"""
    out, at = [], 0
    for B in cs.BATCHES[:-1]:
        if at < n:
            out.append((at, min(n, at + B)))
            at = out[-1][1]
    while at < n:
        out.append((at, min(n, at + cs.BATCHES[-1])))
        at = out[-1][1]
    return out


def _expected(t, lo, hi):
    """the statement's one-iteration result of cases lo .. hi - 1 as arrays"""
    stage, M = t["stage"], t["cfg"].max_iter
    cases, results = t["cases"][lo:hi], t["results"][lo:hi]
    e = np.array([c.entry for c in cases])
    idx = np.array([s["index"] for s in results])
    acc = idx >= 0
    X, U = stage["X"][e].copy(), stage["U"][e].copy()
    X[acc], U[acc] = stage["Xc"][e[acc], idx[acc]], stage["Uc"][e[acc], idx[acc]]
    row1 = np.zeros((len(cases), 5))
    row1[acc] = stage["totals"][e[acc], idx[acc]]
    return dict(e=e, index=idx, status=np.array([s["status"] for s in results]), n_cost=1 + acc.astype(int),
                n_iter=np.full(len(cases), M), n_iter_trajs=1 + np.array([int(s["emits"]) for s in results]),
                row0=stage["cost0"][e], row1=row1, X=X, U=U, X0=stage["X"][e], U0=stage["U"][e])


def _solve(opt, t, lo, hi, n_back=1, cost_old=None):
    cases, M = t["cases"][lo:hi], t["cfg"].max_iter
    e = [c.entry for c in cases]
    seed = dict(cost_old=np.array([c.cost_old for c in cases]) if cost_old is None else cost_old, lam=np.array([c.lam for c in cases]),
                dlam=np.array([c.dlam for c in cases]), iter=np.full(len(cases), M - n_back, np.int32))
    return opt.plan(cs.take_rows(t["scene"], e), max_iter_trajs=n_back + 1, alpha_trace=True,
                    warm=(np.ascontiguousarray(t["stage"]["U"][e]), None, api.ROWS_CONTROLS), seed=seed)


def _hold_batch(g, x, what, M):
    """a one-iteration solve against the statement, bit for bit"""
    at = g["alpha_trace"]
    assert np.array_equal(at[:, M - 1], x["index"]), (what, "accepted index", np.flatnonzero(at[:, M - 1] != x["index"])[:8])
    assert (at[:, :M - 1] == -3).all(), (what, "alpha_trace below the seeded iteration")
    for k in ("status", "n_cost", "n_iter", "n_iter_trajs"):
        assert np.array_equal(g[k], x[k]), (what, k, np.flatnonzero(g[k] != x[k])[:8], g[k][g[k] != x[k]][:8], x[k][g[k] != x[k]][:8])
    assert np.array_equal(_bits(g["cost_hist"][:, 0]), _bits(x["row0"])), (what, "cost row 0 is not the first iterate's true cost")
    assert np.array_equal(_bits(g["cost_hist"][:, 1]), _bits(x["row1"])), (what, "recorded cost row")
    assert not g["cost_hist"][:, 2:].any(), (what, "cost rows beyond n_cost")
    assert np.array_equal(_bits(g["traj"][:, :, 1:7]), _bits(x["X"])) and np.array_equal(_bits(g["traj"][:, :-1, 8:10]), _bits(x["U"])), \
        (what, "trajectory")
    assert np.array_equal(_bits(g["iter_trajs"][:, 0, :, 1:7]), _bits(x["X0"])), (what, "first iterate")
    emits = x["n_iter_trajs"] == 2
    assert np.array_equal(_bits(g["iter_trajs"][emits, 1, :, 1:7]), _bits(x["X"][emits])), (what, "recorded next iterate")


def _device_census(t, outs):
    """The census of one path (outs: its solves, batch by batch).  The branch counters are the statement's, counted for the cases
    in which the device returned the statement's accepted index and status (all of them once _hold_batch has passed: they say
    which branches this path was HELD on, they are not a second measurement); the flip counts come from the device's own
    outputs."""
    M = t["cfg"].max_iter
    idx = np.concatenate([g["alpha_trace"][:, M - 1] for g in outs])
    status = np.concatenate([g["status"] for g in outs])
    rows = np.concatenate([g["cost_hist"][:, 1] for g in outs])
    census = sr.Census()
    for c, s, i, st in zip(t["cases"], t["results"], idx, status):
        if (i, st) == (s["index"], s["status"]):          # the device took the statement's branches: count them as its own
            census.add(s)
    dev = [dict(index=int(i), status=int(st), lam=s["lam"], dlam=s["dlam"], row=None if i < 0 else list(r))
           for i, st, r, s in zip(idx, status, rows, t["results"])]
    cs.count_flips(t["cases"], dev, census)
    return census


ONE_ITERATION_THRESHOLDS = ("z=1e-4", "z=10", "abs_cost_tol", "rel_cost_tol", "lam<1e-5", "lam*ndl>1e11")


def _run_path(n_steps, path):
    t = table(n_steps)
    M = t["cfg"].max_iter
    outs = []
    with _handle(t["cfg"], cs.BIG_CAPACITY, t["scene"]["cmax"], PATHS[path]) as opt:
        for lo, hi in t["batches"]:
            g = _solve(opt, t, lo, hi)
            _hold_batch(g, _expected(t, lo, hi), (n_steps, path, lo, hi), M)
            outs.append(g)
    return t, outs


@pytest.mark.parametrize("path", list(PATHS))
def test_one_iteration_solves_follow_the_statement(path):
    """N = 7 (K = 8: a multiple of k_multi_copy's four knots per thread), the whole table, batches of 1, 9, 65, 257 and 300 on a
    handle of capacity 320; the census of this path complete."""
    t, outs = _run_path(7, path)
    census = _device_census(t, outs)
    print(f"[N = 7, {path}] {census.report()}")
    assert census.missing(MIN_PER_BRANCH) == [], (path, census.report())
    short = [th for th in ONE_ITERATION_THRESHOLDS if census.flips.get(th, 0) < MIN_FLIPS]
    assert short == [], (path, census.report())
    for b, n in t["census"].branches.items():
        assert n >= 2 * MIN_PER_BRANCH, ("the table itself is short of", b)


@pytest.mark.parametrize("path", ["defaults", "round by round", "open speculative", "rounds 4 group 2", "rounds 6 group 4", "rounds 5 group 1"])
def test_one_iteration_solves_at_the_product_horizon(path):
    """N = 50 (K = 51: not a multiple of k_multi_copy's four knots), eight scenes' iterates: the agreement; a first accept at
    every step size, so that the winner's copy runs for the late ones at this shape; the cost-side thresholds flip"""
    t, outs = _run_path(50, path)
    census = _device_census(t, outs)
    print(f"[N = 50, {path}] {census.report()}")
    assert all(census.branches[f"accept {r}"] >= MIN_PER_BRANCH for r in range(11)) and census.branches["accept none"], census.report()
    short = [th for th in ("z=1e-4", "z=10", "abs_cost_tol", "rel_cost_tol") if census.flips.get(th, 0) < MIN_FLIPS]
    assert short == [], (path, census.report())


@pytest.mark.parametrize("path", list(PATHS))
def test_one_iteration_solves_from_the_crafted_table(path):
    """The iterates test_gpu_stages.py holds the cost and quadratise kernels on (barrier arguments on the edge, half-filled plane
    chunks, far planes, unwrapped headings), as warm controls, with the table's own corridors and lane table: the search, pick
    and copy kernels see them on every path"""
    t, outs = _run_path("crafted", path)
    census = _device_census(t, outs)
    print(f"[crafted, {path}] {census.report()}")
    assert all(census.branches[f"accept {r}"] >= MIN_PER_BRANCH for r in range(11)) and census.branches["accept none"], census.report()
    for b in ("reject z<=1e-4", "reject z>=10", "reject dcost<=0", "reject z nan", "exit abs", "exit rel", "exit max_iter"):
        assert census.branches[b] >= MIN_PER_BRANCH, (path, b, census.report())
    short = [th for th in ("z=1e-4", "z=10", "abs_cost_tol", "rel_cost_tol") if census.flips.get(th, 0) < MIN_FLIPS]
    assert short == [], (path, census.report())


@pytest.mark.parametrize("path", list(PATHS))
def test_dcost_exactly_on_a_dyadic_tolerance(path):
    """abs_cost_tol = 2^-6 on the handle: tot + 2^-6 is exact, so dcost == abs_cost_tol in bits -- the exit is `<`: the solve goes
    on (status max_iter, the iterate recorded) -- with the adjacent doubles on either side.  An adjacent pair alone cannot tell
    `<` from `<=`; the case exactly on the tolerance does."""
    t, outs = _run_path("dyadic", path)
    M = t["cfg"].max_iter
    status = np.concatenate([g["status"] for g in outs])
    index = np.concatenate([g["alpha_trace"][:, M - 1] for g in outs])
    n_it = np.concatenate([g["n_iter_trajs"] for g in outs])
    exact = np.array([c.kind == "dcost == abs_cost_tol" for c in t["cases"]])
    e = np.array([c.entry for c in t["cases"]])
    dcost = np.array([c.cost_old for c in t["cases"]]) - t["stage"]["totals"][e, np.maximum(index, 0), 0]
    on_it = exact & (index >= 0) & (dcost == DYADIC)
    census = _device_census(t, outs)
    print(f"[dyadic, {path}] {len(t['cases'])} cases, {int(on_it.sum())} with dcost == 2^-6 in bits; flips {census.flips}")
    assert on_it.sum() >= MIN_PER_BRANCH, path
    # (with dcost on the tolerance the absolute test is false; whether the relative one then ends the solve is the case's own)
    assert (status[on_it] != sr.ST_ABS).all() and np.isin(status[on_it], (sr.ST_REL, sr.ST_MAX_ITER)).all(), (path, status[on_it][:8])
    assert ((status[on_it] == sr.ST_MAX_ITER) == (n_it[on_it] == 2)).all(), path
    assert census.flips.get("abs_cost_tol", 0) >= MIN_FLIPS, (path, census.flips)


def test_every_path_gives_the_same_bits():
    """(each path equals the statement above; here directly, on the batch of 300 that holds the late step sizes)"""
    t = table(7)
    lo, hi = max(t["batches"], key=lambda b: (b[1] - b[0], len({s["index"] for s in t["results"][b[0]:b[1]]})))
    ref = None
    for path, options in PATHS.items():
        with _handle(t["cfg"], cs.BIG_CAPACITY, t["scene"]["cmax"], options) as opt:
            g = _solve(opt, t, lo, hi)
        if ref is None:
            ref = g
        for k in ("traj", "cost_hist", "iter_trajs"):
            assert np.array_equal(_bits(g[k]), _bits(ref[k])), (path, k)
        for k in ("status", "n_cost", "n_iter", "n_iter_trajs", "alpha_trace"):
            assert np.array_equal(g[k], ref[k]), (path, k)


@pytest.mark.parametrize("path", ["defaults", "open speculative", "round by round", "rounds 4 group 2"])
def test_premise_an_accepted_row_is_the_stage_doors_row(path):
    """Stands on its own: over the SOLID accepted cases (far from every threshold, so that the verdict is not in question) the
    cost row a solve records is cilqr_stage_total_cost of the stage door's candidate, and its next iterate is that candidate."""
    t = table(7)
    pick = [i for i, (c, s) in enumerate(zip(t["cases"], t["results"])) if c.kind == "solid accept"][:300]
    sub = dict(t, cases=[t["cases"][i] for i in pick], results=[t["results"][i] for i in pick])
    x = _expected(sub, 0, len(pick))
    with _handle(t["cfg"], cs.BIG_CAPACITY, t["scene"]["cmax"], PATHS[path]) as opt:
        g = _solve(opt, sub, 0, len(pick))
    M = t["cfg"].max_iter
    assert np.array_equal(g["alpha_trace"][:, M - 1], x["index"]), (path, "a solid case was decided otherwise")
    d_row = np.abs(g["cost_hist"][:, 1] - x["row1"]).max()
    d_x = np.abs(g["traj"][:, :, 1:7] - x["X"]).max()
    print(f"[premise, {path}] {len(pick)} accepted solves: largest distance of the recorded row {d_row:.3e}, of the next iterate {d_x:.3e}")
    assert np.array_equal(_bits(g["cost_hist"][:, 1]), _bits(x["row1"])), (path, "cost row", d_row)
    assert np.array_equal(_bits(g["traj"][:, :, 1:7]), _bits(x["X"])), (path, "next iterate", d_x)


# ---------------------------------------------------------------------------------------------
# three-iteration chains: lambda' and dlambda' become visible
# ---------------------------------------------------------------------------------------------
_CHAINS = {}


def chains():
    """The lambda-side cases of the N = 7 table, three iterations each: the numpy loop over the stage doors and the statement."""
    if "x" not in _CHAINS:
        t = table(7)
        cases = [c for c in t["cases"] if c.lambda_side]
        scene = cs.take_rows(t["scene"], [c.entry for c in cases])
        with _handle(t["cfg"], len(cases), t["scene"]["cmax"]) as a, _handle(t["cfg"], len(cases), t["scene"]["cmax"]) as b:
            x, census = cs.run_chains(cases, t["stage"], lambda X, U, lam: cs.device_stage(a, b, scene, X, U, lam), t["tol"])
        _CHAINS["x"] = (t, cases, x, census)
        print(f"[chains] {len(cases)} cases; {census.report()}; pairs that end in different bits: {cs.chain_flips(cases, x)}")
    return _CHAINS["x"]


@pytest.mark.parametrize("path", CHAIN_PATHS)
def test_three_iteration_chains_follow_the_statement(path):
    t, cases, x, _ = chains()
    n, M = len(cases), t["cfg"].max_iter
    sub = dict(t, cases=cases)
    got = []
    with _handle(t["cfg"], cs.BIG_CAPACITY, t["scene"]["cmax"], PATHS[path]) as opt:
        for lo in range(0, n, 300):
            got.append(_solve(opt, sub, lo, min(n, lo + 300), n_back=3))
    g = {k: np.concatenate([o[k] for o in got]) for k in ("alpha_trace", "status", "n_cost", "n_iter", "n_iter_trajs", "cost_hist", "traj", "iter_trajs")}
    assert np.array_equal(g["alpha_trace"][:, M - 3:], x["trace"]), (path, np.flatnonzero((g["alpha_trace"][:, M - 3:] != x["trace"]).any(1))[:8])
    for k in ("status", "n_cost", "n_iter", "n_iter_trajs"):
        assert np.array_equal(g[k], x[k]), (path, k, np.flatnonzero(g[k] != x[k])[:8])
    assert np.array_equal(_bits(g["cost_hist"][:, 1:4]), _bits(x["rows"])), (path, "cost rows")
    assert np.array_equal(_bits(g["traj"][:, :, 1:7]), _bits(x["X"])) and np.array_equal(_bits(g["traj"][:, :-1, 8:10]), _bits(x["U"])), (path, "trajectory")
    for k in range(4):
        have = x["n_iter_trajs"] > k
        assert np.array_equal(_bits(g["iter_trajs"][have, k, :, 1:7]), _bits(x["its"][have, k])), (path, "iterate", k)
    # the lambda-side pairs: only those whose two branches end in different bits under the statement count, and the device
    # shows the same difference
    dev = dict(trace=g["alpha_trace"][:, M - 3:], status=g["status"], n_cost=g["n_cost"], rows=g["cost_hist"][:, 1:4], X=g["traj"][:, :, 1:7])
    want, flips = cs.chain_flips(cases, x), cs.chain_flips(cases, dev)
    print(f"[chains, {path}] pairs whose branches end in different bits: {flips}")
    assert flips == want, (path, flips, want)
    for th in ("fmin(dl/1.6, 1/1.6)", "fmax(dl*1.6, 1.6)", "lam>1e-8", "lam*ndl>1e11"):
        assert flips.get(th, 0) >= MIN_FLIPS, (path, th, flips)


# ---------------------------------------------------------------------------------------------
# pending lists once the active list is no longer the identity
# ---------------------------------------------------------------------------------------------
THINNED_PATHS = ("rounds 1 group 1", "rounds 1 group 4", "rounds 2 group 1", "rounds 2 group 2", "rounds 4 group 2", "rounds 6 group 4",
                 "round by round", "open speculative", "defaults", "compaction off")
_THINNED = {}


def thinned():
    if "x" not in _THINNED:
        t = table(7)
        two = [c for c in t["cases"] if c.two_step]
        fin = [c for c, s in zip(t["cases"], t["results"]) if s["status"] in (sr.ST_ABS, sr.ST_REL, sr.ST_GNORM) and not c.two_step]
        cases = [c for pair in zip(fin, two) for c in pair][:300]        # a problem that leaves in front of each one that stays
        scene = cs.take_rows(t["scene"], [c.entry for c in cases])
        with _handle(t["cfg"], len(cases), t["scene"]["cmax"]) as a, _handle(t["cfg"], len(cases), t["scene"]["cmax"]) as b:
            x, census = cs.run_chains(cases, t["stage"], lambda X, U, lam: cs.device_stage(a, b, scene, X, U, lam), t["tol"], n_back=2)
        _THINNED["x"] = (t, cases, x)
        late = x["trace"][[c.two_step for c in cases], 1]
        print(f"[thinned] {len(cases)} cases, {len(two)} two-step seeds in the table; second-iteration indices of those that stay: "
              f"{dict(zip(*np.unique(late, return_counts=True)))}")
    return _THINNED["x"]


@pytest.mark.parametrize("path", THINNED_PATHS)
def test_pending_lists_after_problems_have_left(path):
    """In a solve's first iteration the active list is the identity and a list position equals its slot, so one-iteration solves
    cannot tell a pending list of positions from one of slots.  Two iterations (iter = max_iter - 2), every other problem leaving
    in the first (a converged or gradient-norm exit), the ones between them rejecting every step size at lambda = 2^-20 and -- the
    same iterate at lambda' = 1 exactly -- first accepting a LATER step size in the second, when positions and slots differ."""
    t, cases, x = thinned()
    M = t["cfg"].max_iter
    stay = np.array([c.two_step for c in cases])
    assert (x["trace"][stay, 0] == -1).all() and (x["n_iter"][~stay] == M - 1).all()
    for r in (1, 2):
        assert (x["trace"][stay, 1] >= r).sum() >= MIN_PER_BRANCH, ("no first accept at or beyond step size", r, "in the second iteration")
    with _handle(t["cfg"], cs.BIG_CAPACITY, t["scene"]["cmax"], PATHS[path]) as opt:
        g = _solve(opt, dict(t, cases=cases), 0, len(cases), n_back=2)
    assert np.array_equal(g["alpha_trace"][:, M - 2:], x["trace"]), (path, np.flatnonzero((g["alpha_trace"][:, M - 2:] != x["trace"]).any(1))[:8])
    for k in ("status", "n_cost", "n_iter", "n_iter_trajs"):
        assert np.array_equal(g[k], x[k]), (path, k, np.flatnonzero(g[k] != x[k])[:8])
    assert np.array_equal(_bits(g["cost_hist"][:, 1:3]), _bits(x["rows"])), (path, "cost rows")
    assert np.array_equal(_bits(g["traj"][:, :, 1:7]), _bits(x["X"])), (path, "trajectory")


# ---------------------------------------------------------------------------------------------
# hostile seeds stay inside their problem
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["defaults", "open speculative", "rounds 4 group 2", "round by round"])
@pytest.mark.parametrize("B", [9, 65])
def test_hostile_seeds_stay_inside_their_problem(path, B):
    """cost_old = NaN, +Inf, -Inf at slots 3 and B - 1: every other problem keeps the bits of the run without them, the spoiled
    ones follow the statement (NaN: every step size rejected by z = NaN; +Inf: by z >= 10; -Inf: by z <= 1e-4)"""
    t = table(7)
    pick = [i for i, c in enumerate(t["cases"]) if c.kind == "solid accept"][:B]
    sub = dict(t, cases=[t["cases"][i] for i in pick], results=[t["results"][i] for i in pick])
    M = t["cfg"].max_iter
    with _handle(t["cfg"], cs.BIG_CAPACITY, t["scene"]["cmax"], PATHS[path]) as opt:
        clean = _solve(opt, sub, 0, B)
        others = np.ones(B, bool)
        others[[3, B - 1]] = False
        for bad in (np.nan, np.inf, -np.inf):
            c = np.array([k.cost_old for k in sub["cases"]])
            c[[3, B - 1]] = bad
            g = _solve(opt, sub, 0, B, cost_old=c)
            for k in ("traj", "cost_hist", "iter_trajs"):
                assert np.array_equal(_bits(g[k][others]), _bits(clean[k][others])), (path, bad, k, "a neighbour changed")
            for k in ("status", "n_cost", "n_iter", "alpha_trace"):
                assert np.array_equal(g[k][others], clean[k][others]), (path, bad, k, "a neighbour changed")
            for b in (3, B - 1):
                k = sub["cases"][b]
                e = k.entry
                s = sr.step(t["stage"]["totals"][e], t["stage"]["dV"][e], t["stage"]["gnorm"][e], bad, k.lam, k.dlam, M - 1,
                            t["tol"]["abs"], t["tol"]["rel"], M)
                assert s["index"] == sr.NONE
                assert g["alpha_trace"][b, M - 1] == -1 and g["status"][b] == s["status"] and g["n_cost"][b] == 1, (path, bad, b)
                assert np.array_equal(_bits(g["traj"][b, :, 1:7]), _bits(t["stage"]["X"][e])), (path, bad, b, "the iterate moved")


def test_the_door_checks_its_arguments_and_is_consumed_once():
    t = table(7)
    M = t["cfg"].max_iter
    sub = dict(t, cases=[c for c in t["cases"] if c.kind == "solid accept"][:9])
    with _handle(t["cfg"], 16, t["scene"]["cmax"]) as opt:
        for bad in (dict(iter=[-1] * 9), dict(iter=[M] * 9), dict(cost_old=np.zeros(17))):
            with pytest.raises(api.CilqrError) as err:
                opt.set_search_seed(bad)
            assert err.value.code == -6     # CILQR_ERR_ARG
        opt.set_search_seed(dict(cost_old=np.zeros(5)))                      # armed for a batch of 5: the batch of 9 refuses it
        e = [c.entry for c in sub["cases"]]
        assert opt.plan(cs.take_rows(t["scene"], e), check=False)["rc"] == -6
        seeded = _solve(opt, sub, 0, 9)
        plain = opt.plan(cs.take_rows(t["scene"], e), alpha_trace=True,
                         warm=(np.ascontiguousarray(t["stage"]["U"][e]), None, api.ROWS_CONTROLS))     # the seed is gone
        assert (seeded["n_iter"] == M).all() and (seeded["alpha_trace"][:, 0] == -3).all() and (plain["alpha_trace"][:, 0] != -3).all()
        # the same seed from device memory
        import torch
        c = sub["cases"]
        host = dict(cost_old=np.array([k.cost_old for k in c]), lam=np.array([k.lam for k in c]), dlam=np.array([k.dlam for k in c]),
                    iter=np.full(9, M - 1, np.int32))
        dev = {k: torch.tensor(v, device="cuda") for k, v in host.items()}
        from_dev = opt.plan(cs.take_rows(t["scene"], e), max_iter_trajs=2, alpha_trace=True,
                            warm=(np.ascontiguousarray(t["stage"]["U"][e]), None, api.ROWS_CONTROLS), seed=dev)
        for k in ("traj", "cost_hist", "iter_trajs"):
            assert np.array_equal(_bits(from_dev[k]), _bits(seeded[k])), k
        assert np.array_equal(from_dev["alpha_trace"], seeded["alpha_trace"]) and np.array_equal(from_dev["status"], seeded["status"])
        with pytest.raises(api.CilqrError):
            opt.set_search_seed(dict(iter=torch.full((9,), M, dtype=torch.int32, device="cuda")))
        # a plan() that raises before its solve leaves no seed behind
        with pytest.raises(Exception):
            opt.plan(cs.take_rows(t["scene"], e), warm=dict(rows=torch.zeros(3)), seed=host)
        after = opt.plan(cs.take_rows(t["scene"], e), alpha_trace=True,
                         warm=(np.ascontiguousarray(t["stage"]["U"][e]), None, api.ROWS_CONTROLS))
        assert np.array_equal(_bits(after["traj"]), _bits(plain["traj"]))
        # a batch with several lane groups refuses an armed seed, and disarms it
        grouped = dict(cs.take_rows(t["scene"], e))
        nl, nr = grouped["left"].shape[0], grouped["right"].shape[0]
        grouped.update(left=np.concatenate([grouped["left"]] * 2), right=np.concatenate([grouped["right"]] * 2),
                       lane_groups=[(0, nl, nr), (5, nl, nr)])
        opt.set_search_seed(host)
        assert opt.plan(grouped, check=False)["rc"] == -6
        assert (opt.plan(grouped, alpha_trace=True)["alpha_trace"][:, 0] != -3).all()
        opt.set_search_seed(dict(cost_old=np.full(9, np.nan)))
        opt.set_search_seed(None)                                            # disarmed
        again = opt.plan(cs.take_rows(t["scene"], e), alpha_trace=True,
                         warm=(np.ascontiguousarray(t["stage"]["U"][e]), None, api.ROWS_CONTROLS))
        assert np.array_equal(_bits(again["traj"]), _bits(plain["traj"])) and np.array_equal(again["alpha_trace"], plain["alpha_trace"])


# ---------------------------------------------------------------------------------------------
# against the oracle
# ---------------------------------------------------------------------------------------------
def test_solid_cases_against_the_seeded_oracle():
    """Only the cases whose statement margin is at least 1e-9 take part (the adjacent pairs are left out by construction):
    oracle_replay_seeded from the device's own iterate, at the project's replay rule of 1e-8."""
    t = table(7)
    M = t["cfg"].max_iter
    pick = [i for i, (c, s) in enumerate(zip(t["cases"], t["results"]))
            if s["margin"] >= cs.MARGIN_SOLID and np.isfinite(c.cost_old) and c.pair is None][:600]
    sub = dict(t, cases=[t["cases"][i] for i in pick], results=[t["results"][i] for i in pick])
    ocfg = oracle_cfg_from(t["cfg"])
    got = []
    with _handle(t["cfg"], cs.BIG_CAPACITY, t["scene"]["cmax"]) as opt:
        for lo in range(0, len(pick), 300):
            got.append(_solve(opt, sub, lo, min(len(pick), lo + 300)))
    g = {k: np.concatenate([o[k] for o in got]) for k in got[0] if isinstance(got[0][k], np.ndarray)}
    worst, excused = 0.0, 0
    for i, c in enumerate(sub["cases"]):
        e = c.entry
        o = orc.Oracle(ocfg)
        assert o.set_problem(t["scene"]["start"][e], t["scene"]["coarse"][e], t["scene"]["corridor"][e], t["scene"]["ccount"][e],
                             t["scene"]["left"], t["scene"]["right"]) == 0
        r = o.replay(t["stage"]["X"][e], t["stage"]["U"][e], c.lam, c.dlam, M - 1, cost_old=c.cost_old, to_the_end=True)
        if r["margins"].size and r["margins"][0] < 1e-9:      # the oracle's own decision sits on a threshold (rule 2(b))
            excused += 1
            continue
        assert int(r["decisions"][0]) == g["alpha_trace"][i, M - 1] and r["status"] == g["status"][i], (i, c, r["decisions"], r["status"])
        assert r["n_cost"] == g["n_cost"][i]
        d = np.abs(r["cost_hist"] - g["cost_hist"][i, :r["n_cost"]]) / np.maximum(np.abs(r["cost_hist"]), 1e-3)
        dx = np.abs(r["traj"][:, 1:7] - g["traj"][i, :, 1:7]).max() / max(1.0, np.abs(r["traj"][:, 1:7]).max())
        worst = max(worst, float(d.max()), float(dx))
        assert d.max() < REPLAY_TOL and dx < REPLAY_TOL, (i, c, d.max(), dx)
    print(f"[oracle] {len(pick)} solid cases of {len(t['cases'])} ({len(t['cases']) - len(pick)} left out), {excused} excused by the oracle's "
          f"own margin; worst distance {worst:.3e}")
    assert excused <= len(pick) // 50
