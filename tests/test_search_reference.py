"""The statement of tests/search_reference.py against the oracle (CPU only): fed the ORACLE'S own candidate totals, delta_V_ and
gradient norm -- through its forward, total_cost and backward stages -- it must reproduce oracle_replay_seeded EXACTLY on the
whole table of tests/search_cases.py: accepted index, status, the three counts, lambda', dlambda' and the recorded cost row,
bit for bit.  Both are restatements of cc:235-319 in doubles, written apart from each other; the table puts every decision on
its threshold, so a `>=` for a `>` or a wrong constant in either shows as a mismatch here.

The census of the table (every branch counter, every threshold's flipping pairs) must be complete, with at least twice what the
GPU tests ask per path (test_gpu_search.MIN_PER_BRANCH, MIN_FLIPS)."""
import numpy as np
import pytest

import search_cases as cs
import search_reference as sr
from oracle import oracle as orc

MIN_PER_BRANCH, MIN_FLIPS = 1, 1       # what tests/test_gpu_search.py asks of every path
N7_SCENES, N50_SCENES = 12, 8
TAGGED_ROWS = 16
SEED = 5100


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _oracle(ocfg, scene, b):
    o = orc.Oracle(ocfg)
    assert o.set_problem(scene["start"][b], scene["coarse"][b], scene["corridor"][b], scene["ccount"][b], scene["left"], scene["right"]) == 0
    return o


def harvest(n_steps, n_scenes):
    """rows = (scene, iterate): the first, middle and last iterate and the final trajectory of zero-tolerance oracle solves;
    n_steps "crafted": rows of the N = 7 table of stage_cases.py, their controls as warm controls"""
    if n_steps == "crafted":
        return cs.crafted_rows()
    scene = cs.zero_tolerance_scene(n_steps, n_scenes, SEED + n_steps)
    zero = orc.default_config(n_steps, abs_cost_tol=0.0, rel_cost_tol=0.0, max_iter=cs.ZERO_TOL_MAX_ITER)
    U = []
    for b in range(n_scenes):
        r = _oracle(zero, scene, b).plan(max_iter_trajs=cs.ZERO_TOL_MAX_ITER + 1)
        U.append(cs.pick_iterates(r["iter_trajs"], r["n_iter_trajs"], r["traj"], n_steps))
    rows = np.repeat(np.arange(n_scenes), 4)
    return cs.take_rows(scene, rows), np.concatenate(U)


_TABLES = {}


def table(n_steps, n_scenes, abs_tol=1e-2):
    key = (n_steps, n_scenes, abs_tol)
    if key not in _TABLES:
        scene, U = harvest(n_steps, n_scenes)
        ocfg = orc.default_config(cs.CRAFTED_N if n_steps == "crafted" else n_steps, abs_cost_tol=abs_tol)
        tol = dict(abs=ocfg.abs_cost_tol, rel=ocfg.rel_cost_tol, max_iter=ocfg.max_iter)
        entries = cs.entries_for(U.shape[0], tagged_rows=TAGGED_ROWS)
        rows = [e[0] for e in entries]
        scene_e, U_e = cs.take_rows(scene, rows), U[rows]
        stage = cs.oracle_stage(ocfg, scene_e, None, U_e, np.array([e[1] for e in entries]))
        cases = cs.lay_table(stage, entries, tol)
        if abs_tol != 1e-2:      # the dyadic tolerance serves its own threshold only
            cases = [c for c in cases if c.threshold == "abs_cost_tol" or c.kind == "dcost == abs_cost_tol"]
        _TABLES[key] = (ocfg, tol, scene_e, stage, cases)
    return _TABLES[key]


def _hold(n_steps, n_scenes, abs_tol=1e-2):
    ocfg, tol, scene, stage, cases = table(n_steps, n_scenes, abs_tol)
    results, census = cs.run_statement(cases, stage, tol)
    oracles = {}
    M = ocfg.max_iter
    for c, s in zip(cases, results):
        e = c.entry
        if e not in oracles:
            oracles[e] = _oracle(ocfg, scene, e)
        r = oracles[e].replay(stage["X"][e], stage["U"][e], c.lam, c.dlam, M - 1, cost_old=c.cost_old, to_the_end=True)
        what = (n_steps, c, s["index"], s["status"])
        assert int(r["decisions"][0]) == s["index"], what
        assert r["status"] == s["status"] and r["n_iter"] == s["it"] == M, (what, r["status"], r["n_iter"])
        assert r["n_cost"] == 1 + int(s["row"] is not None) and r["n_iter_trajs"] == 1 + int(s["emits"]), what
        assert np.array_equal(_bits([r["lam"], r["dlam"]]), _bits([s["lam"], s["dlam"]])), (what, r["lam"], r["dlam"], s["lam"], s["dlam"])
        assert np.array_equal(_bits(r["cost_hist"][0]), _bits(stage["cost0"][e])), what
        if s["row"] is not None:
            assert np.array_equal(_bits(r["cost_hist"][1]), _bits(s["row"])), what
            assert np.array_equal(_bits(r["traj"][:, 1:7]), _bits(stage["Xc"][e, s["index"]])), what
            assert np.array_equal(_bits(r["traj"][:-1, 8:10]), _bits(stage["Uc"][e, s["index"]])), what
    return cases, census


def test_statement_reproduces_the_seeded_oracle_n7():
    cases, census = _hold(7, N7_SCENES)
    print(f"N = 7: {len(cases)} cases; {census.report()}")
    assert census.missing(2 * MIN_PER_BRANCH) == [], census.report()
    short = [t for t in cs.THRESHOLDS if census.flips.get(t, 0) < 2 * MIN_FLIPS]
    assert short == [], census.report()


def test_statement_reproduces_the_seeded_oracle_on_the_crafted_table():
    """The iterates that test_gpu_stages.py holds the cost and quadratise kernels on -- barrier arguments on the edge, half-filled
    plane chunks, far planes, unwrapped headings -- as warm controls (the first iterate is their rollout from the start state)."""
    cases, census = _hold("crafted", 0)
    print(f"crafted: {len(cases)} cases; {census.report()}")
    assert census.branches["accept 0"] and census.branches["accept none"], census.report()
    short = [t for t in ("z=1e-4", "z=10", "abs_cost_tol", "rel_cost_tol") if census.flips.get(t, 0) < MIN_FLIPS]
    assert short == [], census.report()


def test_statement_reproduces_the_seeded_oracle_n50():
    """K = 51 knots, the horizon of the product, on eight scenes: the agreement, every accepted index, every threshold.  (No
    iterate of these scenes has a negative `expected` with z in range: the `dcost <= 0` clause is the N = 7 tables' to reach.)"""
    cases, census = _hold(50, N50_SCENES)
    print(f"N = 50: {len(cases)} cases; {census.report()}")
    assert all(census.branches[f"accept {r}"] for r in range(11)) and census.branches["accept none"], census.report()
    short = [t for t in cs.THRESHOLDS if t != "lam<1e-5" and census.flips.get(t, 0) < MIN_FLIPS]
    assert short == [], census.report()


def test_dcost_exactly_on_a_dyadic_tolerance():
    """abs_cost_tol = 2^-6: tot + 2^-6 is exact for totals below 2^46 ulps of it, so dcost == abs_cost_tol exactly -- the exit is
    `<`, the solve goes on -- with the adjacent pair around it"""
    cases, census = _hold(7, N7_SCENES, abs_tol=2.0 ** -6)
    exact = [c for c in cases if c.kind == "dcost == abs_cost_tol"]
    print(f"dyadic: {len(cases)} cases, {len(exact)} exactly on the tolerance; flips {census.flips}")
    assert len(exact) >= 2 and census.flips.get("abs_cost_tol", 0) >= 2


def test_three_iteration_chains_reproduce_the_seeded_oracle():
    """iter = max_iter - 3 on the lambda-side cases: lambda' and dlambda' act on the next backward pass, so the branches of the
    schedule show in the later rows.  The loop over the oracle's stages and the statement's decisions against ONE replay to the
    end: every accepted index, status, counts, cost rows, trajectory and the final (lambda, dlambda), bit for bit."""
    ocfg, tol, scene, stage, cases = table(7, N7_SCENES)
    cases = [c for c in cases if c.lambda_side]
    sub = cs.take_rows(scene, [c.entry for c in cases])
    x, census = cs.run_chains(cases, stage, lambda X, U, lam: cs.oracle_stage(ocfg, sub, X, U, lam), tol)
    M = ocfg.max_iter
    for i, c in enumerate(cases):
        r = _oracle(ocfg, scene, c.entry).replay(stage["X"][c.entry], stage["U"][c.entry], c.lam, c.dlam, M - 3, cost_old=c.cost_old,
                                               to_the_end=True)
        n = r["n_iter"] - (M - 3)
        assert list(r["decisions"]) == list(x["trace"][i, :n]) and (x["trace"][i, n:] == -3).all(), (c, r["decisions"], x["trace"][i])
        assert (r["status"], r["n_iter"], r["n_cost"], r["n_iter_trajs"]) == (x["status"][i], x["n_iter"][i], x["n_cost"][i], x["n_iter_trajs"][i]), c
        assert np.array_equal(_bits(r["cost_hist"][1:]), _bits(x["rows"][i, :r["n_cost"] - 1])), c
        assert np.array_equal(_bits(r["traj"][:, 1:7]), _bits(x["X"][i])), c
        assert np.array_equal(_bits([r["lam"], r["dlam"]]), _bits([x["lam"][i], x["dlam"][i]])), c
    flips = cs.chain_flips(cases, x)
    print(f"chains: {len(cases)} cases; pairs that end in different bits: {flips}; {census.report()}")
    for th in ("fmin(dl/1.6, 1/1.6)", "fmax(dl*1.6, 1.6)", "lam>1e-8", "lam*ndl>1e11"):
        assert flips.get(th, 0) >= MIN_FLIPS, (th, flips)


def test_census_counts_what_it_names():
    c = sr.Census()
    s = sr.step([[1.0] * 5] * 11, (-1.0, 0.0), 1.0, 1.5, 1.0, 1.0, 3, 1e-2, 1e-2, 200)
    assert s["index"] == 0 and s["status"] == sr.ST_RUNNING and s["row"] == [1.0] * 5 and s["cost_old"] == 1.0
    c.add(s)
    assert c.branches["accept 0"] == 1 and c.branches["lam > 1e-8: 1"] == 1 and len(c.missing()) == len(sr.BRANCHES) - 3
    s = sr.step([[1.0] * 5] * 11, (-1.0, 0.0), 1e-7, 1.5, 0.0, 1.0, 3, 1e-2, 1e-2, 200)
    assert s["index"] == sr.BEFORE and s["status"] == sr.ST_GNORM and s["it"] == 4


@pytest.mark.parametrize("a,b", [(1.0, 2.0), (-3.0, 5.0), (1e-8, 1e-5)])
def test_bisect_finds_adjacent_doubles(a, b):
    x, y = cs.bisect_flip(a, b, lambda v: v < (a + b) / 2)
    assert cs.nxt(x) == y and x < (a + b) / 2 <= y
