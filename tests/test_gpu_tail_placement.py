"""The tail kernel (kernels_tail.hip) at every placement of its working set.

`tail_plan` decides per launch which of a problem's 14 tensors live in the workgroup's LDS and which stay in the private
arena in global memory, and from that which form of every phase runs: tail_backward<true|false>, the three forms of
tail_forward, tail_quadratize / tail_knot_cost with LDS or generic addressing, the split quadratisation.  A flag that is
wrong for one tensor gives wrong numbers or a fault, not a slowdown -- and which placement a launch takes depends only on
the horizon, the plane capacity, the lane tables and the device's LDS grant, so the rest of the suite reaches a handful of
them.  CILQR_OPT_TAIL_LDS_LIMIT caps the LDS a launch plans with and CILQR_OPT_TAIL_PLAN reports what `tail_plan`
answers, so that every placement can be run here on small scenes.

The reference of every tail run is the lockstep loop (CILQR_OPT_TAIL_THRESHOLD 0) on the same handle, bit for bit; the
lockstep result of every scene set is held to the CPU oracle once (parity_util: whole solves at REL_TOL on the
oracle-stable problems, every step of every problem at STEP_TOL)."""
import dataclasses

import numpy as np
import pytest

from parity_util import KNIFE_EDGE, assert_parity, assert_steps, oracle_cfg_from, oracle_reference
from cilqr_amd import api, scenario

pytestmark = pytest.mark.gpu
ITER_CAP = 48
KEYS = ("traj", "cost_hist", "n_cost", "status", "n_iter", "iter_trajs", "n_iter_trajs", "alpha_trace")

# CILQR_OPT_TAIL_PLAN (include/cilqr.h): bit k = TENSORS[k] is in LDS; bits 16.. = FLAGS; 21 = split quadratisation; 24 = supported
TENSORS = ("X", "U", "goals", "cor", "ccnt", "lin", "term", "gains", "Xs", "Us", "parts", "spec_tot", "dbl", "ints")
PRIORITY = ("dbl", "ints", "spec_tot", "term", "gains", "X", "U", "lin", "parts", "Xs", "Us", "goals", "ccnt", "cor")   # order of placement
FLAGS = ("bwd", "fwd_src", "fwd", "quad", "cost")
SPLIT, SUPPORTED = 1 << 21, 1 << 24
ALL_IN = (1 << 14) - 1
# what each phase addresses as LDS when its flag is set (kernels_tail.hip: the comments of TailArgs)
PHASE_TENSORS = {"bwd": ("lin", "term", "gains", "U", "dbl"), "fwd_src": ("X", "U", "gains", "goals"),
                 "fwd": ("X", "U", "gains", "goals", "Xs", "Us"), "quad": ("X", "U", "goals", "cor", "ccnt", "lin", "term"),
                 "cost": ("Xs", "Us", "parts", "goals", "cor", "ccnt")}
LDS_MAX = 160 * 1024     # LDS of a gfx950 workgroup: no device grants more, and a limit above the grant changes nothing

# Set A: 24 dyn20x scenes cut to 20 steps, solved with both cost tolerances at 0 -- long solves with many rejected line
# searches (the recipe of test_four_row_candidate_arena_is_bit_identical), small enough that every tensor fits a fraction
# of the LDS.  dyn20x carries 24 planes per knot, and at that capacity the split quadratisation's scratch rows (1528 bytes
# per knot) never fit the candidates' rows they borrow (1224 bytes per knot): on set A `tail_plan` must never choose the
# split form, whatever the limit.  Set A16 is the same recipe with the generator keeping 16 planes per knot (1208 bytes of
# scratch per knot: the split form is chosen when everything is in LDS), so the two ladders together see both values of
# the split bit.  The seeds were chosen on the CPU from the oracle alone (oracle.solve_batch for the conditions of
# _assert_hard, oracle_reference for the unstable share); every share below is an oracle-only property and was the same
# with 40 perturbed re-runs as with the 8 that oracle_reference makes.
# With both tolerances at 0 these solves end in the rounding-noise plateau, where the oracle's own accept / reject tests sit
# 1e-15 (relative) from their thresholds: such a problem can pass eight perturbed re-runs and still be undecidable, so whole
# solves are compared only where, in addition, no decision of the oracle came within parity_util's KNIFE_EDGE = 1e-9 of its
# threshold -- the rule test_gpu_parity.py::test_exit_paths applies to its zero-tolerance case.  (The B = 70 set showed why:
# problem 9, "stable" in all 40 re-runs, spends its last fifteen iterations on decisions with margins of 1e-15 in the
# oracle, and the lockstep loop ends with one accepted step fewer.)  Both shares are given: unstable under oracle_reference
# alone / with that rule, which is the bound passed to assert_parity.  Every step of every problem is replayed at STEP_TOL
# whatever its class.
OVER_A = dict(max_iter=30, abs_cost_tol=0.0, rel_cost_tol=0.0)
SPEC_A = dataclasses.replace(scenario.SPECS["dyn20x"], n_steps=20)
SPEC_A16 = dataclasses.replace(SPEC_A, cmax=16)
SEED_A, UNSTABLE_A, UNSTABLE_A3 = 417, 12 / 24, 12 / 24   # set A: 1 / 12 of 24 with five discs, 1 / 12 of 24 with three
SEED_A16, UNSTABLE_A16 = 802, 9 / 24                      # set A16: 1 / 9 of 24
SEED_A70, UNSTABLE_A70 = 502, 46 / 70                     # the B = 70 set: 2 / 46 of 70
SEED_LANES, UNSTABLE_LANES = 604, 2 / 24                  # mix11 with 2 x 256 lane segments: 2 of 24
SEED_EDGE, UNSTABLE_EDGE = 701, 1 / 4                     # mix11 at N = 250, ~250 lane rows per side: 1 of 4
# Steps the oracle itself does not reproduce: with both tolerances at 0 the solves iterate on in the rounding-noise plateau,
# where the existing zero-tolerance tests allow 10 % excused steps (test_gpu_parity.py::test_exit_paths); the others keep
# assert_steps' own 2 % (5 % at the long horizon, as test_long_horizon_more_knots_than_a_tail_workgroup_has_threads).
EXCUSED_ZERO_TOL, EXCUSED_LONG = 0.10, 0.05


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _in(plan, name):
    return bool(plan >> TENSORS.index(name) & 1)


def _flag(plan, name):
    return bool(plan >> (16 + FLAGS.index(name)) & 1)


def _describe(plan):
    out = [t for t in PRIORITY if not _in(plan, t)]
    flags = [f for f in FLAGS if _flag(plan, f)] + (["split"] if plan & SPLIT else [])
    return f"mask {plan & ALL_IN:#06x} (out: {','.join(out) or '-'}) flags {','.join(flags) or '-'}"


def _handle(sc, max_lane_segments=64, **cfg_over):
    cfg = api.default_config(sc["n_steps"], **cfg_over)
    return api.BatchIlqrOptimizer(cfg, batch_capacity=sc["coarse"].shape[0], cmax=sc["cmax"], max_lane_segments=max_lane_segments)


def _plan_at(opt, limit):
    """(plan bits, dynamic LDS bytes) of the loaded problem under `limit` -- host calls only"""
    opt.set_option(api.OPT_TAIL_LDS_LIMIT, limit)
    return opt.get_option(api.OPT_TAIL_PLAN)


def _sweep(opt, sc):
    """Every limit from 0 to the largest LDS in 16-byte steps (every tensor's size is a multiple of 16 bytes, so no plan lies
    between two of them): {plan: (first limit that gives it, LDS bytes)} and the fixed block's size."""
    opt.stage_load(sc)
    plans = {}
    fixed = _plan_at(opt, 16)[1]             # nothing fits beside the fixed block and its margin: the launch takes that block alone
    for limit in range(0, LDS_MAX + 16, 16):
        plan, lds = _plan_at(opt, limit)
        # the LDS a launch takes never exceeds the limit in force plus the fixed block (which the limit does not touch)
        assert lds <= (limit or LDS_MAX) + fixed, (limit, lds, fixed)
        assert lds >= fixed and plan & SUPPORTED
        plans.setdefault(plan, (limit, lds))
    granted = _plan_at(opt, 0)
    assert _plan_at(opt, LDS_MAX) == granted == _plan_at(opt, 4 * LDS_MAX), "a limit at or above the grant must change nothing"
    opt.set_option(api.OPT_TAIL_LDS_LIMIT, 0)
    return plans, fixed


def _solve(opt, sc, limit, tail=True):
    """One solve in the tail kernel under `limit` (or in the lockstep loop); returns (outputs, problems the tail took)."""
    opt.set_option(api.OPT_TAIL_THRESHOLD, 1024 if tail else 0)
    opt.set_option(api.OPT_TAIL_LDS_LIMIT, limit)
    g = opt.plan(sc, max_iter_trajs=ITER_CAP, alpha_trace=True)
    return g, int(opt.profile().tail_problems)


def _live(g, k):
    """The specified part of output `k`: the live rows of cost_hist and the iterates that were produced."""
    a = g[k]
    if k == "cost_hist":
        return a[np.arange(a.shape[1])[None, :] < g["n_cost"][:, None]]
    if k == "iter_trajs":
        return a[np.arange(a.shape[1])[None, :] < np.minimum(g["n_iter_trajs"], a.shape[1])[:, None]]
    return a


def _assert_same(ref, got, what):
    for k in KEYS:
        a, b = _live(ref, k), _live(got, k)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, k)
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (what, k, "bytes")


def _anchor(opt, sc, max_unstable_frac, what, max_excused_frac=0.02, allow_lane_tie=False):
    """The lockstep result of a scene set, held to the oracle once: whole solves (not under the fast tie rule, which is
    allowed to leave the reference on a tie strip) and every step."""
    ref, took = _solve(opt, sc, 0, tail=False)
    assert took == 0
    ocfg = oracle_cfg_from(opt.cfg)
    rep = None
    if not allow_lane_tie:
        oref = oracle_reference(sc, ocfg)
        if opt.cfg.abs_cost_tol == 0.0 and opt.cfg.rel_cost_tol == 0.0:
            oref["stable"] &= oref["min_margin"] >= KNIFE_EDGE      # (see the comment on set A)
        rep = assert_parity(ref, oref, max_unstable_frac=max_unstable_frac, what=what)
    steps = assert_steps(ref, sc, ocfg, what=what, max_excused_frac=max_excused_frac, allow_lane_tie=allow_lane_tie)
    print(f"\n{what}: lockstep against the oracle: whole solves {rep}; steps {steps}")
    return ref


def _assert_hard(ref, what):
    """What makes set A say something about a tail: long solves, both later cost chunks, full rejections, several exits."""
    at = ref["alpha_trace"]
    assert ref["n_iter"].max() > 12, what
    assert (at >= 5).any() and (at == 10).any(), (what, "the cost chunks of step sizes 5..9 and 10 must both run")
    assert (at == -1).any(), (what, "no iteration rejects all eleven step sizes")
    assert len(set(ref["status"].tolist())) >= 2, (what, "one exit only")


SETS = {"A": (SPEC_A, SEED_A, UNSTABLE_A), "A16": (SPEC_A16, SEED_A16, UNSTABLE_A16)}


@pytest.fixture(scope="module")
def scenes():
    return {name: scenario.generate(spec, 24, seed=seed) for name, (spec, seed, _) in SETS.items()}


@pytest.fixture(scope="module", params=list(SETS))
def ladder(request, scenes):
    """Set A / A16 on its handle: the sweep's distinct plans and the anchored lockstep reference, shared by the tests below."""
    name, sc = request.param, scenes[request.param]
    opt = _handle(sc, **OVER_A)
    plans, fixed = _sweep(opt, sc)
    ref = _anchor(opt, sc, SETS[name][2], f"set {name}", max_excused_frac=EXCUSED_ZERO_TOL)
    _assert_hard(ref, f"set {name}")
    yield dict(name=name, sc=sc, opt=opt, plans=plans, fixed=fixed, ref=ref)
    opt.close()


def _first_out(plans, name):
    """plans in which `name` is the first tensor, in order of placement, that did not fit"""
    k = PRIORITY.index(name)
    return [p for p in plans if not _in(p, name) and all(_in(p, t) for t in PRIORITY[:k])]


def test_every_placement_of_the_ladder_equals_the_lockstep_loop(ladder):
    """Set A (and A16) under every distinct plan the LDS limit can produce, each solved in the tail kernel and compared with
    the lockstep loop bit for bit.  Each ladder must contain: nothing in LDS, all fourteen tensors, the plan of a 64 KiB
    device (limit 65536), every tensor as the first one out, a tensor out while a later one is in (the skip-and-continue
    branch of the placement), both values of every phase flag, all three forms of tail_forward; the split bit is set on
    some plan of A16 and on none of A (24 planes per knot: its scratch never fits).  Measured on the MI355X: 58 distinct
    plans for either set.  Unstable share under oracle_reference, measured on the CPU: 1 of 24 for either set (12 and 9
    of 24 with the knife-edge rule of zero-tolerance solves: the comment on set A)."""
    sc, opt, plans, ref = ladder["sc"], ladder["opt"], ladder["plans"], ladder["ref"]
    opt.stage_load(sc)
    p64k = _plan_at(opt, 65536)[0]
    assert 0 in {p & ALL_IN for p in plans} and ALL_IN in {p & ALL_IN for p in plans} and p64k in plans
    for name in PRIORITY:
        assert _first_out(plans, name), f"no plan in which {name} is the first tensor out"
    assert any(not _in(p, a) and _in(p, b) for p in plans for i, a in enumerate(PRIORITY) for b in PRIORITY[i + 1:]), "skip-and-continue never taken"
    for f in FLAGS:
        assert {_flag(p, f) for p in plans} == {False, True}, f
    assert {bool(p & SPLIT) for p in plans} == ({False, True} if ladder["name"] == "A16" else {False})
    forms = {("out+src" if _flag(p, "fwd") else "src" if _flag(p, "fwd_src") else "none") for p in plans}
    assert forms == {"out+src", "src", "none"}, forms
    print(f"\nset {ladder['name']}: {len(plans)} distinct plans, fixed block {ladder['fixed']} bytes")
    for plan, (limit, lds) in sorted(plans.items(), key=lambda kv: kv[1][0]):
        opt.stage_load(sc)
        assert _plan_at(opt, limit) == (plan, lds)
        got, took = _solve(opt, sc, limit)
        print(f"limit {limit:6d}  LDS {lds:6d}  {_describe(plan)}  tail problems {took}")
        assert took > 0, (limit, "the solve did not run in the tail kernel")
        _assert_same(ref, got, f"limit {limit}: {_describe(plan)}")
    opt.set_option(api.OPT_TAIL_LDS_LIMIT, 0)


def test_phase_flags_follow_from_the_tensor_mask(ladder):
    """A phase flag makes the phase cast its pointers to the LDS address space: it may be set only if every tensor the phase
    addresses that way is in LDS; the split quadratisation needs the quadratisation's tensors and the candidates' rows
    (its scratch) there, and exists for five discs only.  Checked on every plan of the sweep."""
    for plan in ladder["plans"]:
        for f in FLAGS:
            if _flag(plan, f):
                assert all(_in(plan, t) for t in PHASE_TENSORS[f]), (f, _describe(plan))
        if plan & SPLIT:
            assert _flag(plan, "quad") and all(_in(plan, t) for t in ("parts", "Xs", "Us")), _describe(plan)
            assert ladder["opt"].cfg.num_of_disc == 5
    assert ladder["opt"].get_option(api.OPT_TAIL_LDS_LIMIT) == (0, 0)
    with pytest.raises(api.CilqrError):
        ladder["opt"].set_option(api.OPT_TAIL_PLAN, 1)          # read-only
    with pytest.raises(api.CilqrError):
        ladder["opt"].set_option(api.OPT_TAIL_LDS_LIMIT, -1)
    fresh = api.BatchIlqrOptimizer(n_steps=20)
    with pytest.raises(api.CilqrError):
        fresh.get_option(api.OPT_TAIL_PLAN)                      # nothing loaded yet
    fresh.close()


@pytest.mark.parametrize("which,discs,exact", [("A", 3, 1), ("A", 3, 0), ("A", 5, 0), ("A16", 5, 0)])
def test_generic_disc_count_and_fast_ties_at_the_placements(scenes, which, discs, exact):
    """The other instantiations of the tail kernel -- k_tail<0, *> (a disc count other than five) and k_tail<*, false>
    (CILQR_OPT_EXACT_LANE_TIES 0) -- with everything in LDS, nothing in LDS, the plan of a 64 KiB device, and with the
    corridor planes alone left out (quadratisation and knot costs generic, backward pass and rollouts on LDS).  Set A16
    adds the split quadratisation under the fast rule.  The lockstep reference runs under the same configuration; three
    discs are anchored to the oracle (unstable share measured on the CPU: 1 of 24, 12 with the knife-edge rule), under the
    fast rule by the step replay
    with the lane_tie excuse."""
    sc = scenes[which]
    opt = _handle(sc, num_of_disc=discs, **OVER_A)
    opt.set_option(api.OPT_EXACT_LANE_TIES, exact)
    plans, _ = _sweep(opt, sc)
    assert any(p & SPLIT for p in plans) == (which == "A16"), "the split form exists for five discs and 16 planes only"
    what = f"set {which}, {discs} discs, exact ties {exact}"
    if discs == 3:
        ref = _anchor(opt, sc, UNSTABLE_A3, what, max_excused_frac=EXCUSED_ZERO_TOL, allow_lane_tie=not exact)
    else:
        ref, _ = _solve(opt, sc, 0, tail=False)
    assert ref["n_iter"].max() > 12
    opt.stage_load(sc)
    assert _plan_at(opt, 0)[0] & ALL_IN == ALL_IN and _plan_at(opt, 16)[0] & ALL_IN == 0
    limits = {"everything in": 0, "nothing in": 16, "64 KiB device": 65536,
              "corridor planes out": plans[_first_out(plans, "cor")[0]][0]}
    for name, limit in limits.items():
        opt.stage_load(sc)
        plan = _plan_at(opt, limit)[0]
        got, took = _solve(opt, sc, limit)
        print(f"\n{what}, {name}: limit {limit}  {_describe(plan)}  tail problems {took}")
        assert took > 0
        _assert_same(ref, got, (what, name))
    opt.close()


def test_a_full_grid_over_arena_resident_tensors():
    """70 problems are launched as a grid of 128 workgroups, whose list positions -- and private arenas -- are permuted
    (xcd_local_position).  With nothing in LDS, and with `lin` in the arena while `gains` is in LDS, every tensor access
    goes through that arena index: both equal the lockstep loop, and a problem's result does not depend on its position in
    the batch (the same 70 in reversed order).  Unstable share of this set under oracle_reference, measured on the CPU: 2 of
    70 (46 with the knife-edge rule of zero-tolerance solves: the comment on set A)."""
    B = 70
    sc = scenario.generate(SPEC_A, B, seed=SEED_A70)
    opt = _handle(sc, **OVER_A)
    plans, _ = _sweep(opt, sc)
    ref = _anchor(opt, sc, UNSTABLE_A70, "set A70", max_excused_frac=EXCUSED_ZERO_TOL)
    _assert_hard(ref, "set A70")
    lin_out = [p for p in plans if not _in(p, "lin") and _in(p, "gains")]
    assert lin_out
    for limit in (16, plans[lin_out[0]][0]):
        opt.stage_load(sc)
        plan = _plan_at(opt, limit)[0]
        got, took = _solve(opt, sc, limit)
        print(f"\nB = {B}, limit {limit}: {_describe(plan)}  tail problems {took}")
        assert took == B
        _assert_same(ref, got, f"B = {B}, limit {limit}")
    rev = {k: (np.ascontiguousarray(v[::-1]) if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in sc.items()}
    got, took = _solve(opt, rev, 16)
    assert took == B
    _assert_same(ref, {k: np.ascontiguousarray(got[k][::-1]) for k in KEYS}, "reversed order")
    opt.close()


def _subdivide(tab, rows):
    """A lane table (rows a, b, c, start, end: scenario.lane_constraints) with every segment cut evenly into pieces, `rows`
    rows in all: the same boundary, described in as much detail as the ABI allows."""
    S = tab.shape[0]
    assert rows >= S
    base, extra = divmod(rows, S)
    out = []
    for k in range(S):
        n = base + (1 if k < extra else 0)
        t = np.linspace(0.0, 1.0, n + 1)
        px = tab[k, 3] + t * (tab[k, 5] - tab[k, 3])
        py = tab[k, 4] + t * (tab[k, 6] - tab[k, 4])
        sx, sy, ex, ey = px[:-1], py[:-1], px[1:], py[1:]
        a, b = ey - sy, -(ex - sx)
        out.append(np.stack([a, b, a * sx + b * sy, sx, sy, ex, ey], axis=1))
    out = np.ascontiguousarray(np.concatenate(out))
    assert out.shape == (rows, 7)
    return out


def test_lane_tables_at_the_abi_maximum_push_tensors_out():
    """mix11 at the bench horizon (N = 50, cmax 16) with lane tables of 2 x 256 segments (CILQR_MAX_LANE_SEGMENTS): 45 KB of
    the tail's fixed LDS block, so that with NO limit set the working set no longer fits what the device grants and the
    launch leaves tensors in the arena.  Tail against lockstep bit for bit, lockstep against the oracle (unstable share
    measured on the CPU: see UNSTABLE_LANES)."""
    sc = scenario.generate("mix11", 24, seed=SEED_LANES)
    sc["left"], sc["right"] = _subdivide(sc["left"], 256), _subdivide(sc["right"], 256)
    opt = _handle(sc, max_lane_segments=256)
    opt.stage_load(sc)
    assert opt.get_option(api.OPT_TAIL_LDS_LIMIT) == (0, 0)
    plan, lds = opt.get_option(api.OPT_TAIL_PLAN)
    print(f"\n2 x 256 lane segments, no limit: LDS {lds}  {_describe(plan)}")
    assert plan & SUPPORTED and plan & ALL_IN != ALL_IN, "the device alone must push a tensor out"
    ref = _anchor(opt, sc, UNSTABLE_LANES, "2 x 256 lane segments")
    got, took = _solve(opt, sc, 0)
    assert took == 24
    _assert_same(ref, got, "2 x 256 lane segments")
    opt.close()


def test_the_tail_supported_edge_is_straddled():
    """tail_supported: the fixed block (lane tables, the backward pass's operands and per-step rows, the view) must fit
    62 KiB.  At N = 250 the edge lies inside the ABI's lane-table sizes (about 250 rows per side at 88 bytes per row; measured: 248): the
    number of rows per side is bisected between 200 and 256 on the plan's supported bit.  At the largest supported count the
    solve runs in the tail kernel and equals the lockstep loop; one row more per side and it stays in the lockstep loop,
    whatever CILQR_OPT_TAIL_THRESHOLD says."""
    B = 4
    base = scenario.generate(dataclasses.replace(scenario.SPECS["mix11"], n_steps=250), B, seed=SEED_EDGE)
    opt = _handle(base, max_lane_segments=256)

    def with_rows(rows):
        sc = dict(base)
        sc["left"], sc["right"] = _subdivide(base["left"], rows), _subdivide(base["right"], rows)
        return sc

    def supported(rows):
        opt.stage_load(with_rows(rows))
        return bool(opt.get_option(api.OPT_TAIL_PLAN)[0] & SUPPORTED)

    lo, hi = 200, 256
    assert supported(lo) and not supported(hi), "the edge is not inside 200..256 rows per side at this horizon"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if supported(mid):
            lo = mid
        else:
            hi = mid
    print(f"\nN = 250: the tail is supported up to {lo} lane rows per side")
    # the largest supported table: anchored to the oracle (the boundary is the same whatever the number of pieces), then the tail
    sc = with_rows(lo)
    ref = _anchor(opt, sc, UNSTABLE_EDGE, f"N = 250, {lo} lane rows per side", max_excused_frac=EXCUSED_LONG)
    opt.stage_load(sc)
    plan, lds = opt.get_option(api.OPT_TAIL_PLAN)
    got, took = _solve(opt, sc, 0)
    print(f"{lo} rows: LDS {lds}  {_describe(plan)}  tail problems {took}")
    assert took == B
    _assert_same(ref, got, f"N = 250, {lo} rows")
    # one row more per side: the product default stays in the lockstep loop and equals the run that was told to
    sc = with_rows(hi)
    ref, _ = _solve(opt, sc, 0, tail=False)
    got, took = _solve(opt, sc, 0)
    assert took == 0
    _assert_same(ref, got, f"N = 250, {hi} rows")
    opt.close()
