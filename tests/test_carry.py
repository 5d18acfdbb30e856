"""The carry rule on the host (cilqr_carry_rows, include/cilqr/trajectory_queries.hpp: carry_rows): a trajectory of the
previous cycle as the coarse trajectory of the next.  Held against the NumPy statement cilqr_amd/carry.py bit for bit,
against an independent composition -- cilqr_resample_rows plus a running sum in Python --, and on crafted trajectories
whose branches are counted (tests/carry_cases.py)."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import carry_cases as cc
import resample_cases as rc
from cilqr_amd import api, carry, resample

SENTINEL = -7.0
# the C library's hypot, which the rule names (Python's math.hypot is an algorithm of its own and differs in the last bit)
_LIBM = C.CDLL("libm.so.6")
_LIBM.hypot.restype = C.c_double
_LIBM.hypot.argtypes = [C.c_double, C.c_double]
c_hypot = _LIBM.hypot


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def crafted():
    return cc.crafted_cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def composed(case, layout):
    """the rule from the public resample call and plain Python floats: no code shared with either statement"""
    rows = rc.rows_in_layout(layout, case.plan)
    K = case.n_knots
    zero = dict(coarse9=np.zeros((K, 9)), coarse6=np.zeros((K, 6)), knots3=np.zeros((K, 3)), station=np.zeros(K))
    a = case.advance
    if a < 0.0:
        return dict(state=1, **zero)
    if math.isnan(a) or a > case.max_advance or not (float(rows[-1, 0]) - float(rows[0, 0]) > 0.0):
        return dict(state=2, **zero)
    first = float(rows[0, 0]) + a
    r = api.resample_rows(rows, layout, [first + k * case.delta_t for k in range(K)], api.KEY_TIME)
    cols = {api.ROWS_TRAJ: (1, 2, 3, 7, 4, 5, 6)}.get(layout, (2, 3, 4, 5, 6, 7, 8))
    nine = np.zeros((K, 9))
    s = 0.0
    for k in range(K):
        nine[k, 0] = case.delta_t * k
        nine[k, 2:] = r[k, list(cols)]
        if k > 0:
            s = s + c_hypot(float(nine[k, 2]) - float(nine[k - 1, 2]), float(nine[k, 3]) - float(nine[k - 1, 3]))
        nine[k, 1] = s
    if not all(math.isfinite(v) for v in nine[:, [2, 3, 4, 6, 7, 8]].ravel()):
        return dict(state=2, **zero)
    return dict(state=0, coarse9=nine, coarse6=nine[:, [2, 3, 4, 6, 7, 8]], knots3=nine[:, 2:5], station=nine[:, 1])


def test_entry_points_are_declared_exported_and_mirrored():
    hdr = open(api.HEADER_PATH).read()
    L = api.lib()
    for name in ("cilqr_carry_rows", "cilqr_carry_rows_batch", "cilqr_plan_scenes_batch_carry"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("KEPT", "NOT_ASKED", "REFUSED", "OFF_START", "HIT"):
        value = int(re.search(r"#define CILQR_CARRY_%s (\d+)" % name, hdr).group(1))
        assert getattr(api, "CARRY_" + name) == value == getattr(carry, name), name
    assert re.search(r"CILQR_ABI_VERSION (\d+)", hdr).group(1) == "7" and L.cilqr_abi_version() == 7
    # the struct as the header lays it out: four int32, two pointers, three doubles
    assert C.sizeof(api.Carry) == 4 * 4 + 2 * C.sizeof(C.c_void_p) + 3 * 8
    assert [f[0] for f in api.Carry._fields_] == ["memory", "layout", "n_rows", "reserved0", "rows", "advance", "max_advance",
                                                  "max_start_offset", "collision_buffer"]


def test_crafted_table_reaches_every_branch(crafted):
    names = [c.name for c in crafted]
    for needed in cc.NEEDED:
        assert needed in names, needed
    states, branches = cc.census(crafted)
    assert all(n >= 2 for n in states.values()), states
    assert all(branches[b] >= 1 for b in ("degenerate", "past_end", "first_pair", "search")), branches
    assert branches["before_start"] == 0          # a kept advance is not negative: no knot lies before the first row
    for case in crafted:                          # ... and every case reaches what it was written for
        assert set(case.branches) <= cc.knot_branches(case), (case.name, case.branches, cc.knot_branches(case))
    by_name = {c.name: c for c in crafted}
    c = by_name["advance past the last row"]
    q = (c.plan[0, 0] + c.advance) + np.arange(c.n_knots) * c.delta_t
    assert (q >= c.plan[-1, 0]).sum() == 5        # five knots of extrapolation


def test_host_call_equals_the_numpy_statement_and_the_composition(crafted):
    for case in crafted + cc.random_cases():
        for layout in cc.LAYOUTS:
            got = cc.host_carry(case, layout)
            rows = rc.rows_in_layout(layout, case.plan)
            stated = carry.carry_rows(rows, layout, case.advance, case.max_advance, case.n_knots, case.delta_t)
            assert cc.same_result(got, stated), (case.name, layout, got, stated)
            assert cc.same_result(got, composed(case, layout)), (case.name, layout)
            if case.state is not None:
                assert got["state"] == case.state, (case.name, layout, got["state"])
            if got["state"] != carry.KEPT:        # every row is zero, and +0
                for k in ("coarse9", "coarse6", "knots3", "station"):
                    assert not _bits(got[k]).any(), (case.name, k)


def test_crafted_values_follow_from_the_rule(crafted):
    by_name = {c.name: c for c in crafted}
    P = api.ROWS_PLAN
    # advance 0: row 0 keeps the source's bits (w = 0 on the first pair), time and station start at 0
    c = by_name["advance 0"]
    out = cc.host_carry(c, P)
    lin = [2, 3, 5, 6, 7, 8]
    assert np.array_equal(_bits(out["coarse9"][0, lin]), _bits(1.0 * c.plan[0, lin] + 0.0 * c.plan[1, lin]))
    assert abs(out["coarse9"][0, 4] - resample.normalize_angle(c.plan[0, 4])) < 1e-15      # slerp wraps the heading
    assert np.array_equal(out["coarse9"][0, 2:4], c.plan[0, 2:4]) and out["coarse9"][0, 0] == 0.0 and out["station"][0] == 0.0
    assert np.array_equal(out["coarse9"][:, 0], c.delta_t * np.arange(c.n_knots))
    # the projections are columns of coarse9
    assert np.array_equal(_bits(out["coarse6"]), _bits(out["coarse9"][:, [2, 3, 4, 6, 7, 8]]))
    assert np.array_equal(_bits(out["knots3"]), _bits(out["coarse9"][:, 2:5]))
    assert np.array_equal(_bits(out["station"]), _bits(out["coarse9"][:, 1]))
    # the station is the running sum of the chord lengths, in knot order
    s = 0.0
    for k in range(1, c.n_knots):
        s = s + c_hypot(out["coarse9"][k, 2] - out["coarse9"][k - 1, 2], out["coarse9"][k, 3] - out["coarse9"][k - 1, 3])
        assert out["station"][k] == s
    # on a knot: w = 1 on the pair below it
    c = by_name["advance on a knot"]
    out = cc.host_carry(c, P)
    assert np.array_equal(out["coarse9"][0, [2, 3, 5, 6, 7, 8]], 0.0 * c.plan[2, [2, 3, 5, 6, 7, 8]] + c.plan[3, [2, 3, 5, 6, 7, 8]])
    # past the end: the last pair extrapolates
    c = by_name["advance past the last row"]
    out = cc.host_carry(c, P)
    q = (c.plan[0, 0] + c.advance) + 9 * c.delta_t
    w = (q - c.plan[-2, 0]) / (c.plan[-1, 0] - c.plan[-2, 0])
    assert w > 1 and out["coarse9"][9, 2] == (1 - w) * c.plan[-2, 2] + w * c.plan[-1, 2]
    # the limit is inclusive
    assert cc.host_carry(by_name["advance equal to max_advance"], P)["state"] == carry.KEPT
    assert cc.host_carry(by_name["advance just above max_advance"], P)["state"] == carry.REFUSED
    # a degenerate pair: the first row as bits
    c = by_name["duplicated time"]
    out = cc.host_carry(c, P)
    assert np.array_equal(_bits(out["coarse9"][0, 2:]), _bits(c.plan[0, 2:9]))
    # headings come out wrapped and take the short way round
    for name in ("heading across pi", "heading across -pi"):
        c = by_name[name]
        th = cc.host_carry(c, P)["coarse9"][:, 4]
        assert ((-np.pi <= th) & (th < np.pi)).all() and (th > 0).any() and (th < 0).any()
        assert (np.abs(np.abs(th) - np.pi) < 0.2).all()
    # a NaN curvature is no reason to refuse: it is what a plan that stands still carries
    c = by_name["NaN kappa is carried"]
    out = cc.host_carry(c, P)
    assert out["state"] == carry.KEPT and np.isnan(out["coarse9"][:, 5]).all() and np.isfinite(out["coarse6"]).all()
    # a NaN refuses its own trajectory only when a knot reaches it
    assert cc.host_carry(by_name["NaN in one column of one row"], P)["state"] == carry.REFUSED
    assert cc.host_carry(by_name["NaN in a row no knot reaches"], P)["state"] == carry.KEPT


def test_optional_outputs_and_argument_errors():
    L = api.lib()
    rng = np.random.default_rng(4)
    plan = rc.smooth_plan(rng, np.arange(api.DP_MAX_KNOTS + 1) * 0.1)

    def call(layout=api.ROWS_PLAN, n_rows=5, advance=0.05, max_advance=1.0, n_knots=4, delta_t=0.1, rows=True, state=True,
             give=(True, True, True, True)):
        r = rc.rows_in_layout(layout if layout in rc.LAYOUTS else api.ROWS_PLAN, plan)
        outs = [np.full((max(n_knots, 1), w), SENTINEL) for w in (9, 6, 3, 1)]
        st = C.c_int32(-9)
        code = L.cilqr_carry_rows(layout, r.ctypes.data if rows else None, n_rows, C.c_double(advance), C.c_double(max_advance),
                                  n_knots, C.c_double(delta_t), *[o.ctypes.data if g else None for o, g in zip(outs, give)],
                                  C.byref(st) if state else None)
        if code != api.OK:      # nothing was written
            assert all((o == SENTINEL).all() for o in outs) and st.value == -9
        else:
            for o, g in zip(outs, give):
                assert (o[:n_knots] != SENTINEL).all() == g
        return code

    assert call() == api.OK
    for give in ((False, True, True, True), (True, False, False, False), (False, False, False, False)):
        assert call(give=give) == api.OK
    assert call(rows=False) == api.ERR_NULL and call(state=False) == api.ERR_NULL
    assert call(layout=3) == api.ERR_ARG and call(layout=-1) == api.ERR_ARG and call(layout=api.ROWS_POINTS) == api.ERR_ARG
    assert call(n_rows=1) == api.ERR_ARG and call(n_rows=0) == api.ERR_ARG and call(n_rows=-2) == api.ERR_ARG
    assert call(n_knots=0) == api.ERR_ARG and call(n_knots=-1) == api.ERR_ARG
    assert call(delta_t=0.0) == api.ERR_ARG and call(delta_t=-0.1) == api.ERR_ARG and call(delta_t=float("nan")) == api.ERR_ARG
    assert call(max_advance=-1.0) == api.ERR_ARG and call(max_advance=float("nan")) == api.ERR_ARG
    assert call(max_advance=float("inf")) == api.ERR_ARG and call(max_advance=0.0, advance=0.0) == api.OK
    assert call(n_rows=api.DP_MAX_KNOTS) == api.OK and call(n_rows=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    assert call(n_knots=api.DP_MAX_KNOTS) == api.OK and call(n_knots=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    for layout in (api.ROWS_TRAJ, api.ROWS_COARSE):
        assert call(layout=layout) == api.OK
    with pytest.raises(api.CilqrError) as e:
        api.carry_rows(plan[:1], api.ROWS_PLAN, 0.0, 1.0, 4, 0.1)
    assert e.value.code == api.ERR_ARG
    with pytest.raises(ValueError):
        carry.carry_rows(plan[:5], 7, 0.0, 1.0, 4, 0.1)


def test_selection_rule_of_the_pipeline_in_numpy():
    """carry.source_of, the host statement of the pipeline's selection: first match wins"""
    assert carry.source_of(carry.NOT_ASKED, (0, 0), (9, 9), 3, 0.5) == carry.NOT_ASKED
    assert carry.source_of(carry.REFUSED, (0, 0), (9, 9), 3, 0.5) == carry.REFUSED
    assert carry.source_of(carry.KEPT, (0, 0), (3, 4), 3, 4.999) == carry.OFF_START
    assert carry.source_of(carry.KEPT, (0, 0), (3, 4), 3, 5.0) == carry.HIT          # the offset's limit is inclusive
    assert carry.source_of(carry.KEPT, (0, 0), (3, 4), -2, 5.0) == carry.HIT         # a scene the audit refused
    assert carry.source_of(carry.KEPT, (0, 0), (3, 4), -1, 5.0) == carry.KEPT
    assert carry.source_of(carry.KEPT, (np.nan, 0), (3, 4), -1, 5.0) == carry.OFF_START
