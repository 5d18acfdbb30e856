"""The stop rule on the GPU (cilqr_stop_rows_batch, kernels_stop.hip) against the host call (cilqr_stop_rows, which
tests/test_stop.py holds to the NumPy statement and to fractions): every element of the rows, the statuses, the stop knots
and the travelled stations bit for bit, a NaN matching a NaN.

A workgroup takes a run of whole trajectories and works through the rows in chunks of at most 12 knots, fewer where its LDS
asks for it: the shapes put one trajectory and several hundred, one row and two (a single chunk), 51 (five chunks, the last a
short one), 256 rows of eight profiles on 7 knots (three trajectories a workgroup) and on 256 (the worst case: one
trajectory a workgroup, chunks of 10 or 13), one profile and eight, every layout, both memories.  Sizes are the smallest that reach
every path."""
import ctypes as C

import numpy as np
import pytest

import stop_cases as sc
from cilqr_amd import api, scenario, stop

pytestmark = pytest.mark.gpu

OUTPUTS = ("rows", "status", "stop_knot", "travel")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=128, cmax=16, max_lane_segments=256) as o:
        yield o


def check(got, want, what):
    for k in ("status", "stop_knot"):
        assert np.array_equal(np.asarray(got[k]), want[k]), (what, k)
    for k in ("travel", "rows"):
        if k in got:
            g = np.asarray(got[k]).reshape(want[k].shape)
            bad = ~((g.view(np.uint64) == want[k].view(np.uint64)) | (np.isnan(g) & np.isnan(want[k])))
            assert not bad.any(), (what, k, np.argwhere(bad)[:5])


def run(opt, rows, layout, profiles, dt, n_out, start_va, memory, **kw):
    if memory == api.MEM_HOST:
        return opt.stop_rows(rows, layout, profiles, dt, n_out, start_va, **kw)
    import torch
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    out = opt.stop_rows(torch.from_numpy(rows).to(dev), layout, profiles, dt, n_out,
                        None if start_va is None else torch.from_numpy(start_va).to(dev), **kw)
    assert out["status"].is_cuda and out["status"].dtype == torch.int32
    return {k: v.cpu().numpy() for k, v in out.items()}


# B, knots, rows out, profiles, layout, memory
SHAPES = [(1, 2, 1, 1, layout, memory) for layout in sc.LAYOUTS for memory in (api.MEM_HOST, api.MEM_DEVICE)] + \
         [(B, 51, 51, 3, layout, memory) for B in (63, 64, 65) for layout in sc.LAYOUTS for memory in (api.MEM_HOST, api.MEM_DEVICE)] + \
         [(65, 7, 256, 8, api.ROWS_TRAJ, api.MEM_DEVICE),
          (257, 256, 256, 8, api.ROWS_TRAJ, api.MEM_DEVICE),        # the limits of all three counts: chunks of 13 knots, of 10 for plan rows
          (257, 256, 256, 8, api.ROWS_PLAN, api.MEM_HOST),
          (257, 51, 2, 1, api.ROWS_COARSE, api.MEM_HOST)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d-N%d-M%d-l%d-m%d" % tuple(int(v) for v in s))
def test_kernel_equals_the_host_call_bit_for_bit(opt, shape):
    B, K, N, M, layout, memory = shape
    dt = 0.1 if N <= 51 else 0.05
    plans, start_va, kinds = sc.make_batch(B, K, seed=B * 1000 + K + N)
    rows = np.stack([sc.from_plan(p, layout) for p in plans])
    profiles = sc.BATCH_PROFILES[:M]
    va = start_va if (B + K) % 2 else None        # given and absent
    want = sc.host_batch(api, rows, layout, profiles, dt, N, va)
    got = run(opt, rows, layout, profiles, dt, N, va, memory)
    check(got, want, shape)
    if B >= 63:      # the batch did hold every status, a carried NaN and a degenerate pair that a clamped station meets
        assert set(want["status"].ravel().tolist()) == {stop.STOPPED, stop.MOVING, stop.OVERRUN, stop.REFUSED}
        carried = kinds == sc.KINDS.index("carried_nan")
        assert np.isnan(rows[carried]).any() and (want["status"][:, carried] != stop.REFUSED).all()
        ends = kinds == sc.KINDS.index("short_standing_end")
        assert (plans[ends, -1, 1] == plans[ends, -2, 1]).all() and (want["status"][:, ends] == stop.OVERRUN).any()
        refused = want["status"] == stop.REFUSED
        assert not np.asarray(got["rows"])[refused].view(np.uint64).any()


# LDS a launch plans with (KiB), knots a chunk at the most: the two hooks of kernels_stop.hip's launch plan, which
# tools/stop_bench.py turns.  8 KiB / 3 knots: the smallest workgroups and the most chunks; 60 / 256: the whole image where it
# fits; 24 / 5: a chunk length that divides neither 51 nor 40; 32 / 1: one knot a chunk, every row beside its look-ahead
PLANS = [(8, 3), (60, 256), (24, 5), (32, 1)]


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: "lds%d-chunk%d" % p)
def test_rows_do_not_depend_on_the_launch_plan(opt, plan, monkeypatch):
    monkeypatch.setenv("CILQR_STOP_LDS_KB", str(plan[0]))
    monkeypatch.setenv("CILQR_STOP_CHUNK", str(plan[1]))
    for B, K, N, M, layout in ((65, 51, 51, 3, api.ROWS_TRAJ), (9, 256, 40, 8, api.ROWS_PLAN), (17, 7, 256, 8, api.ROWS_COARSE)):
        plans, va, _ = sc.make_batch(B, K, seed=31 + B)
        rows = np.stack([sc.from_plan(p, layout) for p in plans])
        want = sc.host_batch(api, rows, layout, sc.BATCH_PROFILES[:M], 0.1, N, va)
        check(opt.stop_rows(rows, layout, sc.BATCH_PROFILES[:M], 0.1, N, va), want, (plan, B, K, N, M))
        assert (want["status"] == stop.REFUSED).any() and (want["status"] == stop.STOPPED).any()


def test_crafted_table_alone(opt):
    """every case of the table as a batch of its own (its own counts, profiles and step), HOST arrays: against the host call
    and -- kernel and host call run one pair step (include/cilqr/row_math.hpp), so a wrong one agrees with itself --
    against the NumPy statement"""
    for case in sc.cases():
        va = None if case["start_va"] is None else case["start_va"][None]
        want = sc.host_batch(api, case["rows"][None], case["layout"], case["profiles"], case["delta_t"], case["n_out"], va)
        got = opt.stop_rows(case["rows"][None], case["layout"], case["profiles"], case["delta_t"], case["n_out"], va)
        check(got, want, case["name"])
        check(got, {k: np.asarray(v)[:, None] for k, v in sc.reference(case).items()}, (case["name"], "NumPy statement"))
        if case["expect"] is not None:
            assert got["status"][0, 0] == case["expect"], case["name"]


def test_a_chain_depends_neither_on_its_batch_nor_on_the_profiles_around_it(opt):
    """B = 1 with M = 1 (one trajectory in its workgroup) against the same trajectory and profile inside B = 257 with M = 8
    (two trajectories a workgroup, eight chains each)"""
    K, N, layout, dt = 51, 256, api.ROWS_TRAJ, 0.05
    plans, va, _ = sc.make_batch(257, K, seed=11)
    rows = np.stack([sc.from_plan(p, layout) for p in plans])
    whole = opt.stop_rows(rows, layout, sc.BATCH_PROFILES, dt, N, va)
    for b, m in ((0, 0), (3, 7), (131, 2), (200, 5), (256, 1), (4, 4), (7, 6)):
        one = opt.stop_rows(rows[b:b + 1], layout, sc.BATCH_PROFILES[m:m + 1], dt, N, va[b:b + 1])
        for k in OUTPUTS:
            a, z = np.ascontiguousarray(one[k][0, 0]), np.ascontiguousarray(whole[k][m, b])
            assert a.tobytes() == z.tobytes(), (b, m, k)      # NaNs included: the same code made them


def test_every_pointer_offset_by_one_double_and_outputs_omitted_one_at_a_time(opt):
    """device arrays that start 8 bytes past a 16-byte boundary (4 bytes for the int32 outputs), each output left out in turn"""
    import torch
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    B, K, N, M, layout, dt = 65, 51, 51, 3, api.ROWS_PLAN, 0.1
    plans, va, _ = sc.make_batch(B, K, seed=77)
    rows = np.stack([sc.from_plan(p, layout) for p in plans])
    profiles = sc.BATCH_PROFILES[:M]
    want = sc.host_batch(api, rows, layout, profiles, dt, N, va)

    def shifted(n, dtype=torch.float64, fill=None):
        t = torch.full((n + 1,), -7, dtype=dtype, device=dev)[1:]
        assert t.data_ptr() % 16 == (8 if dtype == torch.float64 else 4)
        if fill is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(fill).ravel()))
        return t

    d_rows, d_va = shifted(rows.size, fill=rows), shifted(va.size, fill=va)
    gives = [(True,) * 4] + [tuple(i != skip for i in range(4)) for skip in range(4)] + \
            [tuple(i == only for i in range(4)) for only in range(4)]
    for give in gives:
        outs = [shifted(M * B * N * 11), shifted(M * B, torch.int32), shifted(M * B, torch.int32), shifted(M * B)]
        code = opt.stop_rows_raw(B, layout, d_rows.data_ptr(), K, profiles, d_va.data_ptr(), dt, N,
                                 *[o.data_ptr() if g else None for o, g in zip(outs, give)], api.MEM_DEVICE)
        assert code == api.OK
        got = {k: o.cpu().numpy().reshape(want[k].shape) for k, o, g in zip(OUTPUTS, outs, give) if g}
        for k in got:
            assert sc.same_bits(got[k], want[k]) if got[k].dtype == np.float64 else np.array_equal(got[k], want[k]), (give, k)
        for k, o, g in zip(OUTPUTS, outs, give):
            if not g:
                assert (o.cpu().numpy() == -7).all(), (give, k)
    # the summaries alone through the wrapper, HOST arrays
    lean = opt.stop_rows(rows, layout, profiles, dt, N, va, with_rows=False)
    assert "rows" not in lean
    check(lean, want, "summaries alone")


def test_refusals_leave_the_outputs_unwritten(opt):
    B, K, N, M, layout = 3, 5, 4, 2, api.ROWS_PLAN
    plans, va, _ = sc.make_batch(B, K, seed=9)
    prof = np.ascontiguousarray(sc.BATCH_PROFILES[:M])
    out, travel = np.full((M, B, N, 11), -7.0), np.full((M, B), -7.0)
    status, knot = np.full((M, B), -9, np.int32), np.full((M, B), -9, np.int32)

    def call(h=True, batch=B, layout=layout, rows=True, n_knots=K, n_profiles=M, profiles=prof, dt=0.1, n_out=N, outputs=True,
             memory=api.MEM_HOST, on=None):
        o = on or opt
        outs = [a.ctypes.data for a in (out, status, knot, travel)] if outputs else [None] * 4
        code = o.L.cilqr_stop_rows_batch(o.h if h else None, batch, layout, plans.ctypes.data if rows else None, n_knots,
                                         n_profiles, None if profiles is None else profiles.ctypes.data, va.ctypes.data,
                                         C.c_double(dt), n_out, *outs, memory)
        if code != api.OK:
            assert (out == -7.0).all() and (travel == -7.0).all() and (status == -9).all() and (knot == -9).all()
        return code

    assert call(h=False) == api.ERR_NULL and call(rows=False) == api.ERR_NULL and call(profiles=None) == api.ERR_NULL
    assert call(batch=0) == api.ERR_ARG and call(memory=7) == api.ERR_ARG and call(outputs=False) == api.ERR_ARG
    assert call(layout=3) == api.ERR_ARG and call(layout=api.ROWS_POINTS) == api.ERR_ARG
    assert call(n_knots=1) == api.ERR_ARG and call(n_out=0) == api.ERR_ARG and call(dt=0.0) == api.ERR_ARG
    assert call(dt=float("nan")) == api.ERR_ARG
    assert call(n_profiles=0) == api.ERR_ARG
    assert call(n_profiles=api.STOP_MAX_PROFILES + 1, profiles=np.tile(prof, (5, 1))) == api.ERR_ARG
    for bad in ((0.5, -1.0), (-1.0, 0.0), (np.nan, -1.0), (-1.0, -np.inf)):
        assert call(profiles=np.array([prof[0], bad])) == api.ERR_ARG, bad
    assert call(n_knots=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY and call(n_out=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    # solves submitted on the handle
    g = scenario.generate("mix11", 64, seed=3)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=64, cmax=g["cmax"]) as busy:
        problem, keep = busy._host_problem(g)
        Bs, iters = 64, busy.cfg.max_iter
        traj, hist = np.zeros((Bs, 51, 10)), np.zeros((Bs, iters + 1, 5))
        nc, st, ni = (np.zeros(Bs, dtype=np.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_HOST, 0, traj.ctypes.data, hist.ctypes.data, nc.ctypes.data, st.ctypes.data,
                                ni.ctypes.data, None, None, None)
        assert busy.L.cilqr_submit(busy.h, C.byref(problem), C.byref(sol)) == api.OK
        assert call(on=busy) == api.ERR_STATE
        assert busy.L.cilqr_wait(busy.h) == api.OK
        assert call(on=busy) == api.OK
        del keep
    want = sc.host_batch(api, plans, layout, prof, 0.1, N, va)
    check(dict(rows=out, status=status, stop_knot=knot, travel=travel), want, "after the refusals")
