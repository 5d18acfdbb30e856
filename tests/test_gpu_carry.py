"""The carry rule on the GPU (cilqr_carry_rows_batch, kernels_carry.hip) against the host call (cilqr_carry_rows, which
tests/test_carry.py holds to the NumPy statement and to a composition of public calls): the state and every element of the
four outputs bit for bit -- carry_cases.same_result: equal bit patterns, a NaN (a carried curvature) matching a NaN.

One wavefront works on one trajectory, its lanes striding over the knots and over the doubles of every output: the shapes
put fewer knots than lanes (1, 2, 51) and more (256), batches of one, either side of 64 and of several hundred, every
layout, both memories.  Sizes are the smallest that still reach every path of the kernel."""
import numpy as np
import pytest

import carry_cases as cc
import resample_cases as rc
from cilqr_amd import api, carry

pytestmark = pytest.mark.gpu

OUTPUTS = (("coarse9", 9), ("coarse6", 6), ("knots3", 3), ("station", 1))


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=128, cmax=16, max_lane_segments=256) as o:
        yield o


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_batch(rows, layout, advance, max_advance, K, dt):
    """the host call, trajectory by trajectory, stacked like the batched call's result"""
    per = [api.carry_rows(rows[b], layout, advance[b], max_advance, K, dt) for b in range(rows.shape[0])]
    out = {k: np.stack([p[k] for p in per]) for k, _ in OUTPUTS}
    out["state"] = np.array([p["state"] for p in per], dtype=np.int32)
    return out


def check(got, want, what):
    assert np.array_equal(np.asarray(got["state"]), want["state"]), (what, got["state"], want["state"])
    for k, _ in OUTPUTS:
        g = np.asarray(got[k]).reshape(want[k].shape)
        bad = ~((_bits(g) == _bits(want[k])) | (np.isnan(g) & np.isnan(want[k])))
        assert not bad.any(), (what, k, np.argwhere(bad)[:5])
    assert got["n_kept"] == int((want["state"] == carry.KEPT).sum()), what


def run(opt, rows, layout, advance, max_advance, K, dt, memory):
    if memory == api.MEM_HOST:
        return opt.carry(rows, layout, advance, max_advance, K, dt)
    import torch
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    out = opt.carry(torch.from_numpy(rows).to(dev), layout, torch.from_numpy(advance).to(dev), max_advance, K, dt)
    assert out["coarse9"].is_cuda and out["state"].dtype == torch.int32
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


# B, rows, knots, layout, memory
SHAPES = [
    (1, 2, 1, api.ROWS_PLAN, api.MEM_HOST),
    (1, 51, 51, api.ROWS_TRAJ, api.MEM_DEVICE),
    (63, 51, 51, api.ROWS_PLAN, api.MEM_DEVICE),
    (64, 51, 2, api.ROWS_TRAJ, api.MEM_HOST),
    (64, 7, 51, api.ROWS_COARSE, api.MEM_HOST),
    (65, 11, 256, api.ROWS_COARSE, api.MEM_DEVICE),
    (65, 2, 51, api.ROWS_PLAN, api.MEM_DEVICE),
    (257, 256, 256, api.ROWS_PLAN, api.MEM_DEVICE),          # the limits of both counts: the largest LDS image
    (257, 51, 51, api.ROWS_TRAJ, api.MEM_HOST),
    (257, 64, 1, api.ROWS_COARSE, api.MEM_DEVICE),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-R%d-K%d-l%d-m%d" % tuple(int(v) for v in s))
def test_kernel_equals_the_host_call_bit_for_bit(opt, shape):
    B, R, K, layout, memory = shape
    dt = 0.1 if K <= 51 else 0.004            # 256 knots stay inside and run past the rows
    plans, advance, kinds = cc.make_batch(B, R, seed=B * 1000 + R + K)
    rows = rc.rows_in_layout(layout, plans)
    want = host_batch(rows, layout, advance, cc.BATCH_MAX_ADVANCE, K, dt)
    got = run(opt, rows, layout, advance, cc.BATCH_MAX_ADVANCE, K, dt, memory)
    check(got, want, shape)
    if B >= 63:      # the batch did hold every state, carried NaN curvatures and zero rows
        assert set(want["state"]) == {carry.KEPT, carry.NOT_ASKED, carry.REFUSED}
        assert np.isnan(want["coarse9"]).any()
        for b in range(B):
            if want["state"][b] != carry.KEPT:
                assert not _bits(np.asarray(got["coarse9"])[b]).any()


def test_crafted_table_alone(opt):
    """every crafted case as a batch of its own (its own row and knot counts, limit and step), every layout, HOST arrays:
    against the host call and -- kernel and host call run one pair step (include/cilqr/row_math.hpp), so a wrong one agrees
    with itself -- against the NumPy statement"""
    for case in cc.crafted_cases():
        for layout in cc.LAYOUTS:
            rows = rc.rows_in_layout(layout, case.plan)[None]
            adv = np.array([case.advance])
            want = host_batch(rows, layout, adv, case.max_advance, case.n_knots, case.delta_t)
            got = opt.carry(rows, layout, adv, case.max_advance, case.n_knots, case.delta_t)
            check(got, want, (case.name, layout))
            stated = carry.carry_rows(rows[0], layout, case.advance, case.max_advance, case.n_knots, case.delta_t)
            check(got, {k: np.asarray(v)[None] for k, v in stated.items()}, (case.name, layout, "NumPy statement"))
            assert want["state"][0] == case.state, case.name


def test_every_pointer_offset_by_one_double_and_optional_outputs(opt):
    """device arrays that start 8 bytes past a 16-byte boundary (4 bytes for the states), with and without each output"""
    import torch
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    B, R, K, layout, dt = 65, 51, 51, api.ROWS_PLAN, 0.1
    plans, advance, _ = cc.make_batch(B, R, seed=77)
    rows = rc.rows_in_layout(layout, plans)
    want = host_batch(rows, layout, advance, cc.BATCH_MAX_ADVANCE, K, dt)

    def shifted(n, dtype=torch.float64, fill=None):
        t = torch.full((n + 1,), -7, dtype=dtype, device=dev)[1:]
        assert t.data_ptr() % 16 == (8 if dtype == torch.float64 else 4)
        if fill is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(fill).ravel()))
        return t

    d_rows, d_adv = shifted(rows.size, fill=rows), shifted(B, fill=advance)
    for give in ((True, True, True, True), (False, True, False, True), (True, False, False, False), (False, False, False, False)):
        outs = [shifted(B * K * w) for _, w in OUTPUTS]
        state = shifted(B, torch.int32)
        rc_, n_kept = opt.carry_raw(B, layout, d_rows.data_ptr(), R, d_adv.data_ptr(), cc.BATCH_MAX_ADVANCE, K, dt,
                                    *[o.data_ptr() if g else None for o, g in zip(outs, give)], state.data_ptr(), api.MEM_DEVICE)
        assert rc_ == api.OK and n_kept == int((want["state"] == carry.KEPT).sum())
        assert np.array_equal(state.cpu().numpy(), want["state"])
        for (k, w), o, g in zip(OUTPUTS, outs, give):
            o = o.cpu().numpy().reshape(want[k].shape)
            if g:
                assert rc.same_rows(o, want[k]), (give, k)
            else:
                assert (o == -7.0).all(), (give, k)


def test_a_trajectory_does_not_depend_on_its_batch(opt):
    B1, B2, R, K, layout, dt = 65, 257, 51, 51, api.ROWS_TRAJ, 0.1
    p1, a1, _ = cc.make_batch(B1, R, seed=5)
    p2, a2, _ = cc.make_batch(B2, R, seed=6)
    where = [(7, 200), (32, 0), (64, 256), (3, 131)]          # (index in the first batch, in the second)
    for i, j in where:
        p2[j], a2[j] = p1[i], a1[i]
    g1 = opt.carry(rc.rows_in_layout(layout, p1), layout, a1, cc.BATCH_MAX_ADVANCE, K, dt)
    g2 = opt.carry(rc.rows_in_layout(layout, p2), layout, a2, cc.BATCH_MAX_ADVANCE, K, dt)
    for i, j in where:
        assert g1["state"][i] == g2["state"][j]
        for k, _ in OUTPUTS:
            assert np.array_equal(_bits(g1[k][i]), _bits(g2[k][j])), (i, j, k)      # NaNs included: the same code made them


def test_refusals_leave_the_outputs_unwritten(opt):
    B, R, K, layout = 3, 5, 4, api.ROWS_PLAN
    plans, advance, _ = cc.make_batch(B, R, seed=9)
    outs = [np.full((B, K, w), -7.0) for _, w in OUTPUTS]
    state = np.full(B, -9, np.int32)

    def call(batch=B, layout=layout, n_rows=R, max_advance=0.5, n_knots=K, dt=0.1, rows=True, adv=True, st=True, memory=api.MEM_HOST):
        code, _ = opt.carry_raw(batch, layout, plans.ctypes.data if rows else None, n_rows, advance.ctypes.data if adv else None,
                                max_advance, n_knots, dt, *[o.ctypes.data for o in outs], state.ctypes.data if st else None, memory)
        if code != api.OK:
            assert all((o == -7.0).all() for o in outs) and (state == -9).all()
        return code

    assert call(rows=False) == api.ERR_NULL and call(adv=False) == api.ERR_NULL and call(st=False) == api.ERR_NULL
    assert call(batch=0) == api.ERR_ARG and call(memory=7) == api.ERR_ARG
    assert call(layout=3) == api.ERR_ARG and call(layout=api.ROWS_POINTS) == api.ERR_ARG
    assert call(n_rows=1) == api.ERR_ARG and call(n_knots=0) == api.ERR_ARG and call(dt=0.0) == api.ERR_ARG
    assert call(max_advance=-0.1) == api.ERR_ARG and call(max_advance=float("nan")) == api.ERR_ARG
    assert call(n_rows=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY and call(n_knots=api.DP_MAX_KNOTS + 1) == api.ERR_CAPACITY
    assert call() == api.OK and (state != -9).all()
