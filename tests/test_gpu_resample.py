"""Resampling of trajectory rows on the GPU (cilqr_resample_rows_batch, kernels_resample.hip) against the host call
(cilqr_resample_rows, which tests/test_resample.py holds to the reference's own class): every output element bit for bit.

"Bit for bit" is resample_cases.same_rows: equal bit patterns, a NaN matching any NaN -- which NaN an arithmetic
operation returns is the processor's choice (x86 and gfx950 differ in the sign of the NaN that inf - inf creates), not
the rule's.  What the rule COPIES -- the two control columns, the whole row of a degenerate pair -- is compared as bits
without that allowance.

Workgroup geometry (kernels_resample.hip): a workgroup takes min(3072 / (K F), ceil(2048 / M)) whole problems and works
through their (problem, query) items in tiles of 256; more than 2048 items per run split over the grid's second dimension.
The shapes below put batch ends inside a run (64 problems in runs of 5; 1300 in runs of 139), take one problem per run
(K = 256), more than one tile per run, a run split in two (3 x 1000 items), M = 1 and B = M = 1."""
import ctypes as C

import numpy as np
import pytest

import resample_cases as rc
from cilqr_amd import api, resample, scenario, scene_io

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=128, cmax=16, max_lane_segments=256) as o:
        yield o


@pytest.fixture(scope="module")
def crafted():
    return rc.crafted_cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _embed(case, K, rng):
    """the crafted rows as the LAST rows of a K-row trajectory: filler rows with smaller, increasing keys in front"""
    n = len(case.plan)
    if n == K:
        return case.plan.copy()
    first = np.nanmin(case.plan[:, 0])
    keys = first - 10.0 - np.arange(K - n, 0, -1) * 0.05
    return np.concatenate([rc.smooth_plan(rng, keys), case.plan], axis=0)


def make_batch(crafted, B, K, M, per_problem, seed):
    """plans [B,K,11], queries [M] or [B,M]; every third problem carries a crafted case (those with at most K rows, in
    turn), with per-problem axes its crafted queries too; a shared axis carries crafted queries of all of them"""
    rng = np.random.default_rng(seed)
    fits = [c for c in crafted if len(c.plan) <= K]
    plans = np.zeros((B, K, 11))
    queries = np.zeros((B, M))
    carried = []
    for b in range(B):
        case = fits[(b // 3) % len(fits)] if (b % 3 == 1 and fits) else None
        if case is not None:
            plans[b] = _embed(case, K, rng)
            cq = case.queries
            carried.append(cq)
        else:
            keys = np.cumsum(rng.uniform(0.02, 0.2, K)) + rng.uniform(1.0, 2.5)
            theta = np.cumsum(rng.uniform(-0.5, 0.5, K)) + rng.uniform(-7.0, 7.0) if b % 2 else None
            plans[b] = rc.smooth_plan(rng, keys, theta)
            cq = plans[b, rng.integers(0, K, 2), 0]
        lo, hi = np.nanmin(plans[b, :, 0]), np.nanmax(plans[b, :, 0])
        q = rng.uniform(lo - 0.2, hi + 0.2, M)
        n = min(M, len(cq))
        q[:n] = cq[:n]
        queries[b] = q
    if per_problem:
        return plans, queries
    shared = rng.uniform(-0.5, 6.0, M)
    pool = np.concatenate(carried) if carried else np.zeros(0)
    n = min(M // 2, len(pool))
    shared[:n] = pool[rng.permutation(len(pool))[:n]]
    return plans, shared


def host_rows(rows, layout, queries, key):
    """the host call, problem by problem: [B,M,F]"""
    per = queries.ndim == 2
    return np.stack([api.resample_rows(rows[b], layout, queries[b] if per else queries, key) for b in range(rows.shape[0])])


def check(got, want, rows, layout, queries, key, what):
    assert got.shape == want.shape, what
    assert rc.same_rows(got, want), (what, np.argwhere(~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))[:5])
    _, _, _, _, c_ctrl = resample.COLUMNS[layout]
    if c_ctrl is not None:     # copied values: their bits, NaN or not
        assert np.array_equal(_bits(got[:, :, c_ctrl:]), _bits(want[:, :, c_ctrl:])), what


def run(opt, rows, layout, queries, key, memory):
    if memory == api.MEM_HOST:
        return opt.resample(rows, layout, queries, key)
    import torch
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    out = opt.resample(torch.from_numpy(rows).to(dev), layout, torch.from_numpy(np.ascontiguousarray(queries)).to(dev), key)
    assert out.is_cuda and out.dtype == torch.float64
    return out.cpu().numpy()


# B, K, M, layout, key, per-problem axes, memory
SHAPES = [
    (1, 2, 1, api.ROWS_PLAN, api.KEY_TIME, False, api.MEM_HOST),
    (1, 51, 7, api.ROWS_PLAN, api.KEY_STATION, True, api.MEM_DEVICE),          # B M F = 77 doubles: odd
    (64, 51, 251, api.ROWS_PLAN, api.KEY_TIME, False, api.MEM_DEVICE),         # runs of 5, the last one of 4; 5 tiles per run
    (130, 256, 7, api.ROWS_PLAN, api.KEY_STATION, True, api.MEM_DEVICE),       # one problem per run
    (130, 256, 257, api.ROWS_COARSE, api.KEY_TIME, False, api.MEM_HOST),
    (1300, 2, 7, api.ROWS_TRAJ, api.KEY_TIME, True, api.MEM_HOST),             # runs of 139, the last one of 49
    (1300, 51, 1, api.ROWS_PLAN, api.KEY_TIME, True, api.MEM_DEVICE),          # M = 1: runs of 5 items
    (64, 2, 1000, api.ROWS_COARSE, api.KEY_STATION, False, api.MEM_DEVICE),    # runs of 3 = 3000 items: two workgroups each
    (130, 51, 1000, api.ROWS_TRAJ, api.KEY_TIME, True, api.MEM_DEVICE),
    (1, 256, 257, api.ROWS_TRAJ, api.KEY_TIME, False, api.MEM_DEVICE),
    (64, 51, 7, api.ROWS_COARSE, api.KEY_TIME, True, api.MEM_HOST),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d-M%d-l%d-k%d-p%d-m%d" % tuple(int(v) for v in s))
def test_kernel_equals_the_host_call_bit_for_bit(opt, crafted, shape):
    B, K, M, layout, key, per_problem, memory = shape
    plans, queries = make_batch(crafted, B, K, M, per_problem, seed=B * 1000 + K + M)
    rows = rc.rows_in_layout(layout, plans)
    want = host_rows(rows, layout, queries, key)
    got = run(opt, rows, layout, queries, key, memory)
    check(got, want, rows, layout, queries, key, shape)
    if B >= 64 and K >= 11:      # the batch did carry the crafted table, its NaN cases included
        assert np.isnan(want).any() and np.isfinite(want).any()


def test_crafted_cases_alone(opt, crafted):
    """every crafted case as a batch of its own (B = 1, its own K), every layout and key, HOST arrays: against the host call
    and -- kernel and host call run one pair step (include/cilqr/row_math.hpp), so a wrong one agrees with itself --
    against the NumPy statement"""
    for case in crafted:
        for layout in rc.LAYOUTS:
            rows = rc.rows_in_layout(layout, case.plan)[None]
            for key in rc.KEYS_OF[layout]:
                want = host_rows(rows, layout, case.queries, key)
                got = opt.resample(rows, layout, case.queries, key)
                check(got, want, rows, layout, case.queries, key, (case.name, layout, key))
                stated = resample.resample_rows(rows[0], layout, case.queries, key)[None]
                check(got, stated, rows, layout, case.queries, key, (case.name, layout, key, "NumPy statement"))
                if "degenerate" in case.branches:    # a copied row: its bits
                    deg = [m for m, q in enumerate(case.queries) if resample.branch_of(rows[0], layout, q, key) == "degenerate"]
                    assert deg and np.array_equal(_bits(got[0, deg]), _bits(want[0, deg])), case.name


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("memory", [api.MEM_HOST, api.MEM_DEVICE])
def test_arrays_aligned_as_doubles_only_and_nothing_written_outside(opt, crafted, offset, memory):
    """rows, queries and out are views that start `offset` doubles into larger arrays (offset 1: 8 bytes off a 16-byte
    boundary); the doubles either side of out keep their bits and every element of out is written"""
    for B, K, M, layout in ((7, 51, 9, api.ROWS_PLAN), (64, 51, 251, api.ROWS_PLAN), (5, 2, 3, api.ROWS_COARSE)):
        F = api.ROWS_FIELDS[layout]
        plans, queries = make_batch(crafted, B, K, M, True, seed=17 + B)
        plans, queries = np.nan_to_num(plans, nan=1.25, posinf=2.5), np.nan_to_num(queries, nan=0.75, posinf=3.0, neginf=-3.0)
        rows = rc.rows_in_layout(layout, plans)
        want = host_rows(rows, layout, queries, api.KEY_TIME)
        assert np.isfinite(want).all()
        n_out, guard = B * M * F, 64
        h_rows = np.full(offset + rows.size + 1, SENTINEL)
        h_rows[offset:offset + rows.size] = rows.ravel()
        h_q = np.full(offset + queries.size + 1, SENTINEL)
        h_q[offset:offset + queries.size] = queries.ravel()
        h_out = np.full(guard + offset + n_out + guard, SENTINEL)
        first = guard + offset
        if memory == api.MEM_HOST:
            rc_ = opt.resample_raw(B, layout, h_rows.ctypes.data + 8 * offset, K, api.KEY_TIME, h_q.ctypes.data + 8 * offset, M, True,
                                   h_out.ctypes.data + 8 * first, api.MEM_HOST)
            after = h_out
        else:
            import torch
            dev = torch.device("cuda", 0)
            d_rows, d_q, d_out = (torch.from_numpy(a).to(dev) for a in (h_rows, h_q, h_out))
            assert d_rows.data_ptr() % 16 == 0 and d_q.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
            opt.set_stream(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            rc_ = opt.resample_raw(B, layout, d_rows.data_ptr() + 8 * offset, K, api.KEY_TIME, d_q.data_ptr() + 8 * offset, M, True,
                                   d_out.data_ptr() + 8 * first, api.MEM_DEVICE)
            torch.cuda.synchronize()
            after = d_out.cpu().numpy()
        assert rc_ == api.OK
        sentinel_bits = _bits(np.array([SENTINEL]))[0]
        assert (_bits(after[:first]) == sentinel_bits).all() and (_bits(after[first + n_out:]) == sentinel_bits).all(), (B, K, M)
        body = after[first:first + n_out]
        assert (_bits(body) != sentinel_bits).all(), (B, K, M)
        assert np.array_equal(_bits(body.reshape(B, M, F)), _bits(want)), (B, K, M)


def test_a_nan_trajectory_leaves_its_neighbours_bits_alone(opt, crafted):
    B, K, M, layout = 64, 51, 7, api.ROWS_PLAN
    plans, queries = make_batch(crafted, B, K, M, True, seed=23)
    rows = rc.rows_in_layout(layout, plans)
    before = run(opt, rows, layout, queries, api.KEY_TIME, api.MEM_DEVICE)
    spoiled = rows.copy()
    spoiled[31] = np.nan              # inside a run of five problems (30 ... 34)
    spoiled[33, :, 4] = np.inf
    after = run(opt, spoiled, layout, queries, api.KEY_TIME, api.MEM_DEVICE)
    others = [b for b in range(B) if b not in (31, 33)]
    assert np.array_equal(_bits(after[others]), _bits(before[others]))
    assert np.isnan(after[31, :, 1:9]).all() and np.array_equal(after[31, :, 0], queries[31])     # the key column is the query
    check(after, host_rows(spoiled, layout, queries, api.KEY_TIME), spoiled, layout, queries, api.KEY_TIME, "spoiled")
    # a NaN query on a shared axis spoils its own column of the output only
    shared = queries[0].copy()
    shared[3] = np.nan
    got = run(opt, rows, layout, shared, api.KEY_TIME, api.MEM_DEVICE)
    check(got, host_rows(rows, layout, shared, api.KEY_TIME), rows, layout, shared, api.KEY_TIME, "NaN query")
    clean = [b for b in range(B) if np.isfinite(rows[b]).all()]
    assert np.isfinite(got[clean][:, [0, 1, 2, 4, 5, 6]]).all() and np.isnan(got[clean][:, 3, :9]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the chain on the device: plan rows -> five times the rate -> collision audit
# ---------------------------------------------------------------------------------------------------------------------
def _audit_device(opt, packed, cfg, d_rows_ptr, B, n_knots):
    import torch
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    mask = torch.full((B, n_knots), 77, dtype=torch.uint8, device=dev)
    first, n_hit = (torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    rc_, n = opt.check_collisions_raw(cfg, sb, api.ROWS_PLAN, d_rows_ptr, n_knots, 0.0, mask.data_ptr(), first.data_ptr(), n_hit.data_ptr())
    torch.cuda.synchronize()
    assert rc_ == api.OK
    return dict(mask=mask.cpu().numpy(), first_hit=first.cpu().numpy(), n_hit=n_hit.cpu().numpy(), n_colliding=n)


def test_plan_rows_resampled_on_the_device_feed_the_audit_where_they_lie(opt):
    import torch
    import collision_cases as cc
    dev = torch.device("cuda", 0)
    B, K, MI = 64, opt.K, opt.cfg.max_iter
    sc, sf = cc.generator_scenes("mix11", B, 91)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    dp_cfg, cor_cfg = api.default_dp_config(tf=5.0), api.default_corridor_config()
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    start = torch.from_numpy(np.ascontiguousarray(sc["start"])).to(dev)
    traj = torch.zeros((B, K, 10), dtype=torch.float64, device=dev)
    hist = torch.zeros((B, MI + 1, 5), dtype=torch.float64, device=dev)
    plan = torch.zeros((B, K, api.PLAN_FIELDS), dtype=torch.float64, device=dev)
    n_cost, status, n_iter, outcome = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                            n_iter.data_ptr(), None, None, None)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rc_, _, _ = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb, start.data_ptr(), K, sol, plan.data_ptr(), None, outcome.data_ptr())
    assert rc_ == api.OK
    M = 5 * (K - 1) + 1
    axis = np.arange(M) * dp_cfg.delta_t / 5
    d_axis = torch.from_numpy(axis).to(dev)
    fine = torch.full((B, M, api.PLAN_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
    assert opt.resample_raw(B, api.ROWS_PLAN, plan.data_ptr(), K, api.KEY_TIME, d_axis.data_ptr(), M, False, fine.data_ptr(),
                            api.MEM_DEVICE) == api.OK
    got = _audit_device(opt, packed, dp_cfg, fine.data_ptr(), B, M)
    # the same rows resampled on the host and uploaded: one audit
    plan_h = plan.cpu().numpy()
    fine_h = host_rows(plan_h, api.ROWS_PLAN, axis, api.KEY_TIME)
    check(fine.cpu().numpy(), fine_h, plan_h, api.ROWS_PLAN, axis, api.KEY_TIME, "plan rows at 5x")
    up = torch.from_numpy(fine_h).to(dev)
    want = _audit_device(opt, packed, dp_cfg, up.data_ptr(), B, M)
    assert all(np.array_equal(got[k], want[k]) for k in ("mask", "first_hit", "n_hit")) and got["n_colliding"] == want["n_colliding"]
    assert (got["mask"] != 77).all() and (got["first_hit"] >= -1).all()


def test_an_obstacle_between_two_knots_is_seen_at_five_times_the_rate(opt):
    """One constructed scene: the vehicle drives along a straight road at 10 m/s, knots 0.1 s apart; a square stands on its
    path at the place the vehicle reaches at t = 0.55, with samples at 0.535, 0.55 and 0.565 only.  At every knot the
    obstacle is absent by the audit's own rule (time[0] > t at 0.5, time[T-1] < t at 0.6): first_hit = -1.  Resampled at
    0.02 s the rows at 0.54 and 0.56 meet it: rows 27 and 28."""
    import torch
    import collision_cases as cc
    dev = torch.device("cuda", 0)
    cfg = api.default_dp_config()
    center = cc.straight_center(length=60.0)
    K, dt = 11, 0.1
    times = np.arange(K) * dt
    plan_h = np.zeros((1, K, api.PLAN_FIELDS))
    plan_h[0, :, 0], plan_h[0, :, 1], plan_h[0, :, 2], plan_h[0, :, 6] = times, 10.0 * times, 5.0 + 10.0 * times, 10.0
    square = np.array([[0.5, 0.5], [0.5, -0.5], [-0.5, -0.5], [-0.5, 0.5]])
    samples = np.array([[0.535, 10.5, 0.0, 0.0], [0.55, 10.5, 0.0, 0.0], [0.565, 10.5, 0.0, 0.0]])
    scene = scene_io.Scene(np.zeros(4), np.zeros((1, 6)), [], [scene_io.DynamicObstacle(square, samples)])
    packed = scene_io.pack_scene_batch(center, [scene])
    M = 5 * (K - 1) + 1
    axis = np.arange(M) * dt / 5
    d_plan, d_axis = torch.from_numpy(plan_h).to(dev), torch.from_numpy(axis).to(dev)
    fine = torch.full((1, M, api.PLAN_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert opt.resample_raw(1, api.ROWS_PLAN, d_plan.data_ptr(), K, api.KEY_TIME, d_axis.data_ptr(), M, False, fine.data_ptr(),
                            api.MEM_DEVICE) == api.OK
    at_knots = _audit_device(opt, packed, cfg, d_plan.data_ptr(), 1, K)
    at_fine = _audit_device(opt, packed, cfg, fine.data_ptr(), 1, M)
    assert at_knots["first_hit"][0] == -1 and at_knots["n_hit"][0] == 0 and at_knots["n_colliding"] == 0
    assert at_fine["first_hit"][0] == 27 and list(np.flatnonzero(at_fine["mask"][0])) == [27, 28] and at_fine["n_colliding"] == 1
    assert at_fine["mask"][0, 27] & (api.HIT_REAR_DYNAMIC | api.HIT_FRONT_DYNAMIC)
    # both verdicts by the NumPy statement of the audit, on the host-resampled rows
    fine_h = host_rows(plan_h, api.ROWS_PLAN, axis, api.KEY_TIME)
    assert np.array_equal(_bits(fine.cpu().numpy()), _bits(fine_h))
    m_knots, f_knots, _ = scene_io.environment_collisions(center, scene, cfg, times, plan_h[0][:, 2:5], 0.0)
    m_fine, f_fine, n_fine = scene_io.environment_collisions(center, scene, cfg, fine_h[0][:, 0], fine_h[0][:, 2:5], 0.0)
    assert f_knots == -1 and not m_knots.any()
    assert f_fine == 27 and n_fine == 2 and np.array_equal(m_fine, at_fine["mask"][0])


# ---------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing_and_leave_the_handle_usable(opt, crafted):
    B, K, M = 16, 51, 9
    plans, queries = make_batch(crafted, B, K, M, True, seed=5)
    big = rc.smooth_plan(np.random.default_rng(6), np.arange(api.DP_MAX_KNOTS + 1) * 0.1)
    L = api.lib()
    reference = host_rows(rc.rows_in_layout(api.ROWS_PLAN, plans), api.ROWS_PLAN, queries, api.KEY_TIME)

    def good():      # a successful call on the same handle
        got = opt.resample(rc.rows_in_layout(api.ROWS_PLAN, plans), api.ROWS_PLAN, queries, api.KEY_TIME)
        assert rc.same_rows(got, reference)
        return True

    def call(handle=True, batch=B, layout=api.ROWS_PLAN, n_knots=K, key=api.KEY_TIME, n_queries=M, per_problem=1,
             memory=api.MEM_HOST, want_rows=True, want_queries=True, want_out=True, alias=False):
        use = layout if layout in rc.LAYOUTS else api.ROWS_PLAN
        rows = rc.rows_in_layout(use, np.broadcast_to(big, (B,) + big.shape)) if n_knots > K else rc.rows_in_layout(use, plans)
        out = np.full((B, max(n_queries, 1), 11), -7.0)
        code = L.cilqr_resample_rows_batch(opt.h if handle else None, batch, layout, rows.ctypes.data if want_rows else None,
                                           n_knots, key, queries.ctypes.data if want_queries else None, n_queries, per_problem,
                                           (rows.ctypes.data if alias else out.ctypes.data) if want_out else None, memory)
        if code != api.OK:    # nothing was launched, nothing written
            assert (out == -7.0).all()
        return code

    assert call() == api.OK
    for what in ("handle", "want_rows", "want_queries", "want_out"):
        assert call(**{what: False}) == api.ERR_NULL and good(), what
    for bad in (dict(batch=0), dict(batch=-2), dict(n_knots=1), dict(n_knots=0), dict(n_knots=-1), dict(n_queries=0),
                dict(n_queries=-5), dict(layout=3), dict(layout=-1), dict(layout=api.ROWS_CONTROLS), dict(key=2), dict(key=-1),
                dict(memory=2), dict(memory=-1), dict(layout=api.ROWS_TRAJ, key=api.KEY_STATION), dict(per_problem=2),
                dict(per_problem=-1), dict(alias=True)):
        assert call(**bad) == api.ERR_ARG and good(), bad
    assert call(n_knots=api.DP_MAX_KNOTS, n_queries=1) == api.OK
    assert call(n_knots=api.DP_MAX_KNOTS + 1, n_queries=1) == api.ERR_CAPACITY and good()
    assert call(layout=api.ROWS_COARSE, key=api.KEY_STATION) == api.OK and call(per_problem=0) == api.OK
    # solves submitted on the handle
    g = scenario.generate("mix11", 64, seed=3)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=64, cmax=g["cmax"]) as busy:
        prob, keep_p = busy._host_problem(g)
        Bs, MI = 64, busy.cfg.max_iter
        traj, hist = np.zeros((Bs, 51, 10)), np.zeros((Bs, MI + 1, 5))
        nc, st, ni = (np.zeros(Bs, dtype=np.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_HOST, 0, traj.ctypes.data, hist.ctypes.data, nc.ctypes.data, st.ctypes.data,
                                ni.ctypes.data, None, None, None)
        assert busy.L.cilqr_submit(busy.h, C.byref(prob), C.byref(sol)) == api.OK
        with pytest.raises(api.CilqrError) as e:
            busy.resample(rc.rows_in_layout(api.ROWS_PLAN, plans), api.ROWS_PLAN, queries, api.KEY_TIME)
        assert e.value.code == api.ERR_STATE
        assert busy.L.cilqr_wait(busy.h) == api.OK
        assert rc.same_rows(busy.resample(rc.rows_in_layout(api.ROWS_PLAN, plans), api.ROWS_PLAN, queries, api.KEY_TIME), reference)
        # ... and the solve's own rows on the finer axis
        fine = busy.resample(traj, api.ROWS_TRAJ, np.arange(251) * 0.02, api.KEY_TIME)
        assert rc.same_rows(fine, host_rows(traj, api.ROWS_TRAJ, np.arange(251) * 0.02, api.KEY_TIME))
    assert good()
