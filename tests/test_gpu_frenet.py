"""The Frenet frame of a centre line on the GPU (cilqr_frenet_rows_batch / cilqr_cartesian_points_batch,
kernels_frenet.hip) against the host calls (cilqr_frenet_rows / cilqr_cartesian_points, which tests/test_frenet.py holds
to the reference's own class).

k_frenet: seven of the eight columns and |lateral| bit for bit (resample_cases.same_rows: equal bit patterns, a NaN
matching any NaN).  The SIGN of lateral comes from a cross product whose sin / cos the kernel takes from its own lean
routine, about an ulp off the C library's: it is compared wherever the host's |cross| > 1e-9 |nr|, and the elements under
that bound are counted -- none on random points, exactly the queries that lie ON the line in the crafted table.
k_cartesian: theta bit for bit against the host call; x and y against the NumPy statement with the device library's
cos / sin (cilqr_device_math fn 7 / 8) handed in.

Workgroup geometry (kernels_frenet.hip): 256 lanes; the centre line passes through LDS in tiles of frenet_cases.TILE
points; a lane owns one query below frenet_cases.WIDE_FROM queries per call and four from there on."""
import ctypes as C

import numpy as np
import pytest

import frenet_cases as fc
from resample_cases import same_rows
from cilqr_amd import api, frenet, scenario, scene_io

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
T = fc.TILE


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


@pytest.fixture(scope="module")
def opt():
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=256, cmax=16, max_lane_segments=256) as o:
        yield o


@pytest.fixture(scope="module")
def road():
    return fc.road_center()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_rows(center, xy):
    """the host call on the flattened points: [..., 8]"""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    return api.frenet_rows(center, xy.reshape(-1, 2), api.ROWS_POINTS).reshape(xy.shape[:-1] + (8,))


def host_cross(xy, want):
    """the cross product behind the sign of the host's lateral, and |nr|, from the host's own rows (NumPy's sin / cos: an
    ulp of theirs is nothing against the 1e-9 of the bound)"""
    with np.errstate(all="ignore"):
        nr_x, nr_y = xy[..., 0] - want[..., 2], xy[..., 1] - want[..., 3]
        return nr_y * np.cos(want[..., 4]) - nr_x * np.sin(want[..., 4]), np.abs(want[..., 1])


def compare(got, want, xy, what):
    """every element as the module's docstring says; returns how many elements lie under the bound of the sign"""
    assert got.shape == want.shape, what
    cols = [0, 2, 3, 4, 5, 6, 7]
    bad = ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))
    bad[..., 1] = False
    assert same_rows(got[..., cols], want[..., cols]), (what, np.argwhere(bad)[:5])
    assert same_rows(np.abs(got[..., 1]), np.abs(want[..., 1])), (what, "|lateral|")
    cross, nr = host_cross(xy, want)
    with np.errstate(all="ignore"):
        sure = np.abs(cross) > 1e-9 * nr
    assert np.array_equal(np.signbit(got[..., 1])[sure], np.signbit(want[..., 1])[sure]), (what, "sign of lateral")
    return int(np.count_nonzero(~sure & ~np.isnan(cross)))


def run(opt, center, rows, layout, memory):
    if memory == api.MEM_HOST:
        return opt.frenet(center, rows, layout)
    import torch
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    out = opt.frenet(center, torch.from_numpy(rows).to(dev), layout)
    assert out.is_cuda and out.dtype == torch.float64
    return out.cpu().numpy()


def line_and_points(n_center, B, K, seed):
    """a dyadic line of n_center points and B K points: random ones beside, before and beyond it; every third slot carries
    one of the line's crafted queries in turn.  Returns (center, xy [B,K,2], how many of them lie on the line)"""
    rng = np.random.default_rng(seed)
    center = fc.dyadic_line(n_center, step=1.0, x0=-2.0, y0=1.0)
    Q = B * K
    xy = np.stack([rng.uniform(center[0, 1] - 3.0, center[-1, 1] + 3.0, Q), 1.0 + rng.normal(0, 2.0, Q)], axis=1)
    crafted = fc.line_queries(center)
    on_line = 0
    for q in range(1, Q, 3):
        _, x, y, on = crafted[(q // 3) % len(crafted)]
        xy[q] = x, y
        on_line += int(on)
    return center, xy.reshape(B, K, 2), on_line


SHAPES = [(1, 1), (1, 51), (64, 51), (130, 7), (3, 256)]
N_CENTER = [2, 3, T - 1, T, T + 1, 2 * T + 5]


@pytest.mark.parametrize("n_center", N_CENTER)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d" % s)
def test_kernel_equals_the_host_call(opt, shape, n_center):
    """every output element, in all four layouts, HOST and DEVICE arrays; the crafted queries of the line spread over
    the batch, and exactly those of them that lie on the line fall under the bound of the sign"""
    B, K = shape
    center, xy, on_line = line_and_points(n_center, B, K, seed=1000 * B + K + n_center)
    want = host_rows(center, xy)
    rng = np.random.default_rng(7)
    for layout in fc.LAYOUTS:
        rows = fc.rows_in_layout(layout, xy, rng)
        for memory in (api.MEM_HOST, api.MEM_DEVICE):
            got = run(opt, center, rows, layout, memory)
            assert compare(got, want, xy, (shape, n_center, layout, memory)) == on_line
    if B * K >= 64:      # the batch did carry the crafted queries, NaN and infinite ones included
        assert np.isnan(want).any() and np.isfinite(want).any() and on_line >= 2


def test_crafted_cases_alone(opt):
    """every crafted case as a call of its own (its own centre line, B = 1), every layout; the elements under the bound of
    the sign are the case's on-line queries, counted by name"""
    for case in fc.crafted_cases():
        want = host_rows(case.center, case.points[None])
        for layout in fc.LAYOUTS:
            got = opt.frenet(case.center, fc.rows_in_layout(layout, case.points[None]), layout)
            assert compare(got, want, case.points[None], (case.name, layout)) == case.on_line, case.name
        if case.name == "degenerate pair":      # a copied row: its bits, the negative zero and the unwrapped heading included
            assert np.array_equal(_bits(got[0][:, [0, 2, 3, 4, 5, 6, 7]]), _bits(np.broadcast_to(case.center[4], (len(case.points), 7))))


@pytest.mark.parametrize("memory", [api.MEM_HOST, api.MEM_DEVICE])
def test_random_points_on_the_road_never_fall_under_the_bound_of_the_sign(opt, road, memory):
    """130 x 51 points within 12 m of the generator's road (1952 centre points: three full tiles and a part)"""
    rng = np.random.default_rng(31)
    xy = fc.points_on_road(rng, road, 130 * 51, half_width=12.0).reshape(130, 51, 2)
    want = host_rows(road, xy)
    got = run(opt, road, fc.rows_in_layout(api.ROWS_PLAN, xy, rng), api.ROWS_PLAN, memory)
    assert compare(got, want, xy, "road") == 0
    assert np.isfinite(got).all() and np.array_equal(np.signbit(got[..., 1]), np.signbit(want[..., 1]))


def test_a_call_large_enough_for_four_queries_per_lane(opt):
    """WIDE_FROM + 456 queries: the wide mapping, its last workgroup with one full run, a part of one and two empty ones"""
    B, K = 2600, 101
    assert fc.WIDE_FROM <= B * K < fc.WIDE_FROM + 1024 and (B * K) % 1024 == 456
    center, xy, on_line = line_and_points(T + 1, B, K, seed=77)
    want = host_rows(center, xy)
    got = run(opt, center, fc.rows_in_layout(api.ROWS_PLAN, xy), api.ROWS_PLAN, api.MEM_DEVICE)
    assert compare(got, want, xy, "wide") == on_line
    got = run(opt, center, fc.rows_in_layout(api.ROWS_POINTS, xy), api.ROWS_POINTS, api.MEM_HOST)
    assert compare(got, want, xy, "wide points") == on_line


@pytest.mark.parametrize("memory", [api.MEM_HOST, api.MEM_DEVICE])
def test_arrays_aligned_as_doubles_only_and_nothing_written_outside(opt, memory):
    """rows and frenet are views that start one double into larger arrays (8 bytes off a 16-byte boundary); the doubles
    either side of frenet keep their bits and every element of it is written"""
    for B, K, n_center, layout in ((7, 51, T + 1, api.ROWS_PLAN), (64, 51, 9, api.ROWS_POINTS), (5, 3, 2, api.ROWS_COARSE),
                                   (3, 256, 2 * T + 5, api.ROWS_TRAJ)):
        center, xy, _ = line_and_points(n_center, B, K, seed=17 + B)
        xy = np.nan_to_num(xy, nan=1.25, posinf=2.5, neginf=-2.5)
        rows = fc.rows_in_layout(layout, xy, np.random.default_rng(B))
        want = host_rows(center, xy)
        assert np.isfinite(want).all()
        n_out, guard, offset = B * K * 8, 64, 1
        h_rows = np.full(offset + rows.size + 1, SENTINEL)
        h_rows[offset:offset + rows.size] = rows.ravel()
        h_out = np.full(guard + offset + n_out + guard, SENTINEL)
        first = guard + offset
        if memory == api.MEM_HOST:
            rc_ = opt.frenet_raw(center, B, layout, h_rows.ctypes.data + 8 * offset, K, h_out.ctypes.data + 8 * first, api.MEM_HOST)
            after = h_out
        else:
            import torch
            dev = torch.device("cuda", 0)
            d_rows, d_out = torch.from_numpy(h_rows).to(dev), torch.from_numpy(h_out).to(dev)
            assert d_rows.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
            opt.set_stream(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            rc_ = opt.frenet_raw(center, B, layout, d_rows.data_ptr() + 8 * offset, K, d_out.data_ptr() + 8 * first, api.MEM_DEVICE)
            torch.cuda.synchronize()
            after = d_out.cpu().numpy()
        assert rc_ == api.OK
        sentinel_bits = _bits(np.array([SENTINEL]))[0]
        assert (_bits(after[:first]) == sentinel_bits).all() and (_bits(after[first + n_out:]) == sentinel_bits).all(), (B, K)
        body = after[first:first + n_out]
        assert (_bits(body) != sentinel_bits).all(), (B, K)
        compare(body.reshape(B, K, 8), want, xy, (B, K, layout))


def test_a_nan_trajectory_leaves_its_neighbours_bits_alone(opt, road):
    rng = np.random.default_rng(23)
    B, K = 64, 51
    xy = fc.points_on_road(rng, road, B * K, half_width=3.0).reshape(B, K, 2)
    rows = fc.rows_in_layout(api.ROWS_PLAN, xy, rng)
    before = run(opt, road, rows, api.ROWS_PLAN, api.MEM_DEVICE)
    spoiled = rows.copy()
    spoiled[31] = np.nan
    spoiled[33, :, 2] = np.inf
    spoiled[35][:, [0, 1, 4, 5, 6, 7, 8, 9, 10]] = np.nan        # everything but x and y: not read
    after = run(opt, road, spoiled, api.ROWS_PLAN, api.MEM_DEVICE)
    others = [b for b in range(B) if b not in (31, 33)]
    assert np.array_equal(_bits(after[others]), _bits(before[others]))
    assert not np.isfinite(after[31, :, :2]).any() and not np.isfinite(after[33, :, :2]).any()
    compare(after, host_rows(road, spoiled[:, :, 2:4]), spoiled[:, :, 2:4], "spoiled")


# ---------------------------------------------------------------------------------------------------------------------
# the inverse
# ---------------------------------------------------------------------------------------------------------------------
def _device_trig(opt):
    return lambda theta: (opt.device_math(8, theta), opt.device_math(7, theta))      # fn 8: sin, fn 7: cos


def check_inverse(opt, center, sl, got, what):
    stated = frenet.cartesian_points(center, sl.reshape(-1, 2), trig=_device_trig(opt)).reshape(got.shape)
    host = api.cartesian_points(center, sl.reshape(-1, 2)).reshape(got.shape)
    assert same_rows(got[..., :2], stated[..., :2]), (what, "x, y")
    assert same_rows(got[..., 2], host[..., 2]), (what, "theta")


def test_cartesian_kernel_on_the_crafted_stations(opt):
    import torch
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    for v in fc.inverse_cases():
        check_inverse(opt, v.center, v.sl, opt.cartesian(v.center, v.sl), v.name)
        check_inverse(opt, v.center, v.sl, opt.cartesian(v.center, torch.from_numpy(v.sl).to(dev)).cpu().numpy(), v.name)


@pytest.mark.parametrize("n", [1, 64, 1300])
def test_cartesian_kernel_on_the_road(opt, road, n):
    import torch
    rng = np.random.default_rng(n)
    sl = np.stack([rng.uniform(-5.0, road[-1, 0] + 5.0, n), rng.uniform(-4.0, 4.0, n)], axis=1)
    sl[::7, 0] = road[rng.integers(0, len(road), len(sl[::7])), 0]           # on a knot
    check_inverse(opt, road, sl, opt.cartesian(road, sl), n)
    # views one double into larger arrays, sentinels either side of the output
    dev = torch.device("cuda", 0)
    opt.set_stream(torch.cuda.current_stream().cuda_stream)
    h_sl = np.full(1 + 2 * n + 1, SENTINEL)
    h_sl[1:1 + 2 * n] = sl.ravel()
    d_sl, d_out = torch.from_numpy(h_sl).to(dev), torch.full((64 + 1 + 3 * n + 64,), SENTINEL, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert opt.cartesian_raw(road, n, d_sl.data_ptr() + 8, d_out.data_ptr() + 8 * 65, api.MEM_DEVICE) == api.OK
    after = d_out.cpu().numpy()
    sentinel_bits = _bits(np.array([SENTINEL]))[0]
    assert (_bits(after[:65]) == sentinel_bits).all() and (_bits(after[65 + 3 * n:]) == sentinel_bits).all()
    check_inverse(opt, road, sl, after[65:65 + 3 * n].reshape(n, 3), (n, "views"))
    # there and back: the distance to the original point is what the two rules give, the host calls' to 1e-12 -- the
    # device library's sin / cos are an ulp (1.1e-16) off, times |lateral| <= 2, plus the rounding of x, y up to 200 (3e-14)
    pts = fc.points_on_road(rng, road, n, half_width=2.0)
    fr = opt.frenet(road, pts[None], api.ROWS_POINTS)[0]
    back = opt.cartesian(road, fr[:, :2])
    host_back = api.cartesian_points(road, api.frenet_rows(road, pts)[:, :2])
    assert np.abs(np.hypot(*(back[:, :2] - pts).T) - np.hypot(*(host_back[:, :2] - pts).T)).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the chain on the device: plan rows -> Frenet rows; plan rows -> five times the rate -> Frenet rows
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_rows_are_projected_where_they_lie(opt):
    import torch
    import collision_cases as cc
    dev = torch.device("cuda", 0)
    B, K, MI = 130, opt.K, opt.cfg.max_iter
    sc, sf = cc.generator_scenes("mix11", B, 91)
    center = np.ascontiguousarray(sf.center, dtype=np.float64)
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
    fr = torch.full((B, K, 8), SENTINEL, dtype=torch.float64, device=dev)
    assert opt.frenet_raw(center, B, api.ROWS_PLAN, plan.data_ptr(), K, fr.data_ptr(), api.MEM_DEVICE) == api.OK
    plan_h, fr_h = plan.cpu().numpy(), fr.cpu().numpy()
    assert np.array_equal(_bits(fr_h), _bits(opt.frenet(center, plan_h, api.ROWS_PLAN)))        # the downloaded rows, HOST arrays
    compare(fr_h, host_rows(center, plan_h[:, :, 2:4]), plan_h[:, :, 2:4], "plan rows")
    ok = outcome.cpu().numpy() == api.PLAN_OK
    assert ok.any() and np.isfinite(fr_h[ok]).all() and (_bits(fr_h) != _bits(np.array([SENTINEL]))[0]).all()
    # the solver's traj rows of the same batch
    fr_traj = torch.full((B, K, 8), SENTINEL, dtype=torch.float64, device=dev)
    assert opt.frenet_raw(center, B, api.ROWS_TRAJ, traj.data_ptr(), K, fr_traj.data_ptr(), api.MEM_DEVICE) == api.OK
    traj_h = traj.cpu().numpy()
    compare(fr_traj.cpu().numpy(), host_rows(center, traj_h[:, :, 1:3]), traj_h[:, :, 1:3], "traj rows")
    # the same batch at five times the knot rate, resampled and projected on the device
    M = 5 * (K - 1) + 1
    axis = np.arange(M) * dp_cfg.delta_t / 5
    d_axis = torch.from_numpy(axis).to(dev)
    fine = torch.full((B, M, api.PLAN_FIELDS), SENTINEL, dtype=torch.float64, device=dev)
    assert opt.resample_raw(B, api.ROWS_PLAN, plan.data_ptr(), K, api.KEY_TIME, d_axis.data_ptr(), M, False, fine.data_ptr(),
                            api.MEM_DEVICE) == api.OK
    fr_fine = torch.full((B, M, 8), SENTINEL, dtype=torch.float64, device=dev)
    assert opt.frenet_raw(center, B, api.ROWS_PLAN, fine.data_ptr(), M, fr_fine.data_ptr(), api.MEM_DEVICE) == api.OK
    fine_h = fine.cpu().numpy()
    compare(fr_fine.cpu().numpy(), host_rows(center, fine_h[:, :, 2:4]), fine_h[:, :, 2:4], "plan rows at 5x")


# ---------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing_and_leave_the_handle_usable(opt):
    B, K = 16, 51
    center, xy, _ = line_and_points(T + 1, B, K, seed=5)
    rows = fc.rows_in_layout(api.ROWS_PLAN, xy)
    reference = host_rows(center, xy)
    sl = np.ascontiguousarray(np.nan_to_num(reference[..., :2].reshape(-1, 2), nan=1.0, posinf=2.0, neginf=-2.0))
    L = api.lib()

    def good():      # successful calls on the same handle
        compare(opt.frenet(center, rows, api.ROWS_PLAN), reference, xy, "good")
        check_inverse(opt, center, sl, opt.cartesian(center, sl), "good")
        return True

    def project(handle=True, n_center=T + 1, batch=B, layout=api.ROWS_PLAN, n_knots=K, memory=api.MEM_HOST, want_center=True,
                want_rows=True, want_out=True, alias=None):
        block = np.full(rows.size + B * K * 8, -7.0)
        block[:rows.size] = rows.ravel()
        out = np.full((B, K, 8), -7.0)
        r, o = rows.ctypes.data, out.ctypes.data
        if alias == "rows":
            r, o = block.ctypes.data, block.ctypes.data + 8 * (rows.size - 1)
        elif alias == "center":
            o = center.ctypes.data + 8 * (center.size - 1)
        before = center.copy()
        code = L.cilqr_frenet_rows_batch(opt.h if handle else None, center.ctypes.data if want_center else None, n_center, batch,
                                         layout, r if want_rows else None, n_knots, o if want_out else None, memory)
        if code != api.OK:    # nothing was launched, nothing written
            assert (out == -7.0).all() and (block[rows.size:] == -7.0).all() and np.array_equal(center, before)
        return code

    def inverse(handle=True, n_center=T + 1, n=len(sl), memory=api.MEM_HOST, want_center=True, want_sl=True, want_out=True, alias=None):
        block = np.full(sl.size + 3 * len(sl), -7.0)
        block[:sl.size] = sl.ravel()
        out = np.full((len(sl), 3), -7.0)
        s, o = sl.ctypes.data, out.ctypes.data
        if alias == "sl":
            s, o = block.ctypes.data, block.ctypes.data + 8 * (sl.size - 1)
        elif alias == "center":
            o = center.ctypes.data
        before = center.copy()
        code = L.cilqr_cartesian_points_batch(opt.h if handle else None, center.ctypes.data if want_center else None, n_center, n,
                                              s if want_sl else None, o if want_out else None, memory)
        if code != api.OK:
            assert (out == -7.0).all() and (block[sl.size:] == -7.0).all() and np.array_equal(center, before)
        return code

    assert project() == api.OK and inverse() == api.OK
    for what in ("handle", "want_center", "want_rows", "want_out"):
        assert project(**{what: False}) == api.ERR_NULL and good(), what
    for what in ("handle", "want_center", "want_sl", "want_out"):
        assert inverse(**{what: False}) == api.ERR_NULL and good(), what
    for bad in (dict(n_center=1), dict(n_center=0), dict(n_center=-3), dict(batch=0), dict(batch=-2), dict(n_knots=0), dict(n_knots=-1),
                dict(layout=3), dict(layout=5), dict(layout=-1), dict(memory=2), dict(memory=-1), dict(alias="rows"), dict(alias="center")):
        assert project(**bad) == api.ERR_ARG and good(), bad
    for bad in (dict(n_center=1), dict(n_center=-1), dict(n=0), dict(n=-4), dict(memory=2), dict(memory=-1), dict(alias="sl"),
                dict(alias="center")):
        assert inverse(**bad) == api.ERR_ARG and good(), bad
    for layout in fc.LAYOUTS:
        assert project(layout=layout, batch=1, n_knots=1) == api.OK
    assert project(n_center=2) == api.OK and inverse(n_center=2, n=1) == api.OK
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
        for call in (lambda: busy.frenet(center, rows, api.ROWS_PLAN), lambda: busy.cartesian(center, sl)):
            with pytest.raises(api.CilqrError) as e:
                call()
            assert e.value.code == api.ERR_STATE
        assert busy.L.cilqr_wait(busy.h) == api.OK
        compare(busy.frenet(center, rows, api.ROWS_PLAN), reference, xy, "after the wait")
        # ... and the solve's own rows on the generator's road
        road = fc.road_center()
        compare(busy.frenet(road, traj, api.ROWS_TRAJ), host_rows(road, traj[:, :, 1:3]), traj[:, :, 1:3], "solved rows")
    assert good()
