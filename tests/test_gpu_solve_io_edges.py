"""The edges of a solve's staging (cilqr_amd/csrc/solve_io.hpp, solver.hip: stage_inputs, job_begin, job_finish; multi.hip):
HOST batches either side of the 4 MiB that separate one pinned block from array-by-array copies, on the way in and on the
way out independently, and sub-ranges of a batch cut at its first and its last problem (lane groups, shards).

The reference of every comparison is the synchronous solve of the same problems from DEVICE arrays on a handle of the same
configuration, bit for bit: the kernels do not know where their arrays came from.

Scenes: the first B of scenario.generate("mix11", 200, seed=3), N = 50, cmax 16 -- all different, so an array that reaches
a neighbouring problem shows."""
import numpy as np
import pytest

from cilqr_amd import api, scenario

pytestmark = pytest.mark.gpu

N, K, CMAX, M = 50, 51, 16, 200
SMALL = 4 << 20          # bytes up to which a HOST batch travels as one pinned block, each way
SHIFTS = np.asarray([0, -1, 3, 0, N + 1, 1, 0, -1, 0, 12, 0], np.int32)   # a mixed shift array: warm, cold, beyond the horizon


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


_S = {}


def _shared():
    """200 scenes, their cold trajectories (the warm rows of every warm case) and one handle per init guess"""
    if not _S:
        _S["sc"] = scenario.generate("mix11", 200, seed=3)
        _S["opt"] = {init: api.BatchIlqrOptimizer(api.default_config(N, init_guess=init), batch_capacity=256, cmax=CMAX)
                     for init in (api.INIT_IQR, api.INIT_TRACKER)}
        _S["cold"] = _S["opt"][api.INIT_IQR].plan(_S["sc"])["traj"]
    return _S


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for o in _S.get("opt", {}).values():
        o.close()
    _S.clear()


def _batch(B, station=False, warm=False):
    """the first B scenes as the arrays a solve is handed: (scene dict, warm tuple or None)"""
    s = _shared()
    sc = {k: (np.ascontiguousarray(v[:B]) if k in ("start", "coarse", "corridor", "ccount") else v) for k, v in s["sc"].items()}
    sc["ccount"] = sc["ccount"].astype(np.int32)
    if station:   # 1 % longer than the chord lengths a NULL column stands for: a column that does not arrive shows
        step = np.hypot(np.diff(sc["coarse"][:, :, 0], axis=1), np.diff(sc["coarse"][:, :, 1], axis=1))
        sc["coarse_station"] = np.ascontiguousarray(1.01 * np.concatenate([np.zeros((B, 1)), np.cumsum(step, axis=1)], axis=1))
    w = (np.ascontiguousarray(s["cold"][:B]), np.resize(SHIFTS, B), api.ROWS_TRAJ) if warm else None
    return sc, w


def _in_arrays(sc, w):
    a = [sc["start"], sc["coarse"], sc["corridor"], sc["ccount"]]
    if "coarse_station" in sc:
        a.append(sc["coarse_station"])
    return a + ([w[0], w[1]] if w is not None else [])


def _in_bytes(sc, w):
    return sum(a.nbytes for a in _in_arrays(sc, w))


def _out_bytes(g):
    return sum(g[k].nbytes for k in ("traj", "cost_hist", "n_cost", "status", "n_iter", "n_iter_trajs", "iter_trajs", "alpha_trace")
               if g.get(k) is not None)


def _device_reference(opt, sc, w, cap):
    """cilqr_solve_batch(_warm) of the same problems with every array in device memory"""
    import torch
    dev = torch.device("cuda", 0)
    B = sc["coarse"].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = {k: up(sc[k]) for k in ("start", "coarse", "corridor", "ccount")}
    left, right = np.ascontiguousarray(sc["left"], np.float64), np.ascontiguousarray(sc["right"], np.float64)
    prob = api.ProblemBatch(B, K, CMAX, api.MEM_DEVICE, t["start"].data_ptr(), t["coarse"].data_ptr(), t["corridor"].data_ptr(),
                            t["ccount"].data_ptr(), left.shape[0], right.shape[0], left.ctypes.data, right.ctypes.data)
    if "coarse_station" in sc:
        t["station"] = up(sc["coarse_station"])
        prob.coarse_station = t["station"].data_ptr()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    o = dict(traj=z((B, K, 10), torch.float64), cost_hist=z((B, M + 1, 5), torch.float64), n_cost=z(B, torch.int32),
             status=z(B, torch.int32), n_iter=z(B, torch.int32), iter_trajs=z((B, cap, K, 10), torch.float64),
             n_iter_trajs=z(B, torch.int32), alpha_trace=torch.full((B, M), -3, dtype=torch.int8, device=dev))
    sol = api.SolutionBatch(api.MEM_DEVICE, cap, o["traj"].data_ptr(), o["cost_hist"].data_ptr(), o["n_cost"].data_ptr(),
                            o["status"].data_ptr(), o["n_iter"].data_ptr(), o["iter_trajs"].data_ptr(),
                            o["n_iter_trajs"].data_ptr(), o["alpha_trace"].data_ptr())
    wd, keep = (None, None) if w is None else api.make_warm((up(w[0]), up(w[1]), w[2]))
    torch.cuda.synchronize()
    assert opt.solve_raw(prob, sol, wd) == api.OK
    torch.cuda.synchronize()
    del keep
    return {k: v.cpu().numpy() for k, v in o.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same(g, ref, cap, what):
    """trajectories, counts, alpha trace; the live cost rows and zeros behind them; the iterates below the count"""
    for k in ("traj", "n_cost", "status", "n_iter", "n_iter_trajs", "alpha_trace"):
        assert np.array_equal(_bits(g[k]), _bits(ref[k])), (what, k)
    assert (ref["status"] >= 1).all() and (ref["n_cost"] >= 1).all(), what   # (the reference did solve)
    live = np.arange(M + 1)[None, :] < np.clip(ref["n_cost"], 0, M + 1)[:, None]
    assert np.array_equal(_bits(g["cost_hist"])[live], _bits(ref["cost_hist"])[live]), (what, "live cost rows")
    assert not _bits(g["cost_hist"])[~live].any(), (what, "cost rows behind the live ones")
    held = np.arange(cap)[None, :] < np.clip(ref["n_iter_trajs"], 0, cap)[:, None]
    assert held.any(), what
    assert np.array_equal(_bits(g["iter_trajs"])[held], _bits(ref["iter_trajs"])[held]), (what, "iterates")


def _host(opt, sc, w, cap, submit=False):
    if submit:
        return opt.collect(opt.submit(sc, max_iter_trajs=cap, alpha_trace=True, warm=w))
    return opt.plan(sc, max_iter_trajs=cap, alpha_trace=True, warm=w)


@pytest.mark.parametrize("way", ["plain", "warm", "tracker", "submit"])
def test_either_side_of_the_input_boundary(way):
    """B = the most problems whose arrays sum to at most 4 MiB (one pinned block, one copy), then one more (array by array,
    for a submitted solve through the transfer thread): plain, with warm rows and a mixed shift array, with the tracker init
    guess and a station column, and submitted.  The outputs stay below 4 MiB throughout."""
    opt = _shared()["opt"][api.INIT_TRACKER if way == "tracker" else api.INIT_IQR]
    one, w_one = _batch(1, station=way == "tracker", warm=way == "warm")
    B0 = SMALL // _in_bytes(one, w_one)
    if way in ("plain", "submit"):
        assert B0 == 188
    cap = 2
    for B in (B0, B0 + 1):
        sc, w = _batch(B, station=way == "tracker", warm=way == "warm")
        assert (_in_bytes(sc, w) <= SMALL) == (B == B0)
        ref = _device_reference(opt, sc, w, cap)
        g = _host(opt, sc, w, cap, submit=way == "submit")
        assert _out_bytes(g) < SMALL
        _assert_same(g, ref, cap, (way, B))


def test_small_inputs_with_large_outputs():
    """8 problems (0.2 MB of inputs) with room for max_iter + 1 iterates each: 6.6 MB of outputs, which travel ragged"""
    opt = _shared()["opt"][api.INIT_IQR]
    cap = M + 1
    sc, w = _batch(8, warm=True)
    assert _in_bytes(sc, w) < SMALL // 8
    ref = _device_reference(opt, sc, w, cap)
    for submit in (False, True):
        g = _host(opt, sc, w, cap, submit=submit)
        assert _out_bytes(g) > SMALL
        _assert_same(g, ref, cap, ("large outputs", submit))


def test_large_inputs_with_small_outputs():
    """just above the input boundary with warm rows and shifts, the outputs (three iterates each) below theirs"""
    opt = _shared()["opt"][api.INIT_IQR]
    cap = 3
    one, w_one = _batch(1, warm=True)
    B = SMALL // _in_bytes(one, w_one) + 1
    sc, w = _batch(B, warm=True)
    assert _in_bytes(sc, w) > SMALL
    ref = _device_reference(opt, sc, w, cap)
    for submit in (False, True):
        g = _host(opt, sc, w, cap, submit=submit)
        assert _out_bytes(g) < SMALL
        _assert_same(g, ref, cap, ("large inputs", submit))


@pytest.mark.parametrize("init", [api.INIT_IQR, api.INIT_TRACKER], ids=["iqr", "tracker"])
def test_lane_groups_cut_at_the_first_and_the_last_problem(init):
    """three lane groups [0, 1), [1, B - 1), [B - 1, B) of one table each: every array of the batch, the station column,
    the warm rows and the shifts are cut with them"""
    opt = _shared()["opt"][init]
    B, cap = 6, 8
    sc, w = _batch(B, station=init == api.INIT_TRACKER, warm=True)
    ref = _device_reference(opt, sc, w, cap)
    nl, nr = len(sc["left"]), len(sc["right"])
    grouped = dict(sc, lane_groups=[(0, nl, nr), (1, nl, nr), (B - 1, nl, nr)], left=np.concatenate([sc["left"]] * 3),
                   right=np.concatenate([sc["right"]] * 3))
    _assert_same(_host(opt, grouped, w, cap), ref, cap, "lane groups")
    _assert_same(_host(opt, sc, w, cap), ref, cap, "ungrouped")


def test_two_shards_cut_at_one_and_at_the_last_problem():
    """device 0 listed twice: B = 2 is cut at 1 = B - 1, B = 3 at 2 = B - 1 (the first shard takes the odd problem)"""
    opt = _shared()["opt"][api.INIT_IQR]
    cap = 8
    with api.MultiDeviceOptimizer(api.default_config(N), devices=(0, 0), batch_capacity=4, cmax=CMAX) as m:
        for B in (2, 3):
            got, first, _ = m.shards(B)
            assert got == 2 and list(first) == [0, B - 1 if B == 3 else 1]
            for warm in (True, False):
                sc, w = _batch(B, warm=warm)
                ref = _device_reference(opt, sc, w, cap)
                _assert_same(m.plan(sc, max_iter_trajs=cap, alpha_trace=True, warm=w), ref, cap, ("shards", B, warm))
