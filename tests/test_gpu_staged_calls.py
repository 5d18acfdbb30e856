"""The staging of the batched entry points that take HOST or DEVICE arrays (cilqr_amd/csrc/staging.hpp): every array of a call
is bound to its slot of the handle's blocks once, and the blocks grow to the largest call.  What can go wrong there is a device
pointer taken before its block grew, or an array bound to the wrong block -- so every entry point is called on ONE handle on
HOST arrays with batch 1, then 65, then 1 again, with a DEVICE call of batch 65 before and after the large one, once with its
optional arrays and once without.  Every result must be, bit for bit, that of the same call on a fresh handle; every DEVICE
result that of the HOST call; and what lies behind the last element of an output keeps its sentinel.

An input that shares a block with the outputs is only a race where one kernel reads and writes; the margins call therefore has
two lane groups, whose kernels run one behind the other.  That second group is the only thing here that sees inputs staged
into the output block (at batch 65, as DEVICE against HOST), so it is not redundant.  The reach of the file ends at the line
of stage() that picks a block by direction: an array handed over as `out` where `inout` was meant is no type error, and the
scene-points and window calls would show it only through the sentinel behind a count.

Shapes are the smallest the generators give: 11 knots, scenes of two obstacles, lane tables of three rows."""
import numpy as np
import pytest

import carry_cases as cyc
import margins_cases as mc
import scene_window_cases as swc
import track_cases as tc
from cilqr_amd import api

pytestmark = pytest.mark.gpu

K = 11
PAD = 7                         # elements behind the last one of every output
SENTINEL = {np.dtype(np.float64): -777.25, np.dtype(np.int32): -9, np.dtype(np.uint32): 0xABCDEF01, np.dtype(np.uint8): 0xA5}
LARGE = 65


def handle():
    return api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=LARGE, cmax=16, max_lane_segments=64)


@pytest.fixture(scope="module")
def opt():
    with handle() as o:
        yield o


class Spec:
    """One call: ins {name: array}, outs {name: (dtype, shape)}, optional = names the caller may leave out (inputs included),
    inout = outputs the call reads as well; call(opt, p, mem) -> (rc, count or None) with p = {name: address or None}."""

    def __init__(self, ins, outs, call, optional=(), inout=()):
        self.ins, self.outs, self.call, self.optional, self.inout = ins, outs, call, tuple(optional), tuple(inout)


def scene_pointers(packed, p, mem):
    return api.scene_batch_struct(packed, mem, **{k: p[k] for k in api._SCENE_BATCH_ARRAYS})


def scenes(B, seed):
    """(packed, t0): B scenes of two dynamic obstacles with up to 8 samples each (scene_window_cases.random_batch)"""
    packed, t0 = swc.random_batch(np.random.default_rng(seed), B, 2, 8)
    return packed, t0, {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}


def road_rows(B, seed):
    """[B,K,9] CILQR_ROWS_COARSE along the straight road of the scenes, close to where their obstacles drive"""
    rng = np.random.default_rng(seed)
    t = np.arange(K) * 0.1
    rows = rng.normal(0.0, 1.0, (B, K, 9))
    rows[..., 0] = t
    rows[..., 2] = rng.uniform(15.0, 25.0, (B, 1)) + 4.0 * t
    rows[..., 3] = rng.uniform(-2.0, 2.0, (B, 1)) + 0.1 * np.sin(t)
    rows[..., 4] = rng.uniform(-0.2, 0.2, (B, 1))
    return np.ascontiguousarray(rows)


def spec_dp_plan(B):
    packed, _, arrays = scenes(B, 11)
    cfg = api.default_dp_config(tf=1.0, delta_t=0.1)
    start3 = np.ascontiguousarray(np.random.default_rng(12).uniform([2.0, -1.0, -0.1], [8.0, 1.0, 0.1], (B, 3)))
    f8, i4 = np.float64, np.int32
    return Spec(dict(arrays, start3=start3),
                dict(coarse9=(f8, (B, K, api.COARSE_FIELDS)), coarse6=(f8, (B, K, 6)), knots3=(f8, (B, K, 3)), station=(f8, (B, K)),
                     found=(i4, (B,))),
                lambda o, p, mem: o.dp_plan_batch_raw(cfg, scene_pointers(packed, p, mem), p["start3"], K, p["coarse9"], p["coarse6"],
                                                      p["knots3"], p["station"], p["found"]),
                optional=("coarse9", "coarse6", "knots3", "station"))


def spec_scene_points(B):
    packed, _, arrays = scenes(B, 21)
    times, P = np.arange(K) * 0.1, 3 * 4
    return Spec(arrays, dict(points=(np.float64, (B, K, P, 2)), count=(np.int32, (B, K)), ok=(np.int32, (B,))),
                lambda o, p, mem: (o.scene_points_raw(scene_pointers(packed, p, mem), K, times, False, P, p["points"], p["count"],
                                                      p["ok"]), None),
                optional=("ok",), inout=("points",))


def spec_collisions(B):
    packed, _, arrays = scenes(B, 31)
    cfg = api.default_dp_config()
    return Spec(dict(arrays, rows=road_rows(B, 32)),
                dict(mask=(np.uint8, (B, K)), first_hit=(np.int32, (B,)), n_hit=(np.int32, (B,))),
                lambda o, p, mem: o.check_collisions_raw(cfg, scene_pointers(packed, p, mem), api.ROWS_COARSE, p["rows"], K, 0.25,
                                                         p["mask"], p["first_hit"], p["n_hit"]),
                optional=("mask", "n_hit"))


def spec_clearance(B):
    packed, _, arrays = scenes(B, 41)
    cfg = api.default_dp_config()
    F = api.CLEARANCE_FIELDS
    return Spec(dict(arrays, rows=road_rows(B, 42)),
                dict(clearance=(np.float64, (B, K, F)), nearest=(np.int32, (B, K, F)), min_clearance=(np.float64, (B,)),
                     min_knot=(np.int32, (B,))),
                lambda o, p, mem: o.clearance_raw(cfg, scene_pointers(packed, p, mem), api.ROWS_COARSE, p["rows"], K, p["clearance"],
                                                  p["nearest"], p["min_clearance"], p["min_knot"], 1.0),
                optional=("clearance", "nearest"))


def spec_margins(B):
    rng = np.random.default_rng(51)
    cmax = 4
    state = rng.normal(0.0, 1.0, (B, K, 8))
    state[..., 0] = rng.uniform(-6.0, 14.0, (B, K))
    rows = np.ascontiguousarray(mc.rows_in_layout(api.ROWS_TRAJ, state))
    corridor = np.ascontiguousarray(rng.normal(0.0, 1.0, (B, K, cmax, 3)) + np.array([0.0, 0.0, 6.0]))
    ccount = rng.integers(0, cmax + 1, (B, K)).astype(np.int32)
    # two lane groups, so that the kernels of the second run behind those of the first: an input that shared a block with the
    # outputs would be read after it was overwritten.  The tables are host memory whatever the call's arrays are.
    left = np.ascontiguousarray(np.concatenate([mc.tables(0)[0], mc.tables(1)[0]]))
    right = np.ascontiguousarray(np.concatenate([mc.tables(0)[1], mc.tables(1)[1]]))
    g_start = np.array([0, (B + 1) // 2, B], dtype=np.int32)
    g_rows = np.array([3, 3], dtype=np.int32)

    def call(o, p, mem):
        prob = api.ProblemBatch(B, K, cmax, mem, None, None, p["corridor"], p["ccount"], 6, 6, left.ctypes.data, right.ctypes.data)
        prob.n_lane_groups = 2
        prob.lane_group_start, prob.lane_group_left, prob.lane_group_right = g_start.ctypes.data, g_rows.ctypes.data, g_rows.ctypes.data
        return o.constraint_margins_raw(prob, api.ROWS_TRAJ, p["rows"], p["margins"], p["which"], p["min_margin"], p["min_knot"],
                                        None, p["violated"])
    M = api.MARGIN_FIELDS
    return Spec(dict(rows=rows, corridor=corridor, ccount=ccount),
                dict(margins=(np.float64, (B, K, M)), which=(np.int32, (B, K, api.MARGIN_WHICH_FIELDS)), min_margin=(np.float64, (B, M)),
                     min_knot=(np.int32, (B, M)), violated=(np.uint32, (B,))),
                call, optional=("margins", "which"))


def spec_track(B):
    rows, start6 = tc.base_rows(knots=K)
    D = 7
    return Spec(dict(rows=np.ascontiguousarray(rows[:B]), start6=np.ascontiguousarray(start6[:B] + [0.1, -0.1, 0.01, 0.2, 0.0, 0.0])),
                dict(driven=(np.float64, (B, D, 10)), ok=(np.int32, (B,))),
                lambda o, p, mem: o.track_raw(B, api.ROWS_TRAJ, p["rows"], K, p["start6"], D, p["driven"], p["ok"], mem),
                optional=("start6",))


def spec_window(B):
    packed, t0, arrays = scenes(B, 71)
    out = 8
    return Spec(dict(arrays, t0=np.ascontiguousarray(t0)),
                dict(trajectories=(np.float64, (B, 2, out, 4)), counts=(np.int32, (B, 2)), ok=(np.int32, (B,))),
                lambda o, p, mem: o.window_scenes_raw(scene_pointers(packed, p, mem), p["t0"], 0.3, out, p["trajectories"], p["counts"],
                                                      p["ok"]),
                optional=("ok",), inout=("trajectories",))


def spec_carry(B):
    plans, advance, _ = cyc.make_batch(B, K, 81)
    f8 = np.float64
    return Spec(dict(rows=np.ascontiguousarray(plans), advance=np.ascontiguousarray(advance)),
                dict(coarse9=(f8, (B, K, api.COARSE_FIELDS)), coarse6=(f8, (B, K, 6)), knots3=(f8, (B, K, 3)), station=(f8, (B, K)),
                     state=(np.int32, (B,))),
                lambda o, p, mem: o.carry_raw(B, api.ROWS_PLAN, p["rows"], K, p["advance"], cyc.BATCH_MAX_ADVANCE, K, cyc.DT,
                                              p["coarse9"], p["coarse6"], p["knots3"], p["station"], p["state"], mem),
                optional=("coarse9", "coarse6", "knots3", "station"))


def spec_resample(B):
    plans, _, _ = cyc.make_batch(B, K, 91)
    plans = np.nan_to_num(plans)
    M = 5
    queries = np.ascontiguousarray(plans[:, :1, 0] + np.linspace(-0.05, 1.2, M))
    return Spec(dict(rows=np.ascontiguousarray(plans), queries=queries), dict(out=(np.float64, (B, M, 11))),
                lambda o, p, mem: (o.resample_raw(B, api.ROWS_PLAN, p["rows"], K, api.KEY_TIME, p["queries"], M, True, p["out"], mem),
                                   None))


def spec_frenet(B):
    rng = np.random.default_rng(101)
    xy = np.ascontiguousarray(np.stack([rng.uniform(-5.0, 125.0, (B, K)), rng.uniform(-4.0, 4.0, (B, K))], axis=-1))
    return Spec(dict(rows=xy), dict(frenet=(np.float64, (B, K, api.FRENET_FIELDS))),
                lambda o, p, mem: (o.frenet_raw(swc.CENTER, B, api.ROWS_POINTS, p["rows"], K, p["frenet"], mem), None))


def spec_cartesian(B):
    rng = np.random.default_rng(111)
    n = 3 * B
    sl = np.ascontiguousarray(np.stack([rng.uniform(-5.0, 125.0, n), rng.uniform(-4.0, 4.0, n)], axis=-1))
    return Spec(dict(sl=sl), dict(xyt=(np.float64, (n, 3))),
                lambda o, p, mem: (o.cartesian_raw(swc.CENTER, n, p["sl"], p["xyt"], mem), None))


def spec_corridors(B):
    rng = np.random.default_rng(121)
    P, cmax = 6, 16
    cfg = api.default_corridor_config()
    knots = np.ascontiguousarray(np.concatenate([rng.uniform(0.0, 50.0, (B, K, 2)), rng.uniform(-3.0, 3.0, (B, K, 1))], axis=-1))
    points = np.ascontiguousarray(knots[:, :, None, :2] + rng.uniform(2.0, 20.0, (B, K, P, 2)) * rng.choice([-1.0, 1.0], (B, K, P, 2)))
    count = rng.integers(0, P + 1, (B, K)).astype(np.int32)
    return Spec(dict(knots=knots, points=points, point_count=count),
                dict(corridor=(np.float64, (B, K, cmax, 3)), corridor_count=(np.int32, (B, K)), polygons=(np.float64, (B, K, cmax, 2))),
                lambda o, p, mem: o.build_corridors_raw(cfg, B, K, p["knots"], p["points"], p["point_count"], P, p["corridor"],
                                                        p["corridor_count"], cmax, mem, p["polygons"]),
                optional=("polygons",))


SPECS = dict(dp_plan=spec_dp_plan, scene_points=spec_scene_points, collisions=spec_collisions, clearance=spec_clearance,
             margins=spec_margins, track=spec_track, window=spec_window, carry=spec_carry, resample=spec_resample,
             frenet=spec_frenet, cartesian=spec_cartesian, corridors=spec_corridors)


def run(o, spec, mem, omit):
    """The call with its outputs filled with sentinels, PAD elements behind each; omit: without the optional arrays.
    Returns {name: bytes of the output with its padding}, count, and checks what must stay untouched."""
    import torch
    left_out = set(spec.optional) if omit else set()
    host = {k: v for k, v in spec.ins.items()}
    for k, (dtype, shape) in spec.outs.items():
        host[k] = np.full(int(np.prod(shape)) + PAD, SENTINEL[np.dtype(dtype)], dtype=dtype)
    if mem == api.MEM_DEVICE:
        held = {k: torch.from_numpy(v).to("cuda:0") for k, v in host.items() if v.dtype != np.uint32}
        held.update({k: torch.from_numpy(v.view(np.int32)).to("cuda:0") for k, v in host.items() if v.dtype == np.uint32})
        torch.cuda.synchronize()
        p = {k: (None if k in left_out else t.data_ptr()) for k, t in held.items()}
    else:
        p = {k: (None if k in left_out else v.ctypes.data) for k, v in host.items()}
    rc, count = spec.call(o, p, mem)
    assert rc == 0, rc
    got = {}
    for k, (dtype, shape) in spec.outs.items():
        a = host[k] if mem == api.MEM_HOST else held[k].cpu().numpy().view(dtype)
        n = int(np.prod(shape))
        assert (a[n:] == SENTINEL[np.dtype(dtype)]).all(), f"{k}: written behind its last element"
        if k in left_out:
            assert (a == SENTINEL[np.dtype(dtype)]).all(), f"{k}: written though it was left out"
        else:
            if k not in spec.inout:
                assert (a[:n] != SENTINEL[np.dtype(dtype)]).any() or n == 0, f"{k}: not written"
            got[k] = a.tobytes()
    return got, count


_FRESH = {}


def fresh(name, B, omit):
    """the HOST call on a handle that has seen no other call"""
    if (name, B, omit) not in _FRESH:
        with handle() as o:
            _FRESH[name, B, omit] = run(o, SPECS[name](B), api.MEM_HOST, omit)
    return _FRESH[name, B, omit]


@pytest.mark.parametrize("name", list(SPECS))
def test_results_do_not_depend_on_what_the_handle_has_staged_before(opt, name):
    small, large = SPECS[name](1), SPECS[name](LARGE)
    for omit in (False, True):
        assert run(opt, small, api.MEM_HOST, omit) == fresh(name, 1, omit), (name, omit, "batch 1")
        device = run(opt, large, api.MEM_DEVICE, omit)
        host = run(opt, large, api.MEM_HOST, omit)
        assert host == fresh(name, LARGE, omit), (name, omit, "batch 65")
        assert device == host, (name, omit, "DEVICE against HOST")
        assert run(opt, large, api.MEM_DEVICE, omit) == host, (name, omit, "DEVICE after HOST")
        assert run(opt, small, api.MEM_HOST, omit) == fresh(name, 1, omit), (name, omit, "batch 1 again")
