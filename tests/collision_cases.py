"""Inputs of the collision audit's tests (tests/test_collisions.py, tests/test_gpu_collisions.py).  A helper module:
nothing here is collected.

crafted_cases() builds scenes on a straight road along x (30 m, barriers at y = +5 / -5) in which the verdict of every
knot follows from the construction.  The ego always heads along +x, so cos = 1 and sin = 0 exactly -- on the host and on
the device -- and its rear / front disc centres are x + r2x, x + f2x; obstacle trajectories carry heading 0 for the same
reason.  With the default vehicle the discs' squares have half side h = 1.21 m (+ buffer) and their centres lie 1.44 m
apart, so every feature is put on the far side of the disc it is meant for (the front disc's +x side, the rear disc's
-x side): the other disc's bounding-box test then rules it out.

  time cases      one dynamic obstacle, a 1 m square, whose samples stand either at HIT (centred on the front square's
                  +x side: FRONT_DYNAMIC and nothing else) or 100 m away; which sample the knot's time selects decides.
  geometry cases  a static polygon 1e-6 inside and 1e-6 outside the decision, or a barrier point at the table's ends.

path_and_shift_rows() gives generator scenes with their host DP coarse path and the same path moved 1.5 m and 3 m to the
left, so that polygons, dynamic obstacles and the left road barrier are all met somewhere.
"""
import dataclasses
import math
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from cilqr_amd import api, scenario, scene_io

MARGIN = 1e-6
TF = {"mix11": 5.0, "demo80": 8.0, "dyn20": 10.0}
RS, RB, RD, FS, FB, FD = api.HIT_BITS


def straight_center(length=30.0, step=1.0, left=5.0, right=5.0):
    s = np.arange(0.0, length + 0.5 * step, step)
    z = np.zeros_like(s)
    return np.ascontiguousarray(np.stack([s, s, z, z, z, z + left, z + right], axis=1))


def _square(cx, cy, half=0.5):
    return np.array([[cx + half, cy + half], [cx + half, cy - half], [cx - half, cy - half], [cx - half, cy + half]])


def _solve(f, target, guess):
    """x next to `guess` with f(x) == target exactly (f monotone, one rounding step at a time)."""
    x = guess
    for _ in range(64):
        v = f(x)
        if v == target:
            return x
        x = math.nextafter(x, math.inf if v < target else -math.inf)
    raise AssertionError("no exact solution next to the guess")


@dataclasses.dataclass
class Case:
    name: str
    scene: scene_io.Scene
    buffer: float
    times: np.ndarray      # [K]
    poses: np.ndarray      # [K, 3]
    expect: np.ndarray     # [K] uint8


def _case(name, static, dynamic, buffer, knots):
    """knots: (time, x, y, expected mask); the heading is 0"""
    k = np.array([[t, x, y, 0.0] for t, x, y, _ in knots], dtype=np.float64)
    scene = scene_io.Scene(np.zeros(4), np.zeros((1, 6)), static, dynamic)
    return Case(name, scene, buffer, k[:, 0].copy(), k[:, 1:4].copy(), np.array([m for *_, m in knots], dtype=np.uint8))


def crafted_cases(cfg=None):
    """(centre line, time cases, geometry cases) for the vehicle of cfg (default: the reference's)."""
    cfg = cfg or api.default_dp_config()
    radius, r2x, f2x = scene_io.vehicle_discs(cfg)
    center = straight_center()
    x, y = 10.0, 0.0
    cf, h = x + f2x * 1.0, radius + 0.0      # (the rear disc: x + r2x)
    body = _square(0.0, 0.0)
    HIT, FAR = (cf + h, y), (cf + h + 100.0, y + 50.0)

    def traj(times, places):
        return np.array([[t, p[0], p[1], 0.0] for t, p in zip(times, places)], dtype=np.float64)

    def dyn(times, places, polygon=body):
        return [scene_io.DynamicObstacle(polygon, traj(times, places))]

    def at(*pairs):
        return [(t, x, y, m) for t, m in pairs]

    tiny = 1e-9
    time_cases = [
        # the first sample with t < time: a knot ON a sample time takes the NEXT sample
        _case("knot on a sample time, next sample hits", [], dyn([0, 1, 2], [FAR, FAR, HIT]), 0.0, at((1.0, FD), (0.5, 0), (1.5, FD))),
        _case("knot on a sample time, its own sample would hit", [], dyn([0, 1, 2], [FAR, HIT, FAR]), 0.0, at((1.0, 0), (0.5, FD), (0.0, FD))),
        # no epsilon on presence: on the first sample time the obstacle is there, a hair earlier it is not
        _case("knot on the first sample time", [], dyn([1, 2, 3], [FAR, HIT, FAR]), 0.0, at((1.0, FD), (1.0 - tiny, 0), (0.0, 0))),
        # on the last sample time std::upper_bound returns end(): the last sample is used
        _case("knot on the last sample time", [], dyn([1, 2, 3], [FAR, FAR, HIT]), 0.0, at((3.0, FD), (3.0 + tiny, 0), (2.0, FD), (1.5, 0))),
        _case("one sample", [], dyn([2], [HIT]), 0.0, at((2.0, FD), (2.0 - tiny, 0), (2.0 + tiny, 0))),
        _case("two samples with one time, the second hits", [], dyn([2, 2], [FAR, HIT]), 0.0, at((2.0, FD), (1.0, 0), (3.0, 0))),
        _case("two samples with one time, the first would hit", [], dyn([2, 2], [HIT, FAR]), 0.0, at((2.0, 0),)),
        _case("begins after the knot", [], dyn([5, 6], [HIT, HIT]), 0.0, at((1.0, 0), (5.5, FD))),
        _case("ends before the knot", [], dyn([-3, -2], [HIT, HIT]), 0.0, at((1.0, 0), (-2.5, FD))),
        _case("a slot without vertices", [np.zeros((0, 2))], dyn([0, 9], [HIT, HIT], polygon=np.zeros((0, 2))), 0.0, at((1.0, 0),)),
    ]

    d = MARGIN
    # a sliver whose lowest vertex A lies on the front square's +x side; its far end C is beside the square, above it: no
    # corner of the square is in the sliver, only A decides (<= h + 1e-10)
    def sliver(delta):
        return [np.array([[cf + h + delta, y], [cf + h + delta + 0.001, y], [cf + h - 0.01, y + h + 3.0]])]

    # a polygon with a V-shaped notch (apex below the front disc, sides of slope 1.6): the two lower corners of the
    # front square sit `inside` below the sides of the V (positive: in the polygon); the rear square's lower left corner
    # is well inside the polygon either way
    def notch(inside):
        y0 = y - h - 2.0 - 1.6 * h + inside
        return [np.array([[cf - 5.0, y0], [cf + 5.0, y0], [cf + 5.0, y0 + 10.0], [cf, y0 + 2.0], [cf - 5.0, y0 + 10.0]])]

    def strip(x0, x1):
        return [np.array([[x0, y - 0.01], [x1, y - 0.01], [x1, y + 0.01], [x0, y + 0.01]])]

    wedge = [np.array([[cf + h + 0.25, y], [cf + h + 2.0, y + 1.0], [cf + h + 2.0, y - 1.0]])]

    def static_case(name, polygons, expect, buffer=0.0):
        return _case(name, polygons, [], buffer, [(0.0, x, y, expect)])

    geometry_cases = [
        static_case("vertex 1e-6 inside the square's side", sliver(-d), FS),
        static_case("vertex on the square's side", sliver(0.0), FS),
        static_case("vertex 1e-6 outside the square's side", sliver(+d), 0),
        static_case("square corners 1e-6 inside the notch's sides", notch(+d), RS | FS),
        static_case("square corners 1e-6 outside the notch's sides", notch(-d), RS),
        static_case("thin polygon ends 1e-6 inside the square", strip(cf + h - d, cf + h + 5.0), FS),
        static_case("thin polygon ends 1e-6 outside the square", strip(cf + h + d, cf + h + 5.0), 0),
        # no vertex in either square, no corner of a square in the polygon: the reference says "no overlap"
        static_case("thin polygon through both squares", strip(cf - 8.0, cf + 8.0), 0),
        static_case("vertex 0.25 m outside, no buffer", wedge, 0),
        static_case("vertex 0.25 m outside, buffer 0.5", wedge, FS, buffer=0.5),
    ]
    # ---- the barrier table's ends.  Its last element is the right barrier (y = -5) of the last station; a disc whose
    # square begins exactly there has that ONE predecessor as its whole window -- the left barrier point of the same
    # station, at the same x, is not in it.
    barrier = scene_io.sorted_road_barriers(center)
    x_first, x_last = float(barrier[0, 0]), float(barrier[-1, 0])
    assert barrier[-1, 1] == -5.0 and barrier[-2, 1] == 5.0 and barrier[-2, 0] == x_last and barrier[0, 0] == barrier[1, 0]
    x_end = _solve(lambda v: (v + r2x * 1.0) - h, x_last, x_last + h - r2x)          # the rear square begins on the last point
    x_begin = x_first - h - f2x                                                       # the front square ends at the first point
    low_in, low_out, high_in = -5.0 + (h - d), -5.0 + (h + d), 5.0 - (h - d)
    geometry_cases += [
        _case("the predecessor element at the end of the barrier table", [], [], 0.0,
              [(0.0, x_end, low_in, RB), (0.0, x_end, low_out, 0), (0.0, x_end, high_in, 0)]),
        _case("beyond the end of the barrier table", [], [], 0.0, [(0.0, x_end + d, low_in, 0), (0.0, x_end + 50.0, low_in, 0)]),
        _case("before and at the start of the barrier table", [], [], 0.0,
              [(0.0, x_begin - d, low_in, 0), (0.0, x_begin + d, low_in, FB), (0.0, x_begin + d, low_out, 0), (0.0, x_begin - 50.0, low_in, 0)]),
    ]
    return center, time_cases, geometry_cases


def write_cases(path, center, cases):
    """The cases as tests/cpp/collision_audit_test.cc reads them (little-endian): "CCASES01", i32 n; per case i32
    n_center, center [n][7], f64 buffer, i32 n_static x (i32 m, [m][2]), i32 n_dynamic x (i32 m, [m][2], i32 T, [T][4]),
    i32 K, rows [K][4] = time x y theta, expected [K] i32."""
    def f64(a):
        return np.ascontiguousarray(a, dtype="<f8").tobytes()
    with open(path, "wb") as o:
        o.write(b"CCASES01" + struct.pack("<i", len(cases)))
        for c in cases:
            o.write(struct.pack("<i", len(center)) + f64(center) + struct.pack("<d", c.buffer))
            o.write(struct.pack("<i", len(c.scene.static)))
            for p in c.scene.static:
                o.write(struct.pack("<i", len(p)) + f64(p))
            o.write(struct.pack("<i", len(c.scene.dynamic)))
            for dob in c.scene.dynamic:
                o.write(struct.pack("<i", len(dob.polygon)) + f64(dob.polygon))
                o.write(struct.pack("<i", len(dob.trajectory)) + f64(dob.trajectory))
            o.write(struct.pack("<i", len(c.times)) + f64(np.concatenate([c.times[:, None], c.poses], axis=1)))
            o.write(np.ascontiguousarray(c.expect, dtype="<i4").tobytes())


def rows_in_layout(layout, times, poses):
    """[..., K, fields] rows of `layout` that carry the poses; every column that is not read holds a NaN."""
    times, poses = np.asarray(times, float), np.asarray(poses, float)
    rows = np.full(poses.shape[:-1] + (api.ROWS_FIELDS[layout],), np.nan)
    ct, cx, cy, cth = api.ROWS_POSE_COLUMNS[layout]
    rows[..., ct] = times
    rows[..., cx], rows[..., cy], rows[..., cth] = poses[..., 0], poses[..., 1], poses[..., 2]
    return np.ascontiguousarray(rows)


def generator_scenes(family, n, seed):
    spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True)
    return sc, scene_io.from_generator(sc)


def path_and_shift_rows(family, n, seed, workers=16, planner=None):
    """n generator scenes of the family: (SceneFile, DP config, times [n, K], poses [n, 3, K, 3]) -- per scene the DP
    planner's coarse path and that path moved 1.5 m and 3 m to its left.  The path comes from the host planner, or from
    the batched one of `planner` (a BatchIlqrOptimizer) where a GPU is at hand: the rows are inputs here, not results."""
    sc, sf = generator_scenes(family, n, seed)
    cfg = api.default_dp_config(tf=TF[family])
    if planner is not None:
        coarse = planner.dp_plan_batch(scene_io.pack_scene_batch(sf.center, sf.scenes), sc["start"], cfg)["dp"]
    else:
        def plan(scene):
            _, path = api.dp_plan(scene_io.flatten_scene(sf.center, scene), scene.start[:3], cfg)
            return path
        with ThreadPoolExecutor(workers) as pool:
            coarse = np.stack(list(pool.map(plan, sf.scenes)))
    th = coarse[:, :, 4]
    poses = np.stack([np.stack([coarse[:, :, 2] - shift * np.sin(th), coarse[:, :, 3] + shift * np.cos(th), th], axis=-1)
                      for shift in (0.0, 1.5, 3.0)], axis=1)
    return sf, cfg, np.ascontiguousarray(coarse[:, :, 0]), np.ascontiguousarray(poses)


def _narrower(cfg, by):
    """cfg with the width that makes the disc radius smaller by `by` (the disc offsets depend on the length alone)."""
    radius, _, _ = scene_io.vehicle_discs(cfg)
    quarter = 0.25 * (cfg.wheel_base + cfg.rear_hang_length + cfg.front_hang_length)
    out = api.DpConfig.from_buffer_copy(cfg)
    out.width = 2.0 * math.sqrt((radius - by) ** 2 - quarter ** 2)
    return out


def host_verdicts(flat, times, poses, cfg, buffer, move=1e-9):
    """The host audit nine times over -- as given, and with each of buffer, x, y, theta moved by +-move: (mask [K] of the
    given inputs, first_hit, n_hit, decided [K] bool: the nine masks agree).  A buffer that would become negative is
    moved by narrowing the vehicle instead: the half side radius + buffer is what both change."""
    def run(dx=0.0, dy=0.0, dth=0.0, dbuf=0.0):
        c, b = cfg, buffer + dbuf
        if b < 0.0:
            c, b = _narrower(cfg, -b), 0.0
        rows = rows_in_layout(api.ROWS_TRAJ, times, poses + np.array([dx, dy, dth]))
        return api.check_collisions(flat, rows, api.ROWS_TRAJ, c, b)
    mask, first, n_hit = run()
    decided = np.ones(len(mask), dtype=bool)
    for sign in (+move, -move):
        for kw in ("dx", "dy", "dth", "dbuf"):
            decided &= run(**{kw: sign})[0] == mask
    return mask, first, n_hit, decided
