"""Scene wire format: a compact binary equivalent of what the reference moves between
its scenario publisher and its planning node -- the six ROS messages under msg/ (CenterLine,
CenterLinePoint, Obstacles, DynamicObstacle, DynamicObstacles, DynamicTrajectoryPoint) and the
pickle {"center", "static", "dynamic"} of script/reference_publisher.py:232-236 -- plus the two
things a replay of the optimizer needs on top (start state, coarse trajectory), so that a scene
can be replayed bit for bit on the CPU oracle and on the GPU.

A file holds ONE road and B scenes on it:

    "CILQRSC1" | u32 version = 1 | u32 B | u32 K | f64 dt
    u32 n_center | center[n_center][7] f64            CenterLinePoint: s x y theta kappa left_bound right_bound
    per scene:
      start[4] f64 (x y theta v) | coarse[K][6] f64 (x y theta v a delta)
      u32 n_static  | per obstacle: u32 m | polygon[m][2] f64 (world frame)           Obstacles.msg
      u32 n_dynamic | per obstacle: u32 m | polygon[m][2] f64 (body frame)            DynamicObstacle.msg
                                  | u32 T | trajectory[T][4] f64 (time x y theta)     DynamicTrajectoryPoint.msg

Everything little-endian.  `environment_points` and `road_barriers` restate the queries the reference's
Environment answers from that data (algorithm/utils/environment.cpp:134-182, planning_node.cc:63-78):
the obstacle corner points valid at a knot's time and the two road barriers -- the inputs of
cilqr_build_corridors / cilqr_lane_constraints.
"""
from __future__ import annotations

import bisect
import ctypes
import ctypes.util
import dataclasses
import math
import struct

import numpy as np

MAGIC = b"CILQRSC1"
K_MATH_EPS = 1e-10  # algorithm/math/vec2d.h:33


@dataclasses.dataclass
class DynamicObstacle:
    polygon: np.ndarray      # [m,2] body frame
    trajectory: np.ndarray   # [T,4] time, x, y, theta


@dataclasses.dataclass
class Scene:
    start: np.ndarray                 # [4]
    coarse: np.ndarray                # [K,6]
    static: list                      # of [m,2] world-frame polygons
    dynamic: list                     # of DynamicObstacle


@dataclasses.dataclass
class SceneFile:
    dt: float
    center: np.ndarray                # [n,7]
    scenes: list


def _rect(hl: float, hw: float) -> np.ndarray:
    return np.array([[hl, hw], [hl, -hw], [-hl, -hw], [-hl, hw]], dtype=np.float64)


def from_generator(sc: dict) -> SceneFile:
    """Scenes of cilqr_amd.scenario.generate(..., scenarios=True) in the reference's vocabulary: an
    obstacle that never moves becomes a static polygon (Obstacles.msg), the others a body-frame
    polygon with the trajectory of the knots at which they exist (pedestrians enter and leave)."""
    road = sc["road"]
    from .scenario import LEFT_BOUND, RIGHT_BOUND
    n = len(road.s)
    center = np.stack([road.s, road.x, road.y, road.theta, road.kappa, np.full(n, LEFT_BOUND), np.full(n, RIGHT_BOUND)], 1)
    pose, live, half, kind = sc["obstacle_pose"], sc["obstacle_live"], sc["obstacle_half_size"], sc["obstacle_kind"]
    B, O, K = live.shape
    t = np.arange(K) * sc["dt"]
    scenes = []
    for b in range(B):
        static, dynamic = [], []
        for o in range(O):
            m = live[b, o]
            if not m.any():
                continue
            body = _rect(*half[o])
            if kind[o] == 2:      # static vehicle: one world-frame polygon
                x, y, th = pose[b, o, 0]
                R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
                static.append(body @ R.T + [x, y])
            else:
                traj = np.concatenate([t[m, None], pose[b, o, m]], axis=1)
                dynamic.append(DynamicObstacle(body, traj))
        scenes.append(Scene(sc["start"][b].copy(), sc["coarse"][b].copy(), static, dynamic))
    return SceneFile(float(sc["dt"]), center, scenes)


def save(path: str, f: SceneFile) -> None:
    K = f.scenes[0].coarse.shape[0] if f.scenes else 0
    with open(path, "wb") as o:
        o.write(MAGIC)
        o.write(struct.pack("<IIId", 1, len(f.scenes), K, f.dt))
        c = np.ascontiguousarray(f.center, dtype="<f8")
        o.write(struct.pack("<I", c.shape[0]))
        o.write(c.tobytes())
        for s in f.scenes:
            o.write(np.ascontiguousarray(s.start, dtype="<f8").tobytes())
            o.write(np.ascontiguousarray(s.coarse, dtype="<f8").tobytes())
            o.write(struct.pack("<I", len(s.static)))
            for p in s.static:
                o.write(struct.pack("<I", len(p)))
                o.write(np.ascontiguousarray(p, dtype="<f8").tobytes())
            o.write(struct.pack("<I", len(s.dynamic)))
            for d in s.dynamic:
                o.write(struct.pack("<I", len(d.polygon)))
                o.write(np.ascontiguousarray(d.polygon, dtype="<f8").tobytes())
                o.write(struct.pack("<I", len(d.trajectory)))
                o.write(np.ascontiguousarray(d.trajectory, dtype="<f8").tobytes())


def load(path: str) -> SceneFile:
    raw = open(path, "rb").read()
    if raw[:8] != MAGIC:
        raise ValueError("not a CILQR scene file")
    pos = 8
    version, B, K, dt = struct.unpack_from("<IIId", raw, pos)
    pos += 20
    if version != 1:
        raise ValueError(f"unsupported scene file version {version}")

    def u32():
        nonlocal pos
        v, = struct.unpack_from("<I", raw, pos)
        pos += 4
        return v

    def f64(*shape):
        nonlocal pos
        n = int(np.prod(shape))
        a = np.frombuffer(raw, dtype="<f8", count=n, offset=pos).reshape(shape).copy()
        pos += 8 * n
        return a

    center = f64(u32(), 7)
    scenes = []
    for _ in range(B):
        start, coarse = f64(4), f64(K, 6)
        static = [f64(u32(), 2) for _ in range(u32())]
        dynamic = []
        for _ in range(u32()):
            poly = f64(u32(), 2)
            dynamic.append(DynamicObstacle(poly, f64(u32(), 4)))
        scenes.append(Scene(start, coarse, static, dynamic))
    if pos != len(raw):
        raise ValueError("trailing bytes in scene file")
    return SceneFile(dt, center, scenes)


def sample_points(polygon: np.ndarray) -> np.ndarray:
    """Polygon2d::sample_points (algorithm/math/polygon2d.cpp:259-271): six points per edge (ratio = 0, 0.2, ... with
    the reference's floating-point accumulation), edges in the counter-clockwise order BuildFromPoints leaves
    (polygon2d.cpp:212-220: a clockwise input is reversed first)."""
    p = np.asarray(polygon, float)
    area = sum((p[i - 1, 0] - p[0, 0]) * (p[i, 1] - p[0, 1]) - (p[i - 1, 1] - p[0, 1]) * (p[i, 0] - p[0, 0]) for i in range(1, len(p)))
    if area < 0:
        p = p[::-1]
    out = []
    for i in range(len(p)):
        q = p[(i + 1) % len(p)]
        ratio = 0.0
        while ratio < 1.0 + K_MATH_EPS:
            out.append([p[i, 0] * (1 - ratio) + q[0] * ratio, p[i, 1] * (1 - ratio) + q[1] * ratio])
            ratio += 1.0 / 5.0
    return np.asarray(out)


def environment_points(scene: Scene, times, multiple_sample: bool = False) -> tuple:
    """Environment::QueryStaticObstaclesPoints + QueryDynamicObstaclesPoints (environment.cpp:153-182,
    is_multiple_sample = false) for every knot time: (points [K,P,2] padded with zeros, counts [K]).
    A dynamic obstacle exists at time t when t lies within its trajectory (to 1e-10); its polygon is
    the one of the first trajectory sample later than t - 1e-10 (std::upper_bound, cpp:143-146),
    placed by that sample's pose (planning_node.cc:68-75).  multiple_sample: the polygons' sample points
    (is_multiple_sample, environment.cpp:163,178) instead of their corners."""
    pick = sample_points if multiple_sample else (lambda p: p)
    per_knot = []
    for t in times:
        pts = [pick(p) for p in scene.static]
        for d in scene.dynamic:
            tt = d.trajectory[:, 0]
            if tt[0] > t + K_MATH_EPS or tt[-1] < t - K_MATH_EPS:
                continue
            i = int(np.searchsorted(tt + K_MATH_EPS, t, side="right"))   # first sample with t < time + eps
            i = min(i, len(tt) - 1)
            _, x, y, th = d.trajectory[i]
            c, s = np.cos(th), np.sin(th)     # Pose::transform (pose.h:40-46): x + rx cos - ry sin, in that order
            pts.append(pick(np.stack([x + d.polygon[:, 0] * c - d.polygon[:, 1] * s,
                                      y + d.polygon[:, 0] * s + d.polygon[:, 1] * c], axis=1)))
        per_knot.append(np.concatenate(pts, axis=0) if pts else np.zeros((0, 2)))
    P = max((len(p) for p in per_knot), default=0)
    out = np.zeros((len(per_knot), P, 2))
    cnt = np.zeros(len(per_knot), dtype=np.int32)
    for k, p in enumerate(per_knot):
        out[k, :len(p)] = p
        cnt[k] = len(p)
    return out, cnt


def _polygon_has_point(q: np.ndarray, px: float, py: float) -> bool:
    """Polygon2d::IsPointIn (polygon2d.cpp:120-140) behind the bounding box of BuildFromPoints."""
    if px < q[:, 0].min() or px > q[:, 0].max() or py < q[:, 1].min() or py > q[:, 1].max():
        return False
    inside = False
    j = len(q) - 1
    for i in range(len(q)):
        xi, yi, xj, yj = q[i, 0], q[i, 1], q[j, 0], q[j, 1]
        if (yi > py) != (yj > py):
            side = (xi - px) * (yj - py) - (xj - px) * (yi - py)
            if (side > 0.0) if yi < yj else (side < 0.0):
                inside = not inside
        j = i
    return inside


def _square_has_points(cx: float, cy: float, h: float, pts: np.ndarray) -> np.ndarray:
    """Box2d::IsPointIn at heading 0 (box2d.cpp:123-129) for every row of pts."""
    return (np.abs(pts[:, 0] - cx) <= h + K_MATH_EPS) & (np.abs(pts[:, 1] - cy) <= h + K_MATH_EPS)


def _polygon_overlaps_square(q: np.ndarray, cx: float, cy: float, h: float) -> bool:
    """Polygon2d::HasOverlap(Box2d) (polygon2d.cpp:150-164): boxes apart -> no; a vertex in the square -> yes; else a
    corner of the square in the polygon."""
    if cx + h < q[:, 0].min() or cx - h > q[:, 0].max() or cy + h < q[:, 1].min() or cy - h > q[:, 1].max():
        return False
    if _square_has_points(cx, cy, h, q).any():
        return True
    return any(_polygon_has_point(q, x, y) for x, y in ((cx + h, cy - h), (cx + h, cy + h), (cx - h, cy + h), (cx - h, cy - h)))


def vehicle_discs(cfg) -> tuple:
    """(radius, rear offset, front offset) of the two collision discs (vehicle_param.h:76-95); cfg carries wheel_base,
    rear_hang_length, front_hang_length and width (api.DpConfig, or anything with those attributes)."""
    length = cfg.wheel_base + cfg.rear_hang_length + cfg.front_hang_length
    return math.hypot(0.25 * length, 0.5 * cfg.width), 0.25 * length - cfg.rear_hang_length, 0.75 * length - cfg.rear_hang_length


def _normalize_angle(a: float) -> float:
    a = math.fmod(a + math.pi, 2.0 * math.pi)      # math_utils.cpp:53-59
    if a < 0.0:
        a += 2.0 * math.pi
    return a - math.pi


def _evaluate_station(c: list, stations: list, station: float) -> tuple:
    """DiscretizedTrajectory::EvaluateStation (discretized_trajectory.cpp:117-128, :66-89) on the rows of a centre line:
    (x, y, theta, left_bound, right_bound) at `station`."""
    n = len(c)
    if station >= stations[-1]:
        it = n - 1
    elif station < stations[0]:
        it = 0
    else:
        it = bisect.bisect_left(stations, station)      # first point with s >= station
    it = max(it, 1)
    p0, p1 = c[it - 1], c[it]
    s0, s1 = p0[0], p1[0]
    if abs(s1 - s0) < K_MATH_EPS:
        return p0[1], p0[2], p0[3], p0[5], p0[6]
    w = (station - s0) / (s1 - s0)
    a0, a1 = _normalize_angle(p0[3]), _normalize_angle(p1[3])      # math::slerp, math_utils.h:208-225
    d = a1 - a0
    if d > math.pi:
        d = d - 2 * math.pi
    elif d < -math.pi:
        d = d + 2 * math.pi
    theta = _normalize_angle(a0 + d * ((station - s0) / (s1 - s0)))
    lin = lambda e: (1 - w) * p0[e] + w * p1[e]
    return lin(1), lin(2), theta, lin(5), lin(6)


def sorted_road_barriers(center: np.ndarray) -> np.ndarray:
    """Environment::set_reference (environment.cpp:20-43): the centre line evaluated every 0.1 m of station and shifted
    by +left_bound / -right_bound along its normal, left and right point of a station one after the other, then stably
    sorted by x: [n,2].  Plain Python floats and the math module, so every operation is the C library's."""
    c = [[float(v) for v in row] for row in np.asarray(center, float)]
    stations = [row[0] for row in c]
    start_s, back_s = stations[0], stations[-1]
    out = []
    for i in range(int((back_s - start_s) / 0.1) + 1):
        s = start_s + i * 0.1
        x, y, th, lb, rb = _evaluate_station(c, stations, s)
        for l in (lb, -rb):                               # ReferenceLine::GetCartesian, cpp:199-203
            out.append((x - l * math.sin(th), y + l * math.cos(th)))
    both = np.array(out, dtype=np.float64).reshape(-1, 2)
    return both[np.argsort(both[:, 0], kind="stable")]


def environment_collisions(center: np.ndarray, scene: Scene, cfg, times, poses, buffer: float = 0.0, barrier=None) -> tuple:
    """Environment::CheckOptimizationCollision(time, pose, collision_buffer) (environment.cpp:92-111) for every knot, all
    six tests made: (mask [K] uint8, first_hit, n_hit).  Bit 0 / 1 / 2: the rear disc against a static polygon / a road
    barrier point / a dynamic polygon; bits 3 - 5: the front disc.  times [K], poses [K,3] = x, y, theta.  The discs
    are axis-aligned squares of half side radius + buffer; the barrier window is two upper_bounds on x plus the one
    predecessor; a dynamic obstacle is absent when time[0] > t or time[-1] < t (no epsilon, cpp:117), else its pose is
    the first sample with t < time[k], past the end the last.  `barrier`: sorted_road_barriers(center), to build it once
    for many scenes."""
    radius, r2x, f2x = vehicle_discs(cfg)
    h = radius + buffer
    if barrier is None:
        barrier = sorted_road_barriers(center)
    bx = np.ascontiguousarray(barrier[:, 0])
    statics = [np.asarray(p, float).reshape(-1, 2) for p in scene.static if len(p) >= 1]
    mask = np.zeros(len(times), dtype=np.uint8)
    for k, (t, (x, y, th)) in enumerate(zip(times, poses)):
        placed = []
        for d in scene.dynamic:
            tt = d.trajectory[:, 0]
            if len(d.polygon) < 1 or len(tt) < 1 or tt[0] > t or tt[-1] < t:
                continue
            i = min(int(np.searchsorted(tt, t, side="right")), len(tt) - 1)   # first sample with t < time; NaN sorts last
            _, ox, oy, oth = d.trajectory[i]
            c, s = math.cos(oth), math.sin(oth)     # Pose::transform (pose.h:40-46): x + rx cos - ry sin, in that order
            placed.append(np.stack([ox + d.polygon[:, 0] * c - d.polygon[:, 1] * s,
                                    oy + d.polygon[:, 0] * s + d.polygon[:, 1] * c], axis=1))
        ct, st = math.cos(th), math.sin(th)
        for shift, off in ((0, r2x), (3, f2x)):
            cx, cy = x + off * ct, y + off * st
            if any(_polygon_overlaps_square(q, cx, cy, h) for q in statics):
                mask[k] |= 1 << shift
            if len(bx) and not (cx + h < bx[0] or cx - h > bx[-1]):
                first = int(np.searchsorted(bx, cx - h, side="right"))
                last = int(np.searchsorted(bx, cx + h, side="right"))
                first = max(first - 1, 0)
                if _square_has_points(cx, cy, h, barrier[first:last]).any():
                    mask[k] |= 2 << shift
            if any(_polygon_overlaps_square(q, cx, cy, h) for q in placed):
                mask[k] |= 4 << shift
    hit = np.flatnonzero(mask)
    return mask, (int(hit[0]) if len(hit) else -1), int(len(hit))


# hypot is the C library's own: math.hypot is Python's algorithm, which is not glibc's in the last bit for every argument
_LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_LIBM.hypot.restype = ctypes.c_double
_LIBM.hypot.argtypes = [ctypes.c_double] * 2
_hypot = _LIBM.hypot


def _std_min(a: float, b: float) -> float:
    return b if b < a else a      # std::min: a NaN second argument is never taken


def _std_max(a: float, b: float) -> float:
    return b if a < b else a


def _normalised_polygon(q) -> list:
    """Polygon2d::BuildFromPoints (polygon2d.cpp:206-234) on [n,2] vertices: the list of (x, y), reversed as a whole when
    the area sum of CrossProd(p0, p[i-1], p[i]) over i = 1 .. n-1 is negative."""
    pts = [(float(x), float(y)) for x, y in np.asarray(q, float).reshape(-1, 2)]
    x0, y0 = pts[0]
    area = 0.0
    for (ax, ay), (bx, by) in zip(pts[:-1], pts[1:]):
        area += (ax - x0) * (by - y0) - (ay - y0) * (bx - x0)
    return pts[::-1] if area < 0 else pts


def polygon_distance(q, px: float, py: float, normalise: bool = True) -> float:
    """Polygon2d::DistanceTo(Vec2d) (polygon2d.cpp:43-52) from (px, py) to the polygon of [n,2] vertices, n >= 1: 0.0
    inside (bounding box, then the crossing count), else the std::min over the edges, in order, of
    LineSegment2d::DistanceTo (line_segment2d.cpp:38-75).  Plain Python floats and the C library's hypot, every operation
    rounded once.  normalise = False measures the vertex array as given (what a test compares the rule against)."""
    pts = _normalised_polygon(q) if normalise else [(float(x), float(y)) for x, y in np.asarray(q, float).reshape(-1, 2)]
    n = len(pts)
    min_x = max_x = pts[0][0]
    min_y = max_y = pts[0][1]
    for x, y in pts:      # the box of the reversed array, by std::min / std::max from its first vertex
        min_x, max_x, min_y, max_y = _std_min(min_x, x), _std_max(max_x, x), _std_min(min_y, y), _std_max(max_y, y)
    if not (px < min_x or px > max_x or py < min_y or py > max_y):
        crossings, j = 0, n - 1
        for i in range(n):
            (xi, yi), (xj, yj) = pts[i], pts[j]
            if (yi > py) != (yj > py):
                side = (xi - px) * (yj - py) - (xj - px) * (yi - py)
                if (side > 0.0) if yi < yj else (side < 0.0):
                    crossings += 1
            j = i
        if crossings & 1:
            return 0.0
    d = math.inf
    for i in range(n):
        (sx, sy), (ex, ey) = pts[i], pts[0 if i >= n - 1 else i + 1]
        dx, dy = ex - sx, ey - sy
        length = _hypot(dx, dy)
        ux, uy = (0.0, 0.0) if length <= K_MATH_EPS else (dx / length, dy / length)
        x0, y0 = px - sx, py - sy
        if length <= K_MATH_EPS:
            e = _hypot(x0, y0)
        else:
            proj = x0 * ux + y0 * uy
            if proj <= 0.0:
                e = _hypot(x0, y0)
            elif proj >= length:
                e = _hypot(px - ex, py - ey)
            else:
                e = abs(x0 * uy - y0 * ux)
        d = _std_min(d, e)
    return d


def environment_clearance(center: np.ndarray, scene: Scene, cfg, times, poses, ego_trig=None, obstacle_trig=None) -> tuple:
    """How far the two vehicle discs stay from the obstacles at every knot (include/cilqr.h, "clearance"): (clearance [K,4]
    = rear disc / static, rear / dynamic, front / static, front / dynamic; nearest [K,4] int32 = index of the obstacle in
    scene.static / scene.dynamic, -1: none; min_clearance; min_knot).  times [K], poses [K,3] = x, y, theta; `center` is
    taken for the sake of the call's shape and not read (the road barriers are no column).  A dynamic obstacle is present
    and placed as in environment_collisions.  ego_trig / obstacle_trig(angle) -> (cos, sin): the math module's by default;
    a test hands in another implementation's (the device's) for the vehicle heading / the obstacle placement."""
    trig = lambda a: (math.cos(a), math.sin(a))
    ego_trig, obstacle_trig = ego_trig or trig, obstacle_trig or trig
    radius, r2x, f2x = vehicle_discs(cfg)
    K = len(times)
    clearance = np.full((K, 4), math.inf)
    nearest = np.full((K, 4), -1, dtype=np.int32)
    lowest, knot = math.inf, -1
    for k, (t, (x, y, th)) in enumerate(zip(times, poses)):
        t, x, y, th = float(t), float(x), float(y), float(th)
        ct, st = ego_trig(th)
        discs = ((x + r2x * ct, y + r2x * st), (x + f2x * ct, y + f2x * st))
        kinds = ([(o, np.asarray(p, float).reshape(-1, 2)) for o, p in enumerate(scene.static) if len(p) >= 1], [])
        for o, d in enumerate(scene.dynamic):
            tt = d.trajectory[:, 0]
            if len(d.polygon) < 1 or len(tt) < 1 or tt[0] > t or tt[-1] < t:
                continue
            i = 0
            while i < len(tt) and not (t < tt[i]):      # first sample with t < time; past the end the last
                i += 1
            _, ox, oy, oth = (float(v) for v in d.trajectory[min(i, len(tt) - 1)])
            c, s = obstacle_trig(oth)      # Pose::transform (pose.h:40-46): x + rx cos - ry sin, in that order
            kinds[1].append((o, [(ox + float(vx) * c - float(vy) * s, oy + float(vx) * s + float(vy) * c) for vx, vy in d.polygon]))
        for disc, (cx, cy) in enumerate(discs):
            for kind, polygons in enumerate(kinds):
                best, slot = math.inf, -1
                for o, q in polygons:
                    dist = polygon_distance(q, cx, cy)
                    if dist < best:
                        best, slot = dist, o
                clearance[k, 2 * disc + kind] = best - radius
                nearest[k, 2 * disc + kind] = slot
        for v in clearance[k]:
            if v < lowest:
                lowest, knot = float(v), k
    return clearance, nearest, lowest, knot


def road_barriers(center: np.ndarray) -> tuple:
    """left_road_barrier / right_road_barrier of the reference's Environment: the centre line shifted by
    +left_bound / -right_bound along its normal (ReferenceLine::GetCartesian at every centre point)."""
    x, y, th, lb, rb = center[:, 1], center[:, 2], center[:, 3], center[:, 5], center[:, 6]
    left = np.stack([x - lb * np.sin(th), y + lb * np.cos(th)], 1)
    right = np.stack([x + rb * np.sin(th), y - rb * np.cos(th)], 1)
    return left, right


def flatten_scene(center: np.ndarray, scene: Scene) -> dict:
    """The scene as the C-ABI's `cilqr_scene` takes it (include/cilqr.h): polygons and trajectories back to back."""
    def cat(arrs, width):
        return np.ascontiguousarray(np.concatenate(arrs, axis=0) if arrs else np.zeros((0, width)), dtype=np.float64)
    return dict(
        center=np.ascontiguousarray(center, dtype=np.float64),
        static_points=cat([np.asarray(p, float).reshape(-1, 2) for p in scene.static], 2),
        static_counts=np.asarray([len(p) for p in scene.static], dtype=np.int32),
        dynamic_polygon_points=cat([np.asarray(d.polygon, float).reshape(-1, 2) for d in scene.dynamic], 2),
        dynamic_polygon_counts=np.asarray([len(d.polygon) for d in scene.dynamic], dtype=np.int32),
        dynamic_trajectories=cat([np.asarray(d.trajectory, float).reshape(-1, 4) for d in scene.dynamic], 4),
        dynamic_trajectory_counts=np.asarray([len(d.trajectory) for d in scene.dynamic], dtype=np.int32))


def pack_scene_batch(center: np.ndarray, scenes: list, max_static: "int | None" = None, max_dynamic: "int | None" = None,
                     max_vertices: "int | None" = None, max_samples: "int | None" = None) -> dict:
    """A list of scenes on one road as the C-ABI's `cilqr_scene_batch` takes it (include/cilqr.h): a fixed number of
    obstacle slots per scene, every polygon padded to max_vertices vertices and every trajectory to max_samples samples
    (zeros), a count per slot -- 0 vertices = slot unused.  The max_* default to the largest the scenes need (at least 1);
    a scene that needs more than a given max_* is refused.  Returns dict(batch, max_static, max_dynamic, max_vertices,
    max_samples, center [n,7], static_points [B,S,V,2], static_counts [B,S], dynamic_polygon_points [B,D,V,2],
    dynamic_polygon_counts [B,D], dynamic_trajectories [B,D,T,4], dynamic_trajectory_counts [B,D])."""
    B = len(scenes)
    statics = [[np.asarray(p, float).reshape(-1, 2) for p in sc.static] for sc in scenes]
    dyns = [[(np.asarray(d.polygon, float).reshape(-1, 2), np.asarray(d.trajectory, float).reshape(-1, 4)) for d in sc.dynamic]
            for sc in scenes]
    need = dict(
        max_static=max((len(s) for s in statics), default=0),
        max_dynamic=max((len(d) for d in dyns), default=0),
        max_vertices=max([len(p) for s in statics for p in s] + [len(p) for d in dyns for p, _ in d], default=0),
        max_samples=max((len(t) for d in dyns for _, t in d), default=0))
    given = dict(max_static=max_static, max_dynamic=max_dynamic, max_vertices=max_vertices, max_samples=max_samples)
    size = {}
    for k, n in need.items():
        if given[k] is None:
            size[k] = max(1, n)
        elif n > given[k]:
            worst = {"max_static": lambda b: len(statics[b]), "max_dynamic": lambda b: len(dyns[b]),
                     "max_vertices": lambda b: max([len(p) for p in statics[b]] + [len(p) for p, _ in dyns[b]], default=0),
                     "max_samples": lambda b: max((len(t) for _, t in dyns[b]), default=0)}[k]
            b = max(range(B), key=worst)
            raise ValueError(f"scene {b} needs {k} = {n}, the batch is packed with {k} = {given[k]}")
        else:
            size[k] = int(given[k])
    for b in range(B):
        for p in statics[b] + [p for p, _ in dyns[b]]:
            if len(p) < 1:
                raise ValueError(f"scene {b} holds a polygon without vertices (0 vertices marks an unused slot)")
    S, D, V, T = size["max_static"], size["max_dynamic"], size["max_vertices"], size["max_samples"]
    out = dict(batch=B, center=np.ascontiguousarray(center, dtype=np.float64), **size,
               static_points=np.zeros((B, S, V, 2)), static_counts=np.zeros((B, S), dtype=np.int32),
               dynamic_polygon_points=np.zeros((B, D, V, 2)), dynamic_polygon_counts=np.zeros((B, D), dtype=np.int32),
               dynamic_trajectories=np.zeros((B, D, T, 4)), dynamic_trajectory_counts=np.zeros((B, D), dtype=np.int32))
    for b in range(B):
        for o, p in enumerate(statics[b]):
            out["static_points"][b, o, :len(p)] = p
            out["static_counts"][b, o] = len(p)
        for o, (p, t) in enumerate(dyns[b]):
            out["dynamic_polygon_points"][b, o, :len(p)] = p
            out["dynamic_polygon_counts"][b, o] = len(p)
            out["dynamic_trajectories"][b, o, :len(t)] = t
            out["dynamic_trajectory_counts"][b, o] = len(t)
    return out


def unpack_scene(packed: dict, b: int) -> dict:
    """Scene b of pack_scene_batch's arrays in the form of flatten_scene (the used slots, back to back)."""
    def cat(arrs, width):
        return np.ascontiguousarray(np.concatenate(arrs, axis=0) if arrs else np.zeros((0, width)), dtype=np.float64)
    sc, dc, tc = packed["static_counts"][b], packed["dynamic_polygon_counts"][b], packed["dynamic_trajectory_counts"][b]
    so, do = np.flatnonzero(sc > 0), np.flatnonzero(dc > 0)
    return dict(
        center=packed["center"],
        static_points=cat([packed["static_points"][b, o, :sc[o]] for o in so], 2),
        static_counts=sc[so].astype(np.int32),
        dynamic_polygon_points=cat([packed["dynamic_polygon_points"][b, o, :dc[o]] for o in do], 2),
        dynamic_polygon_counts=dc[do].astype(np.int32),
        dynamic_trajectories=cat([packed["dynamic_trajectories"][b, o, :tc[o]] for o in do], 4),
        dynamic_trajectory_counts=tc[do].astype(np.int32))


WINDOW_MARGIN = 1e-9   # include/cilqr.h, "scene window"


def _first_true(T: int, pred) -> int:
    """std::lower_bound's halving written out over a predicate (the window rule's two searches)."""
    first, n = 0, T
    while n > 0:
        half = n >> 1
        if not pred(first + half):
            first += half + 1
            n -= half + 1
        else:
            n = half
    return first


def window_bounds(times, t0: float, span: float) -> tuple:
    """(lo, hi) of the window rule for sample times [T]: the samples a scene that starts at t0 reads on 0 ... span;
    (0, -1) for T < 1."""
    s = np.asarray(times, dtype=np.float64) - np.float64(t0)
    T = len(s)
    if T < 1:
        return 0, -1
    upper = np.float64(span) + np.float64(WINDOW_MARGIN)
    L = _first_true(T, lambda k: not (s[k] < -WINDOW_MARGIN))
    H = _first_true(T, lambda k: bool(upper < s[k]))
    return max(0, L - 1), min(T - 1, H)


def window_trajectory(traj, t0: float, span: float) -> np.ndarray:
    """The window rule of include/cilqr.h ("scene window") in NumPy: the samples lo ... hi of traj [T,4] = time x y theta
    with the time column on the clock time - t0 (one rounding), the other columns untouched.  [count,4]."""
    traj = np.asarray(traj, dtype=np.float64).reshape(-1, 4)
    lo, hi = window_bounds(traj[:, 0], t0, span)
    out = traj[lo:hi + 1].copy()
    out[:, 0] = out[:, 0] - np.float64(t0)
    return out


def window_scene(scene: Scene, t0: float, span: float) -> Scene:
    """`scene` as a planning cycle that starts at scene time t0 reads it: every dynamic trajectory cut to its window."""
    return Scene(start=scene.start, coarse=scene.coarse, static=scene.static,
                 dynamic=[DynamicObstacle(polygon=d.polygon, trajectory=window_trajectory(d.trajectory, t0, span))
                          for d in scene.dynamic])


def shift_scene(scene: Scene, t0: float) -> Scene:
    """`scene` with every sample of every dynamic trajectory on the clock time - t0: what the window is cut out of."""
    def shifted(t):
        t = np.asarray(t, dtype=np.float64).reshape(-1, 4).copy()
        t[:, 0] = t[:, 0] - np.float64(t0)
        return t
    return Scene(start=scene.start, coarse=scene.coarse, static=scene.static,
                 dynamic=[DynamicObstacle(polygon=d.polygon, trajectory=shifted(d.trajectory)) for d in scene.dynamic])


PREDICT_MARGIN = 1e-9      # include/cilqr.h, "scene prediction"
PREDICT_MIN_STEP = 1e-10
PREDICT_HOLD, PREDICT_CONSTANT_VELOCITY = 0, 1


def predict_covers(out_samples: int, sample_dt: float, span: float) -> bool:
    """the span condition of the prediction calls: the last of out_samples samples lies past every query time of [0, span]"""
    return bool(np.float64(out_samples - 1) * np.float64(sample_dt) >= np.float64(span) + np.float64(PREDICT_MARGIN))


def predict_out_samples(sample_dt: float, span: float) -> int:
    """the smallest out_samples >= 2 that satisfies the span condition"""
    n = max(2, int(span / sample_dt))
    while not predict_covers(n, sample_dt, span):
        n += 1
    while n > 2 and predict_covers(n - 1, sample_dt, span):
        n -= 1
    return n


def predict_trajectory(traj, t0: float, mode: int, max_age: float, sample_dt: float, out_samples: int) -> np.ndarray:
    """The prediction rule of include/cilqr.h ("scene prediction") in NumPy: from the samples of traj [T,4] = time x y theta
    observed by t0 alone, out_samples samples on the clock 0, sample_dt, ... -- the latest observation held
    (PREDICT_HOLD) or moved on with the velocity of the last two (PREDICT_CONSTANT_VELOCITY), its heading kept as bits.
    [out_samples,4], or [0,4] for an obstacle that is unseen at t0 or older than max_age.  Every operation is rounded once."""
    traj = np.asarray(traj, dtype=np.float64).reshape(-1, 4)
    T = len(traj)
    none = np.zeros((0, 4))
    if T < 1:
        return none
    f = np.float64
    with np.errstate(all="ignore"):
        s = traj[:, 0] - f(t0)
        J = _first_true(T, lambda k: bool(PREDICT_MARGIN < s[k]))
        if J == 0:
            return none
        j = J - 1
        e = -s[j]
        if e > max_age:
            return none
        vx = vy = f(0.0)
        if mode == PREDICT_CONSTANT_VELOCITY and j >= 1:
            h = traj[j, 0] - traj[j - 1, 0]
            if h > PREDICT_MIN_STEP:
                vx = (traj[j, 1] - traj[j - 1, 1]) / h
                vy = (traj[j, 2] - traj[j - 1, 2]) / h
        x0 = traj[j, 1] + vx * e
        y0 = traj[j, 2] + vy * e
        tm = np.arange(int(out_samples), dtype=np.float64) * f(sample_dt)
        out = np.empty((int(out_samples), 4))
        out[:, 0] = tm
        out[:, 1] = x0 + vx * tm
        out[:, 2] = y0 + vy * tm
        out[:, 3] = traj[j, 3]
    return out


def predict_scene(scene: Scene, t0: float, mode: int, max_age: float, sample_dt: float, out_samples: int) -> Scene:
    """`scene` as a planning cycle that starts at scene time t0 and knows the samples up to t0 alone predicts it: every
    dynamic trajectory replaced by its prediction (no sample: the obstacle is not there for the scene calls)."""
    return Scene(start=scene.start, coarse=scene.coarse, static=scene.static,
                 dynamic=[DynamicObstacle(polygon=d.polygon,
                                          trajectory=predict_trajectory(d.trajectory, t0, mode, max_age, sample_dt, out_samples))
                          for d in scene.dynamic])


# ---------------------------------------------------------------------------------------------
# the reference's own scene artefact: reference.pickle
# ---------------------------------------------------------------------------------------------
# script/reference_publisher.py:232-236 dumps {"center": CenterLine, "static": Obstacles | None, "dynamic":
# DynamicObstacles | None} -- ROS message objects (genpy.Message: __slots__ in the field order of msg/*.msg and
# geometry_msgs, pickled as the list of slot values) -- with Python 2's text pickle; script/pickle_publisher.py:24-55
# replays it.  Reading it needs neither rospy nor the generated message modules: the unpickler below maps exactly
# these message classes to slot-ordered stand-ins and refuses everything else.
_MSG_SLOTS = {
    "CenterLine": ("points",),                                                   # msg/CenterLine.msg
    "CenterLinePoint": ("s", "x", "y", "theta", "kappa", "left_bound", "right_bound"),   # msg/CenterLinePoint.msg
    "Obstacles": ("obstacles",),                                                 # msg/Obstacles.msg
    "DynamicObstacles": ("obstacles",),                                          # msg/DynamicObstacles.msg
    "DynamicObstacle": ("polygon", "trajectory"),                                # msg/DynamicObstacle.msg
    "DynamicTrajectoryPoint": ("time", "x", "y", "theta"),                       # msg/DynamicTrajectoryPoint.msg
    "Polygon": ("points",),                                                      # geometry_msgs/Polygon
    "Point32": ("x", "y", "z"),                                                  # geometry_msgs/Point32
}
_MSG_MODULES = ("planning.msg", "geometry_msgs.msg")
_STUBS = {}


def _stub(name):
    if name not in _STUBS:
        slots = _MSG_SLOTS[name]

        def __setstate__(self, state, _slots=slots):           # genpy.Message.__setstate__: slot values in order
            for k, v in zip(_slots, state):
                setattr(self, k, v)

        _STUBS[name] = type(name, (object,), {"__setstate__": __setstate__, "_slots": slots})
    return _STUBS[name]


def _reference_unpickler(f):
    import pickle

    class U(pickle.Unpickler):
        def find_class(self, module, name):
            if module.split("._")[0] in _MSG_MODULES and name in _MSG_SLOTS:
                return _stub(name)
            if (module, name) in (("copy_reg", "_reconstructor"), ("copyreg", "_reconstructor")):
                import copyreg
                return copyreg._reconstructor
            if (module, name) in (("__builtin__", "object"), ("builtins", "object")):
                return object
            raise pickle.UnpicklingError(f"{module}.{name} is not part of a reference scene pickle")

    return U(f, encoding="latin1")


def from_reference_pickle(path: str, start=(0.0, 0.0, 0.0, 10.0), dt: float = 0.1) -> SceneFile:
    """The reference's reference.pickle -> a one-scene SceneFile (save() then gives the .cqs that
    include/cilqr/scene_file.hpp and the DP planner read).  `start` defaults to the state PlanningNode hard-codes
    (x = y = theta = 0, v = 10: algorithm/planning_node.cc:24-30); the scene carries no coarse trajectory (K = 0):
    that is what cilqr_dp_plan produces from it."""
    with open(path, "rb") as f:
        ref = _reference_unpickler(f).load()
    if not isinstance(ref, dict) or "center" not in ref:
        raise ValueError("not a reference scene pickle: no 'center'")
    center = np.array([[getattr(p, k) for k in _MSG_SLOTS["CenterLinePoint"]] for p in ref["center"].points], dtype=np.float64)
    static = []
    if ref.get("static") is not None:
        for poly in ref["static"].obstacles:                     # Obstacles.msg: geometry_msgs/Polygon[], world frame
            static.append(np.array([[q.x, q.y] for q in poly.points], dtype=np.float64))
    dynamic = []
    if ref.get("dynamic") is not None:
        for ob in ref["dynamic"].obstacles:
            poly = np.array([[q.x, q.y] for q in ob.polygon.points], dtype=np.float64)      # body frame
            traj = np.array([[t.time, t.x, t.y, t.theta] for t in ob.trajectory], dtype=np.float64).reshape(-1, 4)
            dynamic.append(DynamicObstacle(poly, traj))
    return SceneFile(float(dt), center, [Scene(np.asarray(start, dtype=np.float64), np.zeros((0, 6)), static, dynamic)])
