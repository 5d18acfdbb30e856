"""Scenes at the declared limits of the scene kernels (include/cilqr.h: 8 vertices per polygon, 32 static and 32 dynamic
slots, 1024 trajectory samples, 256 knots / path samples) for tests/test_scene_limits.py and
tests/test_gpu_scene_limits.py.  A helper module: nothing here is collected.

corner_scenes() takes the scenes of scenario.generate(..., scenarios=True) / scene_io.from_generator (min_clearance =
-1.0, as in the other scene tests), keeps every scene's start and the road, and replaces the obstacles by S static and D
dynamic ones drawn from a Philox stream per (seed, scene):

  polygons      3 .. V vertices (the first static and the first dynamic obstacle: exactly V) from jittered, ascending
                angles and random radii around a centre; a third of those with five and more vertices have one radius
                pulled in (concave); every second one is handed over clockwise; 0.3 - 1.5 m, and in every fourth scene
                one static and one dynamic obstacle of 10 - 14 m that reaches into the right edge of the road: a
                collision square can lie inside it with none of its vertices inside the square; in every sixteenth
                scene the static one lies across the road where the ego stands, so that the planner finds no path;
  static        placed by (station, lateral offset) through road.eval; three in four beside the drivable width;
  dynamic       1 .. T samples (the first obstacle: exactly T) at sorted uniform times -- no multiples of delta_t -- in
                a window that starts before or after 0 and ends before or after tf; poses follow the road with a lateral
                drift plus a heading offset.  Obstacles 1 .. 5 carry the ties (TIES): a sample time, a first and a last
                sample exactly equal to a path-sample time of the DP planner (dp_sample_times: the planner's own
                expression), a trajectory of one sample, two consecutive samples with one time; they are on the road
                more often than the others, and the samples behind a tied one stand 3 m to the side of it.
"""
import dataclasses

import numpy as np

from cilqr_amd import scenario, scene_io

N_LAYERS = 5                      # dp_planner.h:27
GEOM_EPS, DP_EPS = 1e-10, 1e-3    # math::kMathEpsilon; dp_planner.cpp:25
TIES = ("sample", "first", "last", "single", "twin")     # dynamic obstacle 1 + index carries that tie
# what the tests plan these scenes with: the generator's road is 195 m long, which the long horizon covers at 10 m/s
ROWS = {
    "full_8s": dict(S=32, D=32, V=8, T=1024, tf=8.0, over={}),
    "full_25s": dict(S=32, D=32, V=8, T=1024, tf=25.5, over=dict(max_velocity=10.0)),
    "budget_5s": dict(S=7, D=32, V=8, T=200, tf=5.0, over={}),
    "small_5s": dict(S=3, D=4, V=7, T=64, tf=5.0, over={}),
}


def dp_lattice(tf, delta_t=0.1):
    """The time lattice of DpPlanner (include/cilqr/dp_planner.hpp): (unit_time, layer times [5], path samples per
    layer [5]) -- the constructor's LinSpaced and the counting loop of CountSegmentPoints, statement by statement."""
    unit_time = tf / N_LAYERS
    step = (tf - unit_time) / (N_LAYERS - 1)
    time = [unit_time + step * i for i in range(N_LAYERS)]
    nseg = [0] * N_LAYERS
    t = 0.0
    while t < tf + delta_t - GEOM_EPS:
        for layer in range(N_LAYERS):
            if layer == 0:
                if t > 0.0 - DP_EPS and t < unit_time + DP_EPS:
                    nseg[0] += 1
            elif t > time[layer] - unit_time + GEOM_EPS and t < time[layer] + GEOM_EPS:
                nseg[layer] += 1
        t += delta_t
    return unit_time, time, nseg


def dp_counts(tf, delta_t=0.1):
    """(n_knots, nq): the knots the C-ABI asks for and the path samples the planner produces."""
    return int(tf / delta_t + 1), sum(dp_lattice(tf, delta_t)[2])


def dp_sample_times(tf, delta_t=0.1):
    """The time of every path sample, by the planner's expression from_time + i * (unit_time / nseg)."""
    unit_time, time, nseg = dp_lattice(tf, delta_t)
    out = []
    for layer in range(N_LAYERS):
        from_time = 0.0 if layer == 0 else time[layer - 1]
        out += [from_time + i * (unit_time / nseg[layer]) for i in range(nseg[layer])]
    return np.array(out)


def signed_area(q):
    """The sum of Polygon2d::BuildFromPoints (polygon2d.cpp:212-220): negative = clockwise."""
    return sum((q[i - 1, 0] - q[0, 0]) * (q[i, 1] - q[0, 1]) - (q[i - 1, 1] - q[0, 1]) * (q[i, 0] - q[0, 0]) for i in range(1, len(q)))


def is_concave(q):
    e = np.roll(q, -1, axis=0) - q
    cross = e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0]
    return bool((cross > 0).any() and (cross < 0).any())


def _polygon(rng, n, size, concave, clockwise):
    ang = 2 * np.pi * (np.arange(n) + 0.4 * rng.random(n)) / n + rng.uniform(0, 2 * np.pi)
    rad = size * rng.uniform(0.6, 1.0, n)
    if concave and n >= 5:
        rad[rng.integers(n)] *= 0.1
    q = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    return np.ascontiguousarray(q[::-1]) if clockwise else q


def _beside(rng, on_road):
    """A lateral offset: on the road (right bound 6 m, left bound 2.5 m) or beside it."""
    if rng.random() < on_road:
        return rng.uniform(-5.5, 2.0)
    return rng.uniform(4.5, 9.0) if rng.random() < 0.5 else -rng.uniform(8.0, 12.5)


def _vertex_count(b, o, V):
    """V for the first obstacle; behind it every count from 3 to V in turn, shifted from scene to scene."""
    return V if o == 0 else 3 + (o - 1 + b) % (V - 2)


def _large_polygon(rng, n, clockwise):
    """10 - 14 m, nearly round: (the polygon, its largest radius)."""
    size = rng.uniform(10.0, 14.0)
    body = _polygon(rng, n, size, False, clockwise)
    return body / np.hypot(body[:, 0], body[:, 1])[:, None] * size * rng.uniform(0.93, 1.0, (n, 1)), size


def corner_scene(scene, road, rng, b, S, D, V, T, tf, reach, sample_times, on_road=0.25, delta_t=0.1):
    """One scene: the start of `scene`, S static and D dynamic obstacles as the module text says."""
    s0 = float(road.s[np.argmin((road.x - scene.start[0]) ** 2 + (road.y - scene.start[1]) ** 2)])
    far = max(s0 + 12.0, min(s0 + reach, road.length - 1.0))
    big = b % 4 == 1
    static = []
    for o in range(S):
        n = _vertex_count(b, o, V)
        if big and o == 2:
            body, size = _large_polygon(rng, n, o % 2 == 1)
            s, l = rng.uniform(s0 + 10.0, far), -(0.93 * size + rng.uniform(2.5, 4.5))
            if b % 16 == 5:      # ... and in every sixteenth scene it lies across the road where the ego stands: no path
                s, l = s0 + rng.uniform(0.0, 4.0), -1.75
        else:
            body = _polygon(rng, n, rng.uniform(0.3, 1.5), rng.random() < 1 / 3, o % 2 == 1)
            s, l = rng.uniform(s0 + 6.0, far), _beside(rng, on_road)
        x, y, th, _ = road.eval(np.array([s]))
        static.append(body + [x[0] - l * np.sin(th[0]), y[0] + l * np.cos(th[0])])
    dynamic = []
    for o in range(D):
        n = _vertex_count(b, o, V)
        large = big and o == 7
        if large:
            body, size = _large_polygon(rng, n, o % 2 == 1)
        else:
            body = _polygon(rng, n, rng.uniform(0.3, 1.5), rng.random() < 1 / 3, o % 2 == 1)
        tie = TIES[o - 1] if 1 <= o <= len(TIES) else None
        m = T if o == 0 else 1 if tie == "single" else int(rng.integers(1, T + 1))
        if tie in ("sample", "twin"):
            m = max(m, 4)
        m = min(m, T)
        # the window: starts before / after 0, ends before / after tf; a few miss [0, tf] altogether
        kind = int(rng.integers(10)) % (4 if tie else 10)
        t0 = rng.uniform(-3.0, -0.2) if kind % 4 in (0, 1) else rng.uniform(0.05, 0.45) * tf
        t1 = rng.uniform(0.55, 0.95) * tf if kind % 4 in (0, 2) else tf + rng.uniform(0.2, 3.0)
        if kind == 8:
            t0, t1 = -4.0, -0.3
        elif kind == 9:
            t0, t1 = tf + 0.3, tf + 4.0
        tt = np.sort(rng.uniform(t0, t1, m))
        inside = sample_times[(sample_times > t0) & (sample_times < t1)]
        # (the first layer holds one sample more than the others: where a layer's samples fall on knot times -- to an ulp
        # or so --, the tie is taken there and so lies inside the 1e-10 window of the points kernel as well)
        on_knot = inside[np.abs(inside / delta_t - np.round(inside / delta_t)) * delta_t < 1e-12]
        inside = on_knot if len(on_knot) else inside
        pick = float(inside[rng.integers(len(inside))]) if len(inside) else float(sample_times[len(sample_times) // 2])
        if tie == "sample":
            tt = np.sort(np.concatenate([rng.uniform(t0, pick, (m - 1) // 2), [pick], rng.uniform(pick, t1, m - 1 - (m - 1) // 2)]))
        elif tie == "first":
            tt = np.sort(np.concatenate([[pick], rng.uniform(pick, max(t1, pick + 0.5), m - 1)]))
        elif tie == "last":
            tt = np.sort(np.concatenate([rng.uniform(min(t0, pick - 0.5), pick, m - 1), [pick]]))
        elif tie == "single":
            tt = np.array([pick])
        elif tie == "twin" and m >= 3:
            tt[m // 2] = tt[m // 2 - 1]
        l0 = -(0.93 * size + rng.uniform(2.5, 4.5)) if large else _beside(rng, 0.6 if tie else on_road)
        drift = 0.0 if large else rng.uniform(-0.3, 0.3)
        s = rng.uniform(s0 + 8.0, far) + rng.uniform(0.0, 8.0) * tt
        l = l0 + drift * tt
        # the neighbour of a tie stands 3 m to the side: taking it for the tie moves the polygon by more than its size
        if tie == "sample":
            l[int(np.flatnonzero(tt == pick)[0]) + 1:] += 3.0
        elif tie == "twin" and m >= 3:
            l[m // 2] += 3.0
        x, y, th, _ = road.eval(s)
        dynamic.append(scene_io.DynamicObstacle(body, np.ascontiguousarray(np.stack(
            [tt, x - l * np.sin(th), y + l * np.cos(th), th + rng.uniform(-0.6, 0.6) + 0.05 * tt], axis=1))))
    return scene_io.Scene(scene.start.copy(), scene.coarse.copy(), static, dynamic)


def corner_scenes(n, seed, S, D, V, T, tf, over=None, family="mix11", on_road=0.25, delta_t=0.1):
    """n scenes of the corner (S, D, V, T) for a plan over tf: (generator dict, SceneFile, overrides of the DP config)."""
    over = dict(over or {})
    spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True)
    sf = scene_io.from_generator(sc)
    reach = tf * over.get("max_velocity", 10.0)
    times = dp_sample_times(tf, delta_t)
    scenes = []
    for b in range(n):
        rng = np.random.Generator(np.random.Philox(key=seed + 7919, counter=[0, 0, 0, b]))
        scenes.append(corner_scene(sf.scenes[b], sc["road"], rng, b, S, D, V, T, tf, reach, times, on_road, delta_t))
    return sc, scene_io.SceneFile(sf.dt, sf.center, scenes), over
