"""Crafted centre lines and queries for the Frenet rule (include/cilqr.h, "frenet"), shared by tests/test_frenet.py (host
calls, NumPy statement, reference, sanitizer program) and tests/test_gpu_frenet.py (kernels).

A case is a centre line [n][7] = s x y theta kappa left_bound right_bound with its query points [M][2]; it names the
branches of the rule its queries must reach (frenet.branch_of), and the census of the test asserts that each branch is hit
over the table.  `on_line` counts the queries of a case that lie on the line exactly (nr = 0: the sign of the lateral
offset means nothing there).  Lines on dyadic coordinates with heading 0 make distances, ties and projections exact.
"""
import struct
from collections import namedtuple

import numpy as np

from cilqr_amd import api, frenet

TILE = 512          # kFrTile of cilqr_amd/csrc/frenet.hpp: centre points per LDS tile of the scan
WIDE_FROM = 262144  # kFrWideFrom: from this many queries a lane owns four of them
LAYOUTS = (api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE, api.ROWS_POINTS)
X_COLUMN = {api.ROWS_TRAJ: 1, api.ROWS_PLAN: 2, api.ROWS_COARSE: 2, api.ROWS_POINTS: 0}
BRANCHES = ("clamp_low", "clamp_high", "interior", "tie", "no_distance", "degenerate", "w_below_0", "w_above_1", "w_inside",
            "w_nan", "on_line")

Case = namedtuple("Case", "name center points branches on_line")
Inverse = namedtuple("Inverse", "name center sl")


def dyadic_line(n, step=1.0, x0=0.0, y0=0.0):
    """a straight line along +x on exactly representable coordinates; kappa and the bounds vary from point to point, not
    linearly, so that the pair a result was interpolated from shows in it"""
    i = np.arange(n, dtype=np.float64)
    c = np.zeros((n, 7))
    c[:, 0] = i * step
    c[:, 1] = x0 + i * step
    c[:, 2] = y0
    c[:, 4] = 0.001 * np.sin(0.7 * i)
    c[:, 5] = 3.0 + 0.25 * np.cos(1.3 * i)
    c[:, 6] = 4.0 + 0.25 * np.sin(0.9 * i)
    return c


def curved_line(rng, n, theta0=None, wrap=False):
    """a road-like line in the style of test_reference_pins._trajectory; headings unwrapped unless asked otherwise"""
    theta = 0.4 * np.sin(np.linspace(0, 2.5, n) + rng.uniform(0, 6)) + (rng.uniform(-3, 3) if theta0 is None else theta0)
    step = rng.uniform(0.3, 1.2, n)
    x = np.cumsum(step * np.cos(theta)) + rng.uniform(-20, 20)
    y = np.cumsum(step * np.sin(theta)) + rng.uniform(-20, 20)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    if wrap:
        theta = np.arctan2(np.sin(theta), np.cos(theta))
    return np.ascontiguousarray(np.stack([s, x, y, theta, np.gradient(theta) / step, rng.uniform(2, 5, n), rng.uniform(2, 5, n)], axis=1))


def road_center():
    """the generator's road (scenario.build_road: 1952 points 0.1 m apart, unwrapped headings) as a centre line"""
    from cilqr_amd import scenario
    road = scenario.build_road()
    n = len(road.s)
    return np.ascontiguousarray(np.stack([road.s, road.x, road.y, road.theta, road.kappa, np.full(n, scenario.LEFT_BOUND),
                                          np.full(n, scenario.RIGHT_BOUND)], 1))


def points_on_road(rng, center, m, half_width=2.0):
    """m points within `half_width` of the centre line, between its points as well as on them"""
    i = rng.integers(0, len(center) - 1, m)
    t = rng.uniform(0.0, 1.0, m)[:, None]
    base = (1 - t) * center[i, 1:3] + t * center[i + 1, 1:3]
    off = rng.uniform(-half_width, half_width, m)
    return base + off[:, None] * np.stack([-np.sin(center[i, 3]), np.cos(center[i, 3])], axis=1)


def points_beside(rng, center, m, spread=2.0):
    i = rng.integers(0, len(center), m)
    return center[i, 1:3] + rng.normal(0, spread, (m, 2))


def line_queries(center):
    """crafted queries for a dyadic_line of any n >= 2: (name, x, y, lies on the line)"""
    n = len(center)
    step = center[1, 1] - center[0, 1]
    x0, y0, xl = center[0, 1], center[0, 2], center[-1, 1]
    q = [("before the first point", x0 - 2.5 * step, y0 + 0.5, False), ("beyond the last point", xl + 3.25 * step, y0 - 0.75, False),
         ("beside the first point", x0 + 0.125 * step, y0 + 1.0, False), ("beside the last point", xl - 0.125 * step, y0 - 1.0, False),
         ("on the first point", x0, y0, True), ("on the last point", xl, y0, True),
         ("NaN x", np.nan, y0 + 1.0, False), ("NaN y", x0 + step, np.nan, False), ("infinite x", np.inf, y0, False),
         ("infinite x and y", -np.inf, np.inf, False), ("infinite y", x0, -np.inf, False), ("far away", 1e150, -3e149, False)]
    if n >= 3:
        mid = n // 2
        q += [("on a centre point", center[mid, 1], y0, True), ("on a chord", center[mid, 1] + 0.25 * step, y0, True),
              ("tie of two points", center[mid, 1] - 0.5 * step, y0 + 0.75, False),
              ("tie of the first two points", x0 + 0.5 * step, y0 - 0.25, False),
              ("tie of the last two points", xl - 0.5 * step, y0 + 1.5, False)]
    for edge in range(TILE, n, TILE):          # the same tie at indices edge - 1 and edge
        q.append((f"tie across tile edge {edge}", center[edge, 1] - 0.5 * step, y0 + 0.75, False))
    return q


def _case(name, center, points, branches, on_line=0):
    return Case(name, np.ascontiguousarray(center, dtype=np.float64), np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2),
                tuple(branches), on_line)


def crafted_cases():
    rng = np.random.default_rng(911)
    cases = []
    for n, name in ((2, "two centre points"), (3, "three centre points"), (9, "nine centre points"),
                    (TILE + 8, "a line past one tile"), (2 * TILE + 5, "a line past two tiles")):
        c = dyadic_line(n, step=0.5 if n < 100 else 1.0, x0=-2.0, y0=1.0)
        q = line_queries(c)
        br = ["clamp_low", "clamp_high", "w_below_0", "w_above_1", "no_distance", "w_nan", "on_line"]
        if n >= 3:
            br += ["tie"]
        if n >= 9:
            br += ["interior", "w_inside"]
        cases.append(_case(name, c, [[x, y] for _, x, y, _ in q], br, sum(1 for v in q if v[3])))
    # duplicated centre points: rows 4 and 5 are one point, stations included -- equidistant from everything, the first wins
    c = dyadic_line(9)
    c[5] = c[4]
    cases.append(_case("duplicated centre points", c, [[4.0, 0.5], [4.25, -0.5], [3.75, 1.0], [5.0, 0.25]], ["tie", "interior"]))
    # |s[at+1] - s[at-1]| < 1e-10: the result is row at-1 as bits, not the nearest row
    c = dyadic_line(9)
    c[4:7, 0] = [4.0, 4.0 + 2e-11, 4.0 + 5e-11]
    c[4, 3], c[4, 4] = 3 * np.pi + 0.01, -0.0            # bits that an interpolation would not return
    cases.append(_case("degenerate pair", c, [[5.0, 0.5], [5.125, -2.0], [4.875, 0.0]], ["degenerate", "interior"]))
    # stations exactly 1e-10 apart: interpolated (slerp's own `<=` then returns NormalizeAngle(theta of row i0))
    c = dyadic_line(5)
    c[:, 0] = [-1.0, 0.0, 5e-11, 1e-10, 1.0]
    c[:, 3] = [0.1, 0.2, 0.3, 0.4, 0.5]
    assert not abs(c[3, 0] - c[1, 0]) < 1e-10 and abs(c[3, 0] - c[1, 0]) <= 1e-10
    cases.append(_case("stations exactly 1e-10 apart", c, [[2.0, 0.5], [2.25, -1.0]], ["interior"]))
    # c[i0] and c[i1] on one spot: 0 / 0
    c = dyadic_line(9)
    c[3, 1:3] = c[5, 1:3] = [4.0, 2.0]
    cases.append(_case("coincident pair", c, [[4.0, 0.25], [4.0, -1.0]], ["w_nan"]))
    # headings: either side of +-pi on a line that runs along -x, and unwrapped ones
    c = curved_line(rng, 12, theta0=np.pi)
    c[:, 3] = np.where(np.arange(12) % 2 == 0, 3.10, -3.12) + 0.003 * np.arange(12)
    cases.append(_case("headings either side of pi", c, points_beside(rng, c, 40, 1.0), ["interior", "w_inside"]))
    c = curved_line(rng, 12, theta0=np.pi)
    c[:, 3] += 2 * np.pi * np.arange(12).clip(0, 3)        # 3 pi, 5 pi, 7 pi ...
    cases.append(_case("unwrapped headings", c, points_beside(rng, c, 40, 1.0), ["interior", "w_inside"]))
    # a NaN row in the centre line: never the nearest, but part of the pairs of its neighbours
    c = curved_line(rng, 12)
    pts = np.concatenate([c[[3, 4, 5], 1:3] + 0.1, points_beside(rng, c, 20), c[[0, 11], 1:3] - 0.2])
    c[4] = np.nan
    cases.append(_case("NaN row in the centre line", c, pts, ["interior", "w_nan", "w_inside"]))
    return cases


def random_cases(n_lines=300, points=50, seed=912):
    """300 lines in the style of test_reference_pins._trajectory, n in {2, 3, 10, 60, 250}, 50 points each: beside the
    line, on centre points, before and beyond its ends"""
    rng = np.random.default_rng(seed)
    cases = []
    for j in range(n_lines):
        n = (2, 3, 10, 60, 250)[j % 5]
        c = curved_line(rng, n, wrap=(j % 3 == 1))
        pts = np.concatenate([points_beside(rng, c, points - 4), c[rng.integers(0, n, 2), 1:3], c[:1, 1:3] - 10.0, c[-1:, 1:3] + 10.0])
        cases.append(_case(f"random {j}", c, pts, ()))
    return cases


def inverse_cases():
    """(station, lateral) pairs: stations before, on, between and past the knots; lateral 0, +, -, NaN"""
    rng = np.random.default_rng(913)
    out = []
    for name, c in (("curved", curved_line(rng, 40)), ("two points", curved_line(rng, 2)), ("dyadic", dyadic_line(9)),
                    ("unwrapped", crafted_by_name("unwrapped headings").center), ("degenerate", crafted_by_name("degenerate pair").center),
                    ("1e-10", crafted_by_name("stations exactly 1e-10 apart").center), ("NaN row", crafted_by_name("NaN row in the centre line").center)):
        s = c[:, 0]
        lo, hi = np.nanmin(s), np.nanmax(s)
        stations = np.concatenate([[lo - 3.0, lo - 1e-13, lo, hi, hi + 1e-13, hi + 7.0, np.nan, np.inf, -np.inf], s[np.isfinite(s)][::3],
                                   rng.uniform(lo, hi, 12), [5e-11, 4.0 + 1e-11]])
        sl = np.array([[st, lat] for st in stations for lat in (0.0, 1.75, -2.5, np.nan)])
        out.append(Inverse(name, c, sl))
    return out


_CRAFTED = None


def crafted_by_name(name):
    global _CRAFTED
    if _CRAFTED is None:
        _CRAFTED = {c.name: c for c in crafted_cases()}
    return _CRAFTED[name]


def census(cases):
    seen = dict.fromkeys(BRANCHES, 0)
    for c in cases:
        for px, py in c.points.tolist():
            for b in frenet.branch_of(c.center, px, py):
                seen[b] += 1
    return seen


def rows_in_layout(layout, xy, rng=None):
    """xy [..., 2] as rows of `layout`: x, y in their columns, every other column filled (random, or 0.5)"""
    xy = np.asarray(xy, dtype=np.float64)
    F, xc = api.FRENET_ROWS_FIELDS[layout], X_COLUMN[layout]
    rows = np.full(xy.shape[:-1] + (F,), 0.5) if rng is None else rng.uniform(-9.0, 9.0, xy.shape[:-1] + (F,))
    rows[..., xc:xc + 2] = xy
    return np.ascontiguousarray(rows)


def same_frenet(got, want, cross=None):
    """resample_cases.same_rows on [..., 8] rows; where `cross` (the cross product behind the sign of lateral) is a NaN
    the sign of column 1 is that NaN's and not part of the rule: |lateral| is compared there"""
    from resample_cases import same_rows
    got, want = np.array(got, dtype=np.float64), np.array(want, dtype=np.float64)
    if cross is not None:
        loose = np.isnan(np.asarray(cross)).reshape(got.shape[:-1])
        got[..., 1] = np.where(loose, np.abs(got[..., 1]), got[..., 1])
        want[..., 1] = np.where(loose, np.abs(want[..., 1]), want[..., 1])
    return same_rows(got, want)


def write_cases(path, cases, layout, inverses):
    """The cases as tests/cpp/frenet_test.cc reads them (little-endian): "FCASES01", i32 n_cases, i32 n_inverses; per case
    i32 layout, i32 n_center, i32 M, center [n][7], rows [M][F], expected [M][8], cross [M] (the NumPy statement's); per
    inverse i32 n_center, i32 M, center, sl [M][2], expected [M][3]."""
    with open(path, "wb") as o:
        o.write(b"FCASES01" + struct.pack("<ii", len(cases), len(inverses)))
        for c in cases:
            rows = rows_in_layout(layout, c.points)
            want, cross, _ = frenet.frenet_rows(c.center, c.points)
            o.write(struct.pack("<iii", layout, len(c.center), len(rows)))
            o.write(c.center.astype("<f8").tobytes() + rows.astype("<f8").tobytes() + want.astype("<f8").tobytes() + cross.astype("<f8").tobytes())
        for v in inverses:
            want = frenet.cartesian_points(v.center, v.sl)
            o.write(struct.pack("<ii", len(v.center), len(v.sl)))
            o.write(v.center.astype("<f8").tobytes() + v.sl.astype("<f8").tobytes() + want.astype("<f8").tobytes())
