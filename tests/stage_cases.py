"""A crafted table of knot cases for the cost and quadratise stages, and the packer that lays them into problem batches, for
tests/test_stage_reference.py and tests/test_gpu_stages.py.  A helper module: nothing here is collected.

A case is one knot: a state, a control, a goal and the raw corridor planes of the knot; all cases of a table share one pair of
lane tables (lanes()) and one configuration.  Everything is generated deterministically from the configuration; the only random
numbers are those of a few dozen seeded fillers.

What the barriers see is not a distance in metres: the load stage shrinks a plane (a, b, c) by the disc radius (+ safe margin
for corridor planes) and then divides it by hypot(hypot(a, b), c) -- the norm of all THREE coefficients -- so a constraint value
is g = s (signed distance) / hypot(s, c'), s = |(a, b)|.  plane_at() therefore places a plane either by its signed distance
in metres from a point or by the value g it shall have there.

Two consequences for the cases the table was asked to hold:
  * A bound's "double for which the subtraction gives exactly -eps" exists only where bound -+ eps is a double.  With
    eps = 0.01 that is the lower bound of v alone (g = 0 - v); every bound has one under the configuration "dyadic_eps"
    (eps = 2^-6), which is why that configuration is part of CONFIGS.  Where none exists the case sits on the nearest double on
    the relaxed side (its neighbour is then the nearest on the log side): an edge one ulp wide instead of a point.
  * A plane "1e5 m away" only produces a large factor when it is far from the VEHICLE with a small offset c' of its own, since
    |g| <= hypot(|p|, 1): the far family puts the vehicle 4e4 m from planes through the origin's neighbourhood (the only
    coordinates beyond 1e3 m).  4e4 and not 1e5 because the kernels renormalise the running product every 64 planes:
    (4e4)^64 = 1e294 is inside double range, (4e4)^70 = 1e322 is not, and (1e5)^64 = 1e320 would leave it between two
    renormalisations -- outside what the kernels document (factors up to 1e3) and not what the family is there to catch.
"""
import math

import numpy as np

N_STEPS = 7
K = N_STEPS + 1
CMAX_GROUPS = (1, 2, 5, 16, 70)
MAIN_CMAX = 16
FAR = 4.0e4

CONFIGS = {
    "default": {},
    "discs3": dict(num_of_disc=3),
    "discs7": dict(num_of_disc=7),
    "barrier": dict(barrier_t=10.0, barrier_eps=0.05),
    "weights": dict(w_x=0.6, w_y=0.9, w_theta=0.4, w_v=0.3, w_a=0.2, w_delta=0.7, w_jerk=1.5, w_delta_rate=2.5),
    "dyadic_eps": dict(barrier_eps=2.0 ** -6),
}


# ---------------------------------------------------------------------------------------------
# what the load stage makes of planes and lane rows, in plain doubles (checked against the oracle's bit for bit)
# ---------------------------------------------------------------------------------------------
def disc_radius(cfg):
    length = cfg.front_hang + cfg.wheel_base + cfg.rear_hang
    return float(np.hypot(cfg.width / 2.0, length / 2.0 / cfg.num_of_disc))


def disc_offsets(cfg):
    L = (cfg.rear_hang + cfg.wheel_base + cfg.front_hang) / cfg.num_of_disc
    return np.array([L * (j - 0.5) - cfg.rear_hang for j in range(cfg.num_of_disc)])


def _shrink_normalise(abc, by):
    abc = np.asarray(abc, np.float64)
    a, b, c = abc[..., 0], abc[..., 1], abc[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = c - by * (a * a + b * b) / np.hypot(a, b)
        norm = np.hypot(np.hypot(a, b), c)
        return np.stack([a / norm, b / norm, c / norm], axis=-1)


def processed_planes(raw, cfg):
    return _shrink_normalise(raw, disc_radius(cfg) + cfg.safe_margin)


def processed_lanes(rows, cfg):
    return _shrink_normalise(np.asarray(rows)[:, :3], disc_radius(cfg))


def plane_at(cfg, point, phi, scale, metres=None, g=None):
    """Raw plane with normal scale * (cos phi, sin phi) that the stages see at signed distance `metres` from `point` (negative
    = inside), or with constraint value `g` there."""
    s = float(scale)
    a, b = s * math.cos(phi), s * math.sin(phi)
    m = a * point[0] + b * point[1]
    if metres is not None:
        c2 = m - metres * s
    else:
        c2 = (m - g * math.sqrt(m * m + s * s * (1.0 - g * g))) / (1.0 - g * g)
    return [a, b, c2 + (disc_radius(cfg) + cfg.safe_margin) * s]


# ---------------------------------------------------------------------------------------------
# lane tables: a road along +x, 8 m wide, that bends left by atan(0.1) at x = 10; boundary points every 5 m from -40 to 60
# ---------------------------------------------------------------------------------------------
def lanes():
    xs = np.arange(-40.0, 60.0 + 1e-9, 5.0)
    bend = np.where(xs > 10.0, 0.1 * (xs - 10.0), 0.0)

    def rows(sx, sy, ex, ey):
        a, b = ey - sy, -(ex - sx)
        return np.ascontiguousarray(np.stack([a, b, a * sx + b * sy, sx, sy, ex, ey], axis=1))

    ly, ry = 4.0 + bend, -4.0 + bend
    return rows(xs[1:], ly[1:], xs[:-1], ly[:-1]), rows(xs[:-1], ry[:-1], xs[1:], ry[1:])


# ---------------------------------------------------------------------------------------------
# exact edges
# ---------------------------------------------------------------------------------------------
def _steps(x, ks):
    """x moved by k ulps, for every k of ks (doubles)."""
    x = np.float64(x)
    bits = np.array([x]).view(np.int64)[0]
    sign = 1 if x >= 0 else -1
    return (bits + sign * np.asarray(ks, np.int64)).view(np.float64)


def bound_edge(bound, upper, eps):
    """(value on the edge, its neighbour on the log side, does the subtraction give exactly -eps?) for g = value - bound (upper)
    or bound - value."""
    centre = bound - eps if upper else bound + eps
    cand = _steps(centre, np.arange(-8, 9))
    g = cand - bound if upper else bound - cand
    hit = np.nonzero(g == -eps)[0]
    if hit.size:
        i = int(hit[0])
    else:
        relaxed = np.nonzero(g > -eps)[0]
        i = int(relaxed[np.argmin(g[relaxed])])
    x = cand[i]
    log_side = [c for c, gg in zip(cand, g) if gg < -eps]
    nb = min(log_side, key=lambda c: abs(c - x))
    return float(x), float(nb), bool(hit.size)


def scan_exact(g_of, x0, eps, span=200000):
    """The double nearest x0, within `span` ulps, at which g_of (doubles in, doubles out, the kernels' expression order) gives
    exactly -eps; None if there is none."""
    ks = np.arange(-span, span + 1)
    xs = _steps(x0, ks)
    hit = np.nonzero(g_of(xs) == -eps)[0]
    if not hit.size:
        return None
    return float(xs[hit[np.argmin(np.abs(ks[hit]))]])


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
def _neutral(k=0):
    x = np.array([2.3 + 0.013 * (k % 17), 0.2 - 0.011 * (k % 5), 0.03 + 0.002 * (k % 7), 8.0 + 0.1 * (k % 9), 0.5, 0.05])
    u = np.array([1.0 + 0.05 * (k % 4), 0.02])
    return x, u


def _box(cfg, x, n=4, k=0):
    """n planes well clear of the vehicle (every disc on the log branch)"""
    return [plane_at(cfg, x[:2], 0.4 + 2.0 * math.pi * i / n + 0.05 * k, 0.5 + (i % 3), metres=-(4.0 + (i + k) % 5)) for i in range(n)]


def _case(cls, name, x, u, planes, cmax, tie=False):
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    goal = x[:3] + np.array([0.3, -0.2, 0.05])
    planes = np.asarray(planes, np.float64).reshape(-1, 3)
    assert planes.shape[0] <= cmax
    return dict(cls=cls, name=name, x=x, u=u, goal=goal, planes=planes, cmax=cmax, tie=tie)


def _bound_cases(cfg):
    eps = float(cfg.barrier_eps)
    out = []
    bounds = [("v", 3, 0.0, False), ("v", 3, cfg.max_velocity, True), ("a", 4, cfg.min_acceleration, False), ("a", 4, cfg.max_acceleration, True),
              ("delta", 5, cfg.delta_min, False), ("delta", 5, cfg.delta_max, True), ("jerk", 6, cfg.jerk_min, False), ("jerk", 6, cfg.jerk_max, True),
              ("rate", 7, cfg.delta_rate_min, False), ("rate", 7, cfg.delta_rate_max, True)]
    for k, (what, comp, bound, upper) in enumerate(bounds):
        bound = float(bound)
        edge, log_nb, exact = bound_edge(bound, upper, eps)
        sgn = 1.0 if upper else -1.0
        places = [("deep", None), ("edge_exact" if exact else "edge_nearest", edge), ("edge_log_neighbour", log_nb), ("g0", bound),
                  ("g_small_positive", bound + sgn * 1e-6), ("g_plus5", bound + sgn * 5.0)]
        for j, (place, val) in enumerate(places):
            x, u = _neutral(6 * k + j)
            if val is not None:
                if comp < 6:
                    x[comp] = val
                else:
                    u[comp - 6] = val
            out.append(_case("bound", f"{what}_{'max' if upper else 'min'}:{place}", x, u, _box(cfg, x, 4, k), MAIN_CMAX))
    return out


PLANE_KINDS = ("deep", "inside", "touching", "crossed", "mixed_log_first", "mixed_relaxed_first")


def _planes_of_kind(cfg, x, kind, count, k):
    D = int(cfg.num_of_disc)
    off = disc_offsets(cfg)
    eps = float(cfg.barrier_eps)
    out = []
    for i in range(count):
        j = (i + k) % D
        p = (x[0] + off[j] * math.cos(x[2]), x[1] + off[j] * math.sin(x[2]))
        phi, s = 0.7 * i + 0.3 * k, 0.5 + (i % 3)
        sub = kind
        if kind.startswith("mixed"):
            first_log = kind == "mixed_log_first"
            sub = "deep" if (i % 2 == 0) == first_log else ("inside", "crossed", "touching")[(i // 2) % 3]
        if sub == "deep":
            out.append(plane_at(cfg, p, phi, s, metres=-(4.0 + (i + k) % 5)))
        elif sub == "inside":
            out.append(plane_at(cfg, p, phi, s, g=-eps * (0.15 + 0.7 * ((i * 7 + k) % 10) / 10.0)))
        elif sub == "touching":
            out.append(plane_at(cfg, p, phi, s, metres=0.0))
        else:
            out.append(plane_at(cfg, p, phi, s, metres=0.1 + 2.9 * ((i * 3 + k) % 8) / 7.0))
    return out


def _corridor_cases(cfg):
    out = []
    k = 0
    for cmax in CMAX_GROUPS:
        counts = sorted({c for c in (0, 1, 2, 3, cmax - 1, cmax) if 0 <= c <= cmax} | (set(range(63, 71)) if cmax == 70 else set()))
        for count in counts:
            for kind in (PLANE_KINDS if count else ("none",)):
                k += 1
                x, u = _neutral(k)
                x[2] = 0.03 + 0.4 * (k % 5)
                out.append(_case("corridor", f"cmax{cmax}:count{count}:{kind}", x, u, _planes_of_kind(cfg, x, kind, count, k), cmax))
        if cmax == 70:
            # far family: the vehicle FAR metres from planes with small offsets of their own
            for count in range(63, 71):
                k += 1
                x, u = _neutral(k)
                x[0], x[1], x[2] = -FAR + 3.0 * k, 0.3 * FAR + k, 0.2 + 0.1 * (k % 4)
                sh = disc_radius(cfg) + cfg.safe_margin
                planes = []
                for i in range(count):
                    phi, s = -0.5 + 0.4 * i / count, 0.5 + (i % 3)          # normals within 0.5 rad of +x: every disc ~FAR inside
                    planes.append([s * math.cos(phi), s * math.sin(phi), (0.3 + 0.01 * i) * s + sh * s])
                out.append(_case("far", f"cmax70:count{count}:far", x, u, planes, 70))
    # a corridor plane exactly on the edge: heading 0, normal +x, the vehicle moved ulp by ulp until the rounded g is -eps
    eps = float(cfg.barrier_eps)
    off = disc_offsets(cfg)
    # (one plane offers one target value and the products a * px step by more than an ulp, so a few positions are tried)
    j = min(1, off.size - 1)
    for q in range(12):
        x, u = _neutral(3)
        x[0], x[2] = x[0] + 0.37 * q, 0.0
        raw = np.array(plane_at(cfg, (x[0] + off[j], x[1]), 0.0, 1.0, g=-eps))
        a, b, c = processed_planes(raw[None], cfg)[0]
        found = scan_exact(lambda xs: a * (xs + off[j] * 1.0) + b * (x[1] + off[j] * 0.0) - c, x[0], eps)
        if found is not None:
            x[0] = found
            out.append(_case("corridor_edge", "cmax16:count3:edge_exact", x, u, [raw] + _box(cfg, x, 2), MAIN_CMAX))
            break
    return out


HEADINGS = (0.0, math.pi / 2, -math.pi / 2, -math.pi, float(np.nextafter(math.pi, 0.0)), 3.0, 7.0, 40.0, -25.0)


def _heading_cases(cfg):
    out = []
    for k, th in enumerate(HEADINGS):
        for kind in ("mixed_log_first", "deep"):
            x, u = _neutral(k)
            x[2] = th
            x[5] = 0.05 if kind == "deep" else -0.3 + 0.07 * k
            out.append(_case("heading", f"theta={th!r}:{kind}", x, u, _planes_of_kind(cfg, x, kind, 3, k), MAIN_CMAX))
    return out


def _lane_cases(cfg, exact_ties):
    left, right = lanes()
    eps = float(cfg.barrier_eps)
    r = disc_radius(cfg)
    out = []
    spots = [("first_segment", -37.4, 0.3, 0.02), ("last_segment", 57.6, 4.9, 0.1), ("past_the_start", -52.0, -0.4, 0.0),
             ("past_the_end", 73.0, 6.5, 0.1), ("bend", 11.3, 0.1, 0.05),
             ("outside_grid_west", -150.0, 1.0, 0.3), ("outside_grid_east", 250.0, 30.0, -0.2), ("outside_grid_north", 1.7, 120.0, 1.0),
             ("outside_grid_south", 2.1, -90.0, 2.0),
             ("on_left_line", 2.4, 4.0 - r, 0.0), ("on_right_line", 2.4, -4.0 + r, 0.0),
             ("across_left_line", 2.6, 3.6, 0.01), ("centre_over_left_line", 2.2, 4.5, -0.02), ("across_right_line", 2.6, -3.7, 0.01),
             ("centre_over_right_line", 2.2, -4.6, 0.03), ("inside_left_relaxed", 2.4, 4.0 - r - 0.4 * eps, 0.0),
             ("inside_right_relaxed", 2.4, -4.0 + r + 0.4 * eps, 0.0)]
    for k, (name, px, py, th) in enumerate(spots):
        x, u = _neutral(k)
        x[0], x[1], x[2] = px, py, th
        out.append(_case("lane", name, x, u, _box(cfg, x, 4, k), MAIN_CMAX))
    # a lane plane exactly on the edge: heading 0 inside the straight part, y moved ulp by ulp (every disc has the same y)
    # (disc 0 is the one on the edge; a segment offers one target value, so the straight part is tried first, then bent segments)
    off = disc_offsets(cfg)
    for side, rows in (("left", left), ("right", right)):
        for k in (8, 12, 13, 14, 15, 16, 17):
            a, b, c = processed_lanes(rows, cfg)[k]
            x, u = _neutral(5)
            x[0], x[2] = 0.5 * (rows[k, 3] + rows[k, 5]) - 0.1, 0.0
            y0 = (c - eps - a * (x[0] + off[0])) / b
            found = scan_exact(lambda ys: a * (x[0] + off[0] * 1.0) + b * (ys + off[0] * 0.0) - c, y0, eps)
            if found is not None:
                x[1] = found
                out.append(_case("lane_edge", f"{side}_lane:edge_exact", x, u, _box(cfg, x, 4, 1), MAIN_CMAX))
                break
    if exact_ties:
        out += _tie_cases(cfg, left)
    return out


def reference_distances(seg, px, py):
    """The reference's distance of (px, py) to every segment [m, 4] and its square-free twin the fast search orders by."""
    sx, sy, ex, ey = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    ln = np.hypot(ex - sx, ey - sy)
    ux, uy = (ex - sx) / ln, (ey - sy) / ln
    x0, y0, x1, y1 = px - sx, py - sy, px - ex, py - ey
    proj = x0 * ux + y0 * uy
    cross = x0 * uy - y0 * ux
    d = np.where(proj <= 0.0, np.hypot(x0, y0), np.where(proj >= ln, np.hypot(x1, y1), np.abs(cross)))
    d2 = np.where(proj <= 0.0, x0 * x0 + y0 * y0, np.where(proj >= ln, x1 * x1 + y1 * y1, cross * cross))
    return d, d2


def _tie_cases(cfg, left):
    """Intended ties (run only under CILQR_OPT_EXACT_LANE_TIES): disc 0 just beside the normal through the bend's joint, where
    the end-point distance to the straight segment and the perpendicular distance to the bent one are the same double although
    their squares differ -- the reference keeps the earlier segment, an ordering by squares the nearer one."""
    seg = left[:, 3:7]
    off = disc_offsets(cfg)
    k = int(np.nonzero((seg[:, 2] == 10.0) & (seg[:, 3] == 4.0))[0][0])       # the bent segment that ENDS at the joint (10, 4)
    d = seg[k, 0:2] - seg[k, 2:4]
    un = d / np.hypot(*d)
    nrm = np.array([un[1], -un[0]])                                             # towards the road
    out = []
    for r in (1.5, 2.25, 2.9):
        for t in np.geomspace(3e-9, 3e-7, 600):
            p = np.array([10.0, 4.0]) + r * nrm + t * un
            x0 = p[0] - off[0]
            px, py = x0 + off[0] * 1.0, p[1] + off[0] * 0.0
            dd, d2 = reference_distances(seg, px, py)
            if np.argmin(dd) != np.argmin(d2):
                x, u = _neutral(len(out))
                x[0], x[1], x[2] = x0, p[1], 0.0
                out.append(_case("lane_tie", f"tie_at_the_bend:r={r}", x, u, _box(cfg, x, 4, 2), MAIN_CMAX, tie=True))
                break
    return out


def _fillers(cfg, n=36, seed=20260):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        x = np.array([rng.uniform(-30, 50), rng.uniform(-3, 3), rng.uniform(-3.1, 3.1), rng.uniform(0.5, 19), rng.uniform(-4, 4), rng.uniform(-0.6, 0.6)])
        u = np.array([rng.uniform(-9, 9), rng.uniform(-0.2, 0.2)])
        cnt = int(rng.integers(0, MAIN_CMAX + 1))
        kind = PLANE_KINDS[int(rng.integers(0, len(PLANE_KINDS)))]
        out.append(_case("filler", f"filler{k}", x, u, _planes_of_kind(cfg, x, kind, cnt, k), MAIN_CMAX))
    return out


def table(cfg, exact_ties=False):
    """Every case of the table under configuration cfg, as {cmax: [case, ...]}; the intended lane ties only on request."""
    cases = _bound_cases(cfg) + _corridor_cases(cfg) + _heading_cases(cfg) + _lane_cases(cfg, exact_ties) + _fillers(cfg)
    groups = {c: [] for c in CMAX_GROUPS}
    for c in cases:
        groups[c["cmax"]].append(c)
    # no two neighbours of a group with the same class where it can be helped: classes dealt round-robin, so that neighbouring
    # slots of a batch differ in plane count and in the branches their lanes take
    for cmax, g in groups.items():
        by = {}
        for c in g:
            by.setdefault((c["cls"], c["planes"].shape[0]), []).append(c)
        dealt, pools = [], list(by.values())
        while pools:
            for p in pools:
                dealt.append(p.pop(0))
            pools = [p for p in pools if p]
        groups[cmax] = dealt
    return groups


# ---------------------------------------------------------------------------------------------
# the packer
# ---------------------------------------------------------------------------------------------
def pack(cases, B, rotation=0):
    """Lay the cases into B problems of K knots.  Problem b carries case (b + rotation * n / 2) mod n at its terminal knot and
    the cases ((7 b + i) step + 3 rotation) mod n at its interior knots i, step coprime to n: with B >= n every case sits at
    a terminal knot, and at interior ones, in both rotations, and never in the same place twice.
    Returns (scene dict for the stage API, X [B, K, 6], U [B, N, 2], which [B, K] = index of the case at every knot)."""
    n = len(cases)
    assert B >= n
    step = next(s for s in range(5, 5 + 2 * n + 2, 2) if math.gcd(s, n) == 1)
    cmax = cases[0]["cmax"]
    which = np.zeros((B, K), int)
    for b in range(B):
        which[b, K - 1] = (b + rotation * (n // 2)) % n
        for i in range(K - 1):
            which[b, i] = (((K - 1) * b + i) * step + 3 * rotation) % n
    X, U = np.zeros((B, K, 6)), np.zeros((B, K - 1, 2))
    coarse, cor, cnt = np.zeros((B, K, 6)), np.zeros((B, K, cmax, 3)), np.zeros((B, K), np.int32)
    for b in range(B):
        for i in range(K):
            c = cases[which[b, i]]
            X[b, i] = c["x"]
            if i < K - 1:
                U[b, i] = c["u"]
            coarse[b, i, :3] = c["goal"]
            coarse[b, i, 3] = c["x"][3]
            m = c["planes"].shape[0]
            cor[b, i, :m] = c["planes"]
            cnt[b, i] = m
    start = np.ascontiguousarray(coarse[:, 0, :4])
    left, right = lanes()
    scene = dict(start=start, coarse=coarse, corridor=cor, ccount=cnt, left=left, right=right, n_steps=N_STEPS, cmax=cmax)
    return scene, X, U, which


def batch_size(cases, at_least=0):
    return max(len(cases), at_least)


# ---------------------------------------------------------------------------------------------
# the table evaluated on the CPU: the oracle and the long-double statement, once per (configuration, ties, rotation)
# ---------------------------------------------------------------------------------------------
_EVALUATED = {}
MAIN_BATCH = 300          # problems of the main group (cmax 16): crosses a 256-thread block and ends inside a wave


def oracle_config(name):
    from oracle import oracle as orc
    return orc.default_config(N_STEPS, **CONFIGS[name])


def evaluate(name, exact_ties=False, rotation=0):
    """{cmax: dict(scene, X, U, which, cases, oracle = dict(cost [B, 5], A, B, lx, lu, lxx, luu), stage inputs as the oracle holds
    them (goals, cor, left, right = (abc, seg)), ld = stage_reference.problems(...) on those, census)} -- computed once, shared
    by the tests, never written to."""
    key = (name, bool(exact_ties), int(rotation))
    if key in _EVALUATED:
        return _EVALUATED[key]
    import stage_reference as sr
    from oracle import oracle as orc
    ocfg = oracle_config(name)
    out = {}
    for cmax, cases in table(ocfg, exact_ties).items():
        B = batch_size(cases, MAIN_BATCH if cmax == MAIN_CMAX else 0)
        scene, X, U, which = pack(cases, B, rotation)
        o = orc.Oracle(ocfg)
        cost = np.zeros((B, 5))
        q = dict(A=np.zeros((B, N_STEPS, 6, 6)), B=np.zeros((B, N_STEPS, 6, 2)), lx=np.zeros((B, K, 6)), lu=np.zeros((B, N_STEPS, 2)),
                 lxx=np.zeros((B, K, 6, 6)), luu=np.zeros((B, N_STEPS, 2, 2)))
        goals, cor = np.zeros((B, K, 6)), np.zeros((B, K, cmax, 3))
        for b in range(B):
            assert o.set_problem(scene["start"][b], scene["coarse"][b], scene["corridor"][b], scene["ccount"][b], scene["left"], scene["right"]) == 0
            goals[b], cor[b], l_abc, r_abc, _ = o.constraints()
            cost[b] = o.total_cost(X[b], U[b])
            for k, v in o.quadratize(X[b], U[b]).items():
                q[k][b] = v
        left, right = (l_abc, scene["left"][:, 3:7]), (r_abc, scene["right"][:, 3:7])
        census = {k: 0 for k in sr.census_keys()}
        ld = sr.problems(X, U, goals, cor, scene["ccount"], left, right, ocfg, census)
        out[cmax] = dict(scene=scene, X=X, U=U, which=which, cases=cases, oracle=dict(cost=cost, **q), goals=goals, cor=cor, left=left,
                         right=right, ld=ld, census=census, cfg=ocfg)
    _EVALUATED[key] = out
    return out
