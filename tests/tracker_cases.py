"""Crafted coarse trajectories with start states for the tracker init guess (kernels_tracker.hip, CILQR_INIT_TRACKER), shared by
tests/test_tracker.py (the CPU oracle against tests/tracker_reference.py) and tests/test_gpu_tracker.py (the kernel against
the oracle).  A helper module: nothing here is collected.

A case is a dict: name, n_steps, knot_dt, start [4] = x y theta v, coarse [K,6] = x y theta v a delta, station [K] (the arc
length the path was drawn with: it differs from the chord length on every arc), tracker = overrides of cilqr_tracker_config,
vehicle = overrides of the cilqr_config fields the tracker reads (wheel_base and the five pairs of bounds).  cases() is the
table, groups() the same cases keyed by what one handle can run (n_steps, knot_dt, tracker, vehicle).

Paths are drawn knot by knot from a speed and a curvature per knot (unicycle, explicit Euler: exactness does not matter, the
tracker only follows them); headings are wrapped into [-pi, pi) like the DP planner's, so a path that turns through +-pi jumps
by 2 pi in its heading column.
"""
import math

import numpy as np

# the reference's TrackerConfig / VehicleParam defaults live in oracle.TRACKER_CFG_DEFAULT; only overrides are named here
TRACKER_FIELDS = ("weight_l", "weight_theta", "weight_delta", "weight_delta_rate", "preview_time", "weight_s", "weight_v",
                  "weight_a", "weight_j", "sumulation_dt", "dt", "tolerance", "max_num_iteration")
VEHICLE_FIELDS = ("wheel_base", "delta_min", "delta_max", "delta_rate_min", "delta_rate_max", "jerk_min", "jerk_max",
                  "min_acceleration", "max_acceleration")


def _wrap(a):
    return (a + math.pi) % (2.0 * math.pi) - math.pi


def path(n_steps, knot_dt, v, kappa=0.0, x0=0.0, y0=0.0, th0=0.0, wrap=True):
    """coarse [K,6] and station [K] of a path with speed v[k] and curvature kappa[k] (scalars broadcast)."""
    K = n_steps + 1
    v = np.broadcast_to(np.asarray(v, float), (K,)).copy()
    kappa = np.broadcast_to(np.asarray(kappa, float), (K,))
    c = np.zeros((K, 6))
    s = np.zeros(K)
    x, y, th = x0, y0, th0
    for k in range(K):
        c[k, :4] = x, y, (_wrap(th) if wrap else th), v[k]
        if k + 1 < K:
            s[k + 1] = s[k] + v[k] * knot_dt
            x += v[k] * math.cos(th) * knot_dt
            y += v[k] * math.sin(th) * knot_dt
            th += v[k] * kappa[k] * knot_dt
    return c, s


def _case(name, n_steps, knot_dt, coarse_station, start=None, tracker=None, vehicle=None):
    coarse, station = coarse_station
    start = coarse[0, :4].copy() if start is None else np.asarray(start, float)
    return dict(name=name, n_steps=n_steps, knot_dt=knot_dt, start=start, coarse=coarse, station=station,
                tracker=dict(tracker or {}), vehicle=dict(vehicle or {}))


def _offset(coarse, lateral=0.0, dtheta=0.0, v=None):
    """start state: knot 0 moved `lateral` to its left, turned by dtheta, with speed v"""
    x, y, th, v0 = coarse[0, :4]
    return [x - math.sin(th) * lateral, y + math.cos(th) * lateral, th + dtheta, v0 if v is None else v]


def cases():
    out = []
    N, dt = 50, 0.1

    def add(name, cs, n=N, d=dt, **kw):
        out.append(_case(name, n, d, cs, **kw))

    # ---- the default configuration, N = 50, dt = 0.1 ----
    add("straight", path(N, dt, 8.0))
    add("arc_left", path(N, dt, 8.0, 0.05, th0=0.3))
    add("arc_right", path(N, dt, 6.0, -0.08, x0=5.0, y0=-3.0, th0=-1.0))
    add("through_pi", path(N, dt, 7.0, 0.06, th0=math.pi - 0.9))             # the heading column jumps from +pi to -pi
    add("through_minus_pi", path(N, dt, 7.0, -0.06, th0=-math.pi + 0.9))
    # every heading of the path is the double nearest pi.  (The vehicle starts beside it: one that starts ON it with the same
    # heading keeps a heading error of exactly 0, and whether its heading reads +pi or -pi after a step is decided by the last
    # bit of the steering noise -- in the kernel, in the oracle and in long double alike.)
    add("exactly_pi", path(N, dt, 5.0, 0.0, x0=40.0, th0=math.pi, wrap=False), start=[40.0, -0.3, math.pi, 5.0])
    add("exactly_pi_offset", path(N, dt, 5.0, 0.0, x0=40.0, th0=math.pi, wrap=False),
        start=[40.0, 0.4, math.pi - 0.2, 5.0])
    add("stopped", path(N, dt, 0.0, x0=3.0, y0=1.0, th0=0.4))                 # one point, K times: every station equal
    add("stopped_moving_start", path(N, dt, 0.0, x0=3.0, y0=1.0, th0=0.4), start=[3.0, 1.0, 0.4, 3.0])
    v_half = np.concatenate([np.linspace(6.0, 0.0, 26), np.zeros(25)])
    add("stops_halfway", path(N, dt, v_half, 0.02))
    add("slow_1mps", path(N, dt, 1.0, 0.05))
    add("offset_start", path(N, dt, 8.0, 0.01), start=_offset(path(N, dt, 8.0, 0.01)[0], 2.0, 0.5))
    add("offset_start_right", path(N, dt, 8.0, -0.01), start=_offset(path(N, dt, 8.0, -0.01)[0], -2.0, -0.5))
    add("start_far_faster", path(N, dt, 1.0), start=[0.0, 0.0, 0.0, 15.0])
    add("standing_start", path(N, dt, 10.0), start=[0.0, 0.0, 0.0, 0.0])
    add("curvature_0p3", path(N, dt, 5.0, 0.3))
    add("curvature_0p3_right", path(N, dt, 5.0, -0.3, th0=2.0))
    add("start_beyond_the_end", path(N, dt, 2.0), start=[14.0, 0.5, 0.1, 4.0])   # nearest knot: the last one, all the way
    add("start_before_the_path", path(N, dt, 6.0, x0=10.0), start=[2.0, 0.3, 0.0, 6.0])   # nearest knot: the first one
    # ---- horizons ----
    for n in (1, 2, 3, 5, 100, 280):
        add(f"N{n}_straight", path(n, dt, 6.0), n=n, start=[0.0, 0.5, 0.1, 5.0])
        add(f"N{n}_arc", path(n, dt, 4.0 if n > 100 else 7.0, 0.03 if n > 100 else 0.06, th0=2.6), n=n)
    add("N280_stops", path(280, dt, np.concatenate([np.linspace(8.0, 0.0, 141), np.zeros(140)]), -0.01), n=280)
    # ---- knot spacing ----
    for d in (0.05, 0.08, 0.2):
        add(f"dt{d}_arc", path(N, d, 7.0, 0.05, th0=-0.5), d=d)
        add(f"dt{d}_offset", path(N, d, 5.0, -0.02), d=d, start=_offset(path(N, d, 5.0, -0.02)[0], 1.0, -0.3, v=7.0))
    # ---- the simulation step ----
    for sd in (0.005, 0.02, 0.025, 0.05, 0.1):
        add(f"sim{sd}_arc", path(N, dt, 7.0, 0.05), tracker=dict(sumulation_dt=sd))
        add(f"sim{sd}_offset", path(N, dt, 3.0, -0.1, th0=3.0), tracker=dict(sumulation_dt=sd),
            start=_offset(path(N, dt, 3.0, -0.1, th0=3.0)[0], -1.0, 0.3, v=1.0))
    # ---- the DARE loop's stopping rule ----
    for tol, cap, n in ((1e-8, 150, 50), (0.0, 7, 50), (0.01, 1, 50), (0.0, 150, 5), (0.01, 7, 50)):
        tr = dict(tolerance=tol, max_num_iteration=cap)
        # (not along the x axis: with a cap of 1 the gains are ~1e-12 and the vehicle drives straight on)
        add(f"tol{tol}_cap{cap}_arc", path(n, dt, 7.0, 0.05, x0=2.0, y0=1.0, th0=0.4), n=n, tracker=tr)
        add(f"tol{tol}_cap{cap}_slow_offset", path(n, dt, 1.5, 0.1), n=n, tracker=tr,
            start=_offset(path(n, dt, 1.5, 0.1)[0], 0.5, 0.2, v=2.5))
    # ---- non-default weights, controller dt and preview time ----
    tr = dict(weight_l=0.7, weight_theta=0.3, weight_delta=0.05, weight_delta_rate=0.4, preview_time=0.5, weight_s=0.2,
              weight_v=0.6, weight_a=0.03, weight_j=0.25, dt=0.05)
    add("weights_arc", path(N, dt, 7.0, 0.05), tracker=tr)
    add("weights_offset", path(N, dt, 8.0, -0.02), tracker=tr, start=_offset(path(N, dt, 8.0, -0.02)[0], 2.0, 0.5, v=4.0))
    add("weights_slow", path(N, dt, 1.0, 0.2), tracker=tr)
    # ---- another vehicle ----
    veh = dict(wheel_base=2.8, delta_min=-0.5, delta_max=0.45, delta_rate_min=-0.3, delta_rate_max=0.25, jerk_min=-6.0,
               jerk_max=4.0, min_acceleration=-3.0, max_acceleration=2.0)
    add("vehicle_arc", path(N, dt, 7.0, 0.05), vehicle=veh)
    add("vehicle_tight", path(N, dt, 5.0, 0.3), vehicle=veh)
    add("vehicle_offset", path(N, dt, 8.0, -0.02), vehicle=veh, start=_offset(path(N, dt, 8.0, -0.02)[0], -2.0, -0.5, v=14.0))
    add("vehicle_standing", path(N, dt, 10.0), vehicle=veh, start=[0.0, 0.0, 0.0, 0.0])
    add("vehicle_far_faster", path(N, dt, 1.0), vehicle=veh, start=[0.0, 0.0, 0.0, 12.0])
    return out


def group_key(case):
    return (case["n_steps"], case["knot_dt"], tuple(sorted(case["tracker"].items())), tuple(sorted(case["vehicle"].items())))


def groups():
    """[(key, [cases])]: the cases one handle can run together, in table order"""
    out = {}
    for c in cases():
        out.setdefault(group_key(c), []).append(c)
    return list(out.items())


def oracle_overrides(case):
    """keyword overrides of oracle.tracker_init_guess for a case"""
    return dict(case["tracker"], **case["vehicle"])


def box_corridors(coarse, cmax=16, half=10.0):
    """A plain box of `half` metres around every knot, [B,K,cmax,3] and counts [B,K]: the corridor a load needs (the init guess
    does not read it)."""
    B, K = coarse.shape[:2]
    th = coarse[:, :, 2]
    n = np.stack([np.stack([np.cos(th), np.sin(th)], -1), np.stack([-np.cos(th), -np.sin(th)], -1),
                  np.stack([-np.sin(th), np.cos(th)], -1), np.stack([np.sin(th), -np.cos(th)], -1)], 2)   # [B,K,4,2]
    cor = np.zeros((B, K, cmax, 3))
    cor[:, :, :4, :2] = n
    cor[:, :, :4, 2] = (n * coarse[:, :, None, :2]).sum(-1) + half
    return cor, np.full((B, K), 4, np.int32)
