"""Inputs of the scene window tests (tests/test_scene_window.py, tests/test_gpu_scene_window.py, tests/test_gpu_plan_warm.py,
tests/test_gpu_episode.py).  A helper module: nothing here is collected.

crafted() is a table of single trajectories, each with its own t0, that puts samples on and beside every comparison of the
window rule (include/cilqr.h, "scene window").  Cases with t0 = 0 have s[k] = time[k] exactly, so a sample can be placed ON a
border (-1e-9, span + 1e-9) and one double either side of it.  Every case uses out_samples = OUT and one of two spans, so a
batched call can carry a whole group.  census() names the branches of the rule a case takes."""
import math
import struct

import numpy as np

import collision_cases as cc
from cilqr_amd import api, scene_io

OUT = 64
SPAN = 5.0
M = scene_io.WINDOW_MARGIN
SENTINEL = -777.25
BRANCHES = ("T0", "T1", "none_reaches_t0", "all_after", "lo_is_first", "lo_is_predecessor", "hi_is_last", "hi_is_successor",
            "overflow", "exact_fit", "span0", "negative_t0", "sample_at_t0", "equal_times_lower", "equal_times_upper")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def traj_of(times):
    """[T,4]: the given times with poses that name their sample (x = k + 0.5, y = -k, theta = 0.001 k)"""
    t = np.asarray(times, dtype=np.float64)
    k = np.arange(len(t), dtype=np.float64)
    return np.ascontiguousarray(np.stack([t, k + 0.5, -k, 0.001 * k], axis=1))


def _case(name, times, t0, span=SPAN, out=OUT):
    return dict(name=name, traj=traj_of(times), t0=float(t0), span=float(span), out_samples=int(out))


def crafted():
    up = SPAN + M                      # the rule's upper border, rounded as the rule rounds it
    dn, nx = (lambda v: math.nextafter(v, -math.inf)), (lambda v: math.nextafter(v, math.inf))
    grid = np.arange(0.0, 12.05, 0.1)  # 121 samples, 0 ... 12
    cases = [
        _case("no sample", [], 1.0),
        _case("one sample inside", [2.0], 1.0),
        _case("one sample before", [0.5], 1.0),
        _case("one sample after", [9.0], 1.0),
        _case("every sample before t0 - 1e-9", np.arange(0.0, 1.0, 0.1), 5.0),
        _case("every sample after t0 + span + 1e-9", np.arange(10.0, 11.0, 0.1), 1.0),
        _case("a sample exactly at t0", grid, grid[17]),
        _case("a sample at -1e-9", [-1.0, -0.5, -M, 0.5, 1.0], 0.0),
        _case("a sample one double below -1e-9", [-1.0, -0.5, dn(-M), 0.5, 1.0], 0.0),
        _case("a sample one double above -1e-9", [-1.0, -0.5, nx(-M), 0.5, 1.0], 0.0),
        _case("two samples within 1e-10 below t0", [-1.0, -0.9e-10, -0.3e-10, 0.5, 1.0], 0.0),
        _case("two samples within 1e-10 below t0 = 2.5", [1.0, 2.5 - 0.9e-10, 2.5 - 0.3e-10, 3.0, 4.0], 2.5),
        _case("a sample at span + 1e-9", [0.0, 4.0, up, 6.0, 7.0], 0.0),
        _case("a sample one double below span + 1e-9", [0.0, 4.0, dn(up), 6.0, 7.0], 0.0),
        _case("a sample one double above span + 1e-9", [0.0, 4.0, nx(up), 6.0, 7.0], 0.0),
        _case("two samples within 1e-10 above span", [0.0, 4.0, SPAN + 0.3e-10, SPAN + 0.9e-10, 6.0, 7.0], 0.0),
        _case("two samples within 1e-10 above t0 + span", [1.0, 4.0, 7.5 + 0.3e-10, 7.5 + 0.9e-10, 8.0, 9.0], 2.5),
        _case("equal times across the lower border", [-1.0, -M, -M, -M, 0.0, 0.0, 1.0], 0.0),
        _case("equal times one double below the lower border", [-1.0, dn(-M), dn(-M), dn(-M), 0.0, 1.0], 0.0),
        _case("equal times across the upper border", [0.0, 4.0, up, up, up, nx(up), nx(up), 7.0], 0.0),
        _case("equal times everywhere", [3.0] * 9, 1.0),
        _case("negative t0", np.arange(-5.0, 5.05, 0.25), -3.25),
        _case("span 0", grid, 3.05, span=0.0),
        _case("span 0 on a sample", grid, grid[30], span=0.0),
        _case("span 0, equal times at t0", [0.0, 1.0, 1.0, 1.0, 2.0], 1.0, span=0.0),
        _case("5000 samples", np.arange(5000) * 0.1, 217.33),
        _case("5000 samples, the window at the end", np.arange(5000) * 0.1, 497.0),
        _case("a window of exactly out_samples", np.arange(200) * 0.08 + 0.04, 3.01),
        _case("a window of one more: overflow", np.arange(200) * 0.08, 3.01),
    ]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def census(case):
    """the branches of the rule `case` takes: a subset of BRANCHES"""
    t, t0, span = case["traj"][:, 0], case["t0"], case["span"]
    T = len(t)
    seen = set()
    if T == 0:
        return {"T0"}
    if T == 1:
        seen.add("T1")
    s = t - t0
    lo, hi = scene_io.window_bounds(t, t0, span)
    if not (s >= -M).any():
        seen.add("none_reaches_t0")
    if (s > span + M).all():
        seen.add("all_after")
    seen.add("lo_is_first" if (s[0] >= -M) else "lo_is_predecessor")
    seen.add("hi_is_successor" if (s > span + M).any() else "hi_is_last")
    n = hi - lo + 1
    if n > case["out_samples"]:
        seen.add("overflow")
    if n == case["out_samples"]:
        seen.add("exact_fit")
    if span == 0.0:
        seen.add("span0")
    if t0 < 0.0:
        seen.add("negative_t0")
    if (s == 0.0).any():
        seen.add("sample_at_t0")
    if lo + 1 < T and s[lo] == s[lo + 1]:
        seen.add("equal_times_lower")
    if hi >= 1 and s[hi] == s[hi - 1]:
        seen.add("equal_times_upper")
    return seen


def expected(traj, t0, span, out_samples, fill=SENTINEL):
    """(rows [out_samples,4] with `fill` behind the count, count) by the NumPy statement; an overflow: all `fill`, -1"""
    rows = np.full((out_samples, 4), fill)
    w = scene_io.window_trajectory(traj, t0, span)
    if len(w) > out_samples:
        return rows, -1
    rows[:len(w)] = w
    return rows, len(w)


CENTER = cc.straight_center(length=120.0)
BODY = np.array([[1.0, 0.5], [1.0, -0.5], [-1.0, -0.5], [-1.0, 0.5]])


def scene_with(trajs, static=()):
    return scene_io.Scene(np.zeros(4), np.zeros((1, 6)), list(static),
                          [scene_io.DynamicObstacle(BODY, np.asarray(t, dtype=np.float64).reshape(-1, 4)) for t in trajs])


def host_window(trajs, t0, span, out_samples, fill=SENTINEL):
    """cilqr_window_scene on a scene of these trajectories, the output filled with `fill` first"""
    flat = scene_io.flatten_scene(CENTER, scene_with(trajs))
    out = np.full((len(trajs), out_samples, 4), fill)
    rows, counts, n = api.window_scene(flat, t0, span, out_samples, out)
    return rows, counts, n


def random_times(rng, T, start, mean_step=0.02):
    """T non-decreasing times from `start`, steps that are multiples of nothing, now and then a repeated time"""
    steps = rng.uniform(0.2, 1.8, T) * mean_step
    steps[rng.random(T) < 0.05] = 0.0
    steps[0] = 0.0
    return start + np.cumsum(steps)


def random_trajectory(rng, T, start, mean_step=0.02, x0=20.0, lane=0.0):
    """an obstacle that drives along the straight road from x0 at about 4 m/s"""
    t = random_times(rng, T, start, mean_step)
    x = x0 + 4.0 * (t - t[0]) + rng.normal(0.0, 0.01, T)
    y = lane + 0.5 * np.sin(0.3 * (t - t[0])) + rng.normal(0.0, 0.01, T)
    th = 0.15 * np.cos(0.3 * (t - t[0]))
    return np.ascontiguousarray(np.stack([t, x, y, th], axis=1))


def write_cases(path, cases, results):
    """The cases as tests/cpp/scene_window_test.cc reads them (little-endian): "SWCASE01", i32 n; per case i32 T, traj [T][4],
    f64 t0 span, i32 out_samples, i32 count, rows [out_samples][4] (SENTINEL behind the count)."""
    with open(path, "wb") as o:
        o.write(b"SWCASE01" + struct.pack("<i", len(cases)))
        for c, (rows, count) in zip(cases, results):
            o.write(struct.pack("<i", len(c["traj"])) + np.ascontiguousarray(c["traj"], dtype="<f8").tobytes())
            o.write(struct.pack("<ddii", c["t0"], c["span"], c["out_samples"], int(count)))
            o.write(np.ascontiguousarray(rows, dtype="<f8").tobytes())


# ---------------------------------------------------------------------------------------------------------------------
# batches (the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
def empty_batch(B, D, S, center=None):
    """a packed batch (scene_io.pack_scene_batch's dict) of B scenes with D dynamic slots of S samples, no static obstacle,
    every slot with the body polygon and no sample yet"""
    center = CENTER if center is None else center
    out = dict(batch=B, center=np.ascontiguousarray(center), max_static=1, max_dynamic=D, max_vertices=4, max_samples=S,
               static_points=np.zeros((B, 1, 4, 2)), static_counts=np.zeros((B, 1), dtype=np.int32),
               dynamic_polygon_points=np.tile(BODY, (B, D, 1, 1)),
               dynamic_polygon_counts=np.full((B, D), 4, dtype=np.int32),
               dynamic_trajectories=np.zeros((B, D, S, 4)), dynamic_trajectory_counts=np.zeros((B, D), dtype=np.int32))
    return out


def random_batch(rng, B, D, S, span=SPAN):
    """(packed, t0 [B]): trajectories of 0 ... S samples (slot 0 of scene 0: S), steps between 5 ms and 0.5 s, a t0 per scene
    that lies before, inside or behind the recordings"""
    p = empty_batch(B, D, S)
    t0 = np.zeros(B)
    for b in range(B):
        ends = []
        for d in range(D):
            T = S if (b, d) == (0, 0) else int(rng.integers(0, S + 1))
            if T:
                tr = random_trajectory(rng, T, rng.uniform(-2.0, 6.0), float(rng.choice([0.005, 0.02, 0.1, 0.5])))
                p["dynamic_trajectories"][b, d, :T] = tr
                ends.append(tr[-1, 0])
            p["dynamic_trajectory_counts"][b, d] = T
        t0[b] = rng.uniform(-4.0, max(ends, default=1.0) + 1.0)
    return p, t0


def host_batch(packed, t0, span, out_samples, fill):
    """cilqr_window_scene for every scene of a packed batch: (rows [B,D,out,4] with `fill` behind the counts, counts [B,D],
    ok [B] int32)"""
    B, D = packed["batch"], packed["max_dynamic"]
    rows, counts = np.full((B, D, out_samples, 4), fill), np.zeros((B, D), dtype=np.int32)
    template = scene_io.flatten_scene(CENTER, scene_with([np.zeros((0, 4))] * D))
    for b in range(B):
        n = packed["dynamic_trajectory_counts"][b]
        flat = dict(template, dynamic_trajectory_counts=np.ascontiguousarray(n),
                    dynamic_trajectories=np.ascontiguousarray(np.concatenate([packed["dynamic_trajectories"][b, d, :n[d]] for d in range(D)])))
        rows[b], counts[b], _ = api.window_scene(flat, float(t0[b]), span, out_samples, np.ascontiguousarray(rows[b]))
    return rows, counts, (counts >= 0).all(axis=1).astype(np.int32)


def host_arrays_window(opt, packed, t0, span, out_samples, fill):
    """cilqr_window_scenes_batch on HOST arrays: (rows, counts, ok, rc, n_overflow)"""
    B, D = packed["batch"], packed["max_dynamic"]
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_HOST, **{k: keep[k].ctypes.data for k in keep})
    rows, counts, ok = np.full((B, D, out_samples, 4), fill), np.full((B, D), -9, np.int32), np.full(B, -9, np.int32)
    t0 = np.ascontiguousarray(t0, dtype=np.float64)
    rc, n = opt.window_scenes_raw(sb, t0.ctypes.data, span, out_samples, rows.ctypes.data, counts.ctypes.data, ok.ctypes.data)
    return rows, counts, ok, rc, n


def device_arrays_window(opt, packed, t0, span, out_samples, fill, odd=False):
    """the same on DEVICE arrays; odd: the source and the output start on an odd double (8 bytes past a 16-byte boundary)"""
    import torch
    dev = torch.device("cuda", 0)
    B, D = packed["batch"], packed["max_dynamic"]

    def f64(a):    # a device copy that starts on a 16-byte boundary, or 8 bytes behind one
        a = np.ascontiguousarray(a, dtype=np.float64)
        buf = torch.empty(a.size + 2, dtype=torch.float64, device=dev)
        first = (buf.data_ptr() // 8 + (1 if odd else 0)) % 2     # 0 / 1 doubles to skip so that the parity is the wanted one
        view = buf[first:first + a.size]
        view.copy_(torch.from_numpy(a.ravel()))
        assert (view.data_ptr() % 16 == 8) == odd
        return view
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    src = f64(packed["dynamic_trajectories"])
    ptrs = {k: t[k].data_ptr() for k in t}
    ptrs["dynamic_trajectories"] = src.data_ptr()
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **ptrs)
    rows = f64(np.full((B, D, out_samples, 4), fill))
    counts = torch.full((B, D), -9, dtype=torch.int32, device=dev)
    ok = torch.full((B,), -9, dtype=torch.int32, device=dev)
    t0_d = torch.from_numpy(np.ascontiguousarray(t0, dtype=np.float64)).to(dev)
    torch.cuda.synchronize()
    rc, n = opt.window_scenes_raw(sb, t0_d.data_ptr(), span, out_samples, rows.data_ptr(), counts.data_ptr(), ok.data_ptr())
    torch.cuda.synchronize()
    return rows.cpu().numpy().reshape(B, D, out_samples, 4), counts.cpu().numpy(), ok.cpu().numpy(), rc, n


def recording(traj, seconds=15.0, dt=0.01):
    """a recording of `seconds` at `dt` (1501 samples for 15 s at 10 ms) of an obstacle that keeps the mean velocity and the
    first heading of traj [T,4]"""
    traj = np.asarray(traj, dtype=np.float64).reshape(-1, 4)
    t = np.arange(int(round(seconds / dt)) + 1) * dt
    span = max(traj[-1, 0] - traj[0, 0], dt)
    v = (traj[-1, 1:3] - traj[0, 1:3]) / span
    return np.ascontiguousarray(np.stack([t, traj[0, 1] + v[0] * t, traj[0, 2] + v[1] * t, np.full_like(t, traj[0, 3])], axis=1))
