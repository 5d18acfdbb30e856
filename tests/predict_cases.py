"""Inputs of the scene prediction tests (tests/test_predict.py, tests/test_gpu_predict.py, tests/test_gpu_episode_predict.py).
A helper module: nothing here is collected.

crafted() is a table of single trajectories, each with its own t0, mode and max_age, that puts samples on and beside every
comparison of the prediction rule (include/cilqr.h, "scene prediction").  Cases with t0 = 0 have s[k] = time[k] exactly, so a
sample can be placed ON a border (1e-9, max_age, the 1e-10 of the velocity) and one double past it.  Every case uses
SAMPLE_DT, OUT and SPAN, so a batched call can carry a whole group (groups(): the cases that share t0, mode and max_age).
census() names the branches of the rule a case takes."""
import math
import struct

import numpy as np

import scene_window_cases as sw
from cilqr_amd import api, scene_io

SPAN = 5.0
SAMPLE_DT = 0.1
OUT = 52                # 51 * 0.1 = 5.1000000000000005 >= 5 + 1e-9; 50 * 0.1 = 5.0 is not
M = scene_io.PREDICT_MARGIN
H = scene_io.PREDICT_MIN_STEP
HOLD, CV = api.PREDICT_HOLD, api.PREDICT_CONSTANT_VELOCITY
SENTINEL = -777.25
BRANCHES = ("T0", "T1", "unseen", "too_old", "age_at_limit", "negative_age", "sample_at_t0", "hold", "cv_first_sighting",
            "cv_step_too_small", "cv_step_at_limit", "cv_equal_times", "cv_moving", "nonfinite", "negative_t0", "long")
CENTER, BODY = sw.CENTER, sw.BODY
scene_with, empty_batch = sw.scene_with, sw.empty_batch


def same_bits(a, b):
    """the same shape, type and bits -- except that any NaN equals any NaN: which NaN an operation returns (sign, payload) is
    the processor's choice, not the rule's, and an x86 host and the GPU choose differently.  On finite values and infinities
    this is the comparison of the bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return a.tobytes() == b.tobytes()
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | both_nan).all())


def traj_of(times):
    """[T,4]: the given times with poses that name their sample (x = 0.75 k + 0.5, y = -0.3 k, theta = 0.1 + 0.001 k)"""
    t = np.asarray(times, dtype=np.float64)
    k = np.arange(len(t), dtype=np.float64)
    return np.ascontiguousarray(np.stack([t, 0.75 * k + 0.5, -0.3 * k, 0.1 + 0.001 * k], axis=1))


def _case(name, times, t0=0.0, mode=CV, max_age=1.0, poses=None):
    traj = traj_of(times)
    if poses is not None:
        traj[:, 1:] = np.asarray(poses, dtype=np.float64).reshape(len(traj), 3)
    return dict(name=name, traj=traj, t0=float(t0), mode=int(mode), max_age=float(max_age))


def crafted():
    dn, nx = (lambda v: math.nextafter(v, -math.inf)), (lambda v: math.nextafter(v, math.inf))
    inf, nan = math.inf, math.nan
    grid = np.arange(0.0, 12.05, 0.1)
    long = np.arange(5000) * 0.1 - 217.33
    cases = [
        _case("no sample", []),
        _case("one sample before t0", [-0.5]),
        _case("one sample at t0", [0.0]),
        _case("one sample after t0", [0.5]),
        _case("one sample at 1e-9: observed", [M]),
        _case("one sample one double above 1e-9: unseen", [nx(M)]),
        _case("the latest at 1e-9", [-1.0, -0.5, M]),
        _case("the latest one double above 1e-9 is not observed", [-1.0, -0.5, nx(M)]),
        _case("a sample at 1e-9 among later ones", [-0.75, -0.5, M, 0.5, 1.0]),
        _case("age exactly max_age", [-2.0, -1.0, 3.0]),
        _case("age one double above max_age", [-2.0, dn(-1.0), 3.0]),
        _case("age exactly max_age = 0", [-1.0, 0.0, 3.0], max_age=0.0),
        _case("age one double above max_age = 0", [-1.0, -5e-324], max_age=0.0),
        _case("the recording ended before t0", np.arange(-9.0, -2.0, 0.1)),
        _case("step exactly 1e-10", [-1.0, -H, 0.0, 2.0]),
        _case("step one double above 1e-10", [-1.0, -nx(H), 0.0, 2.0]),
        _case("two samples at one time", [-1.0, -0.5, -0.5, 2.0]),
        _case("three samples at t0", [-1.0, 0.0, 0.0, 0.0, 2.0]),
        _case("first sighting in CV mode", [-0.5, 0.5, 1.0]),
        _case("first sighting in HOLD mode", [-0.5, 0.5, 1.0], mode=HOLD),
        _case("moving, held", [-1.0, -0.5, -0.25, 2.0], mode=HOLD),
        _case("moving", [-1.0, -0.5, -0.25, 2.0]),
        _case("moving, every sample observed", [-1.0, -0.5, -0.25]),
        _case("a sample exactly at t0 = 1.7", grid, t0=grid[17]),
        _case("t0 between samples", grid, t0=3.14159),
        _case("negative t0", np.arange(-5.0, 5.05, 0.25), t0=-3.3),
        _case("negative t0, held", np.arange(-5.0, 5.05, 0.25), t0=-3.3, mode=HOLD),
        _case("5000 samples", long),
        _case("5000 samples, held", long, mode=HOLD),
        _case("5000 samples, the latest is the last", long - 282.6),
        _case("NaN x at the latest", [-1.0, -0.5, 1.0], poses=[[1.0, 2.0, 0.1], [nan, 2.5, 0.2], [3.0, 3.0, 0.3]]),
        _case("NaN y before the latest, held", [-1.0, -0.5, 1.0], mode=HOLD, poses=[[1.0, nan, 0.1], [2.0, 2.5, 0.2], [3.0, 3.0, 0.3]]),
        _case("inf x before the latest", [-1.0, -0.5, 1.0], poses=[[inf, 2.0, 0.1], [2.0, 2.5, 0.2], [3.0, 3.0, 0.3]]),
        _case("inf y twice", [-1.0, -0.5, 1.0], poses=[[1.0, inf, 0.1], [2.0, inf, 0.2], [3.0, 3.0, 0.3]]),
        _case("NaN heading", [-1.0, -0.5, 1.0], poses=[[1.0, 2.0, 0.1], [2.0, 2.5, nan], [3.0, 3.0, 0.3]]),
        _case("the sample before at -inf", [-inf, -0.5, 1.0]),
        _case("the latest at -inf", [-inf, 0.5, 1.0]),
        _case("a later sample at +inf", [-1.0, -0.5, inf]),
    ]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def groups(cases):
    """{(t0, mode, max_age): [index of a case]}: the cases one scene of one call can carry"""
    out = {}
    for i, c in enumerate(cases):
        out.setdefault((c["t0"], c["mode"], c["max_age"]), []).append(i)
    return out


def census(case):
    """the branches of the rule `case` takes: a subset of BRANCHES"""
    tr, t0, mode, max_age = case["traj"], case["t0"], case["mode"], case["max_age"]
    T = len(tr)
    seen = set()
    if T == 0:
        return {"T0"}
    if T == 1:
        seen.add("T1")
    if T >= 5000:
        seen.add("long")
    if t0 < 0.0:
        seen.add("negative_t0")
    if not np.isfinite(tr).all():
        seen.add("nonfinite")
    s = tr[:, 0] - t0
    J = scene_io._first_true(T, lambda k: bool(M < s[k]))
    if J == 0:
        return seen | {"unseen"}
    j = J - 1
    e = -s[j]
    if e > max_age:
        return seen | {"too_old"}
    if e == max_age:
        seen.add("age_at_limit")
    if e < 0.0:
        seen.add("negative_age")
    if e == 0.0:
        seen.add("sample_at_t0")
    if mode == HOLD:
        return seen | {"hold"}
    if j == 0:
        return seen | {"cv_first_sighting"}
    h = tr[j, 0] - tr[j - 1, 0]
    if h == 0.0:
        seen.add("cv_equal_times")
    if h == H:
        seen.add("cv_step_at_limit")
    seen.add("cv_moving" if h > H else "cv_step_too_small")
    return seen


def expected(case, fill=SENTINEL, sample_dt=SAMPLE_DT, out_samples=OUT):
    """(rows [out_samples,4], count) by the NumPy statement; count 0: all `fill`"""
    rows = np.full((out_samples, 4), fill)
    p = scene_io.predict_trajectory(case["traj"], case["t0"], case["mode"], case["max_age"], sample_dt, out_samples)
    rows[:len(p)] = p
    return rows, len(p)


def host_predict(trajs, t0, mode, max_age, span=SPAN, sample_dt=SAMPLE_DT, out_samples=OUT, fill=SENTINEL, counts=None):
    """cilqr_predict_scene on a scene of these trajectories, the output filled with `fill` first; counts: the source counts
    to declare instead of the trajectories' own (a negative one takes no samples)"""
    flat = scene_io.flatten_scene(CENTER, scene_with(trajs))
    if counts is not None:
        flat = dict(flat, dynamic_trajectory_counts=np.asarray(counts, dtype=np.int32))
    out = np.full((len(trajs), out_samples, 4), fill)
    return api.predict_scene(flat, t0, span, mode, max_age, sample_dt, out_samples, out)


def write_cases(path, cases, results, sample_dt=SAMPLE_DT, out_samples=OUT):
    """The cases as tests/cpp/scene_predict_test.cc reads them (little-endian): "SPCASE01", i32 n; per case i32 T, traj [T][4],
    f64 t0 max_age sample_dt, i32 mode out_samples count, rows [out_samples][4] (SENTINEL where nothing is written)."""
    with open(path, "wb") as o:
        o.write(b"SPCASE01" + struct.pack("<i", len(cases)))
        for c, (rows, count) in zip(cases, results):
            o.write(struct.pack("<i", len(c["traj"])) + np.ascontiguousarray(c["traj"], dtype="<f8").tobytes())
            o.write(struct.pack("<dddiii", c["t0"], c["max_age"], sample_dt, c["mode"], out_samples, int(count)))
            o.write(np.ascontiguousarray(rows, dtype="<f8").tobytes())


def dyadic_recording(T=200, step=0.125, v=(1.5, -0.25), start=(12.0, 1.0), theta=0.375):
    """[T,4]: constant velocity with dyadic times, positions and velocity, so that every product and sum of the rule is exact"""
    t = np.arange(T) * step
    return np.ascontiguousarray(np.stack([t, start[0] + v[0] * t, start[1] + v[1] * t, np.full(T, theta)], axis=1))


# ---------------------------------------------------------------------------------------------------------------------
# batches (the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
def random_batch(rng, B, D, S):
    """(packed, t0 [B]): trajectories of 0 ... S samples (slot 0 of scene 0: S, the last slot of the last scene: 0), steps
    between 5 ms and 0.5 s and now and then a repeated time, a t0 per scene that lies before, inside or behind the recordings"""
    p = empty_batch(B, D, S)
    t0 = np.zeros(B)
    for b in range(B):
        ends = []
        for d in range(D):
            T = S if (b, d) == (0, 0) else 0 if (b, d) == (B - 1, D - 1) and B * D > 1 else int(rng.integers(0, S + 1))
            if T:
                tr = sw.random_trajectory(rng, T, rng.uniform(-2.0, 6.0), float(rng.choice([0.005, 0.02, 0.1, 0.5])))
                p["dynamic_trajectories"][b, d, :T] = tr
                ends.append(tr[-1, 0])
            p["dynamic_trajectory_counts"][b, d] = T
        t0[b] = rng.uniform(-3.0, max(ends, default=1.0) + 1.5)
    t0[0] = p["dynamic_trajectories"][0, 0, S // 2, 0] + 0.001      # the full slot is observed and young
    return p, t0


def host_batch(packed, t0, mode, max_age, span, sample_dt, out_samples, fill):
    """cilqr_predict_scene for every scene of a packed batch: (rows [B,D,out,4] with `fill` where nothing is written, counts
    [B,D], ok [B] int32)"""
    B, D = packed["batch"], packed["max_dynamic"]
    rows, counts = np.full((B, D, out_samples, 4), fill), np.zeros((B, D), dtype=np.int32)
    for b in range(B):
        n = packed["dynamic_trajectory_counts"][b]
        trajs = [packed["dynamic_trajectories"][b, d, :n[d]] for d in range(D)]
        rows[b], counts[b], _ = host_predict(trajs, float(t0[b]), mode, max_age, span, sample_dt, out_samples, fill)
    return rows, counts, (counts >= 0).all(axis=1).astype(np.int32)


def host_arrays_predict(opt, packed, t0, mode, max_age, span, sample_dt, out_samples, fill):
    """cilqr_predict_scenes_batch on HOST arrays: (rows, counts, ok, rc, n_refused)"""
    B, D = packed["batch"], packed["max_dynamic"]
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_HOST, **{k: keep[k].ctypes.data for k in keep})
    rows, counts, ok = np.full((B, D, out_samples, 4), fill), np.full((B, D), -9, np.int32), np.full(B, -9, np.int32)
    t0 = np.ascontiguousarray(t0, dtype=np.float64)
    rc, n = opt.predict_scenes_raw(sb, t0.ctypes.data, span, mode, max_age, sample_dt, out_samples, rows.ctypes.data,
                                   counts.ctypes.data, ok.ctypes.data)
    return rows, counts, ok, rc, n


def device_arrays_predict(opt, packed, t0, mode, max_age, span, sample_dt, out_samples, fill, odd=False):
    """the same on DEVICE arrays; odd: the source and the output start on an odd double (8 bytes past a 16-byte boundary)"""
    import torch
    dev = torch.device("cuda", 0)
    B, D = packed["batch"], packed["max_dynamic"]

    def f64(a):    # a device copy that starts on a 16-byte boundary, or 8 bytes behind one
        a = np.ascontiguousarray(a, dtype=np.float64)
        buf = torch.empty(a.size + 2, dtype=torch.float64, device=dev)
        first = (buf.data_ptr() // 8 + (1 if odd else 0)) % 2
        view = buf[first:first + a.size]
        view.copy_(torch.from_numpy(a.ravel()))
        assert (view.data_ptr() % 16 == 8) == odd
        return view
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS if k != "dynamic_trajectories"}
    src = f64(packed["dynamic_trajectories"])
    ptrs = {k: t[k].data_ptr() for k in t}
    ptrs["dynamic_trajectories"] = src.data_ptr()
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **ptrs)
    rows = f64(np.full((B, D, out_samples, 4), fill))
    counts = torch.full((B, D), -9, dtype=torch.int32, device=dev)
    ok = torch.full((B,), -9, dtype=torch.int32, device=dev)
    t0_d = torch.from_numpy(np.ascontiguousarray(t0, dtype=np.float64)).to(dev)
    torch.cuda.synchronize()
    rc, n = opt.predict_scenes_raw(sb, t0_d.data_ptr(), span, mode, max_age, sample_dt, out_samples, rows.data_ptr(),
                                   counts.data_ptr(), ok.data_ptr())
    torch.cuda.synchronize()
    return rows.cpu().numpy().reshape(B, D, out_samples, 4), counts.cpu().numpy(), ok.cpu().numpy(), rc, n
