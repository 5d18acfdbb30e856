#!/usr/bin/env python3
"""cilqr_window_scenes_batch (kernels_scene_window.hip) at bench scale: 65536 scenes of 9 dynamic obstacles with 1501
source samples each, resident in HBM, every scene at its own t0, windows of span 5 s.

    python tools/scene_window_bench.py
    python tools/scene_window_bench.py --scenes 4096 --cycle-scenes 256 --out /tmp/x.json

Two recordings of 1501 samples are measured: `rate_10ms` is the 15 s recording at 10 ms (a 5 s window
is 503 samples, so out_samples = 512: into 64 every obstacle would overflow), `rate_100ms` the same 1501 samples at 100 ms
(a window is 53 samples, out_samples = 64).

Before the kernel runs the tool writes down an ESTIMATE from the shapes alone: the window's bytes read plus written (and the
counts, t0) at the 4.41 TB/s profiles/r11_resample.json records for a streaming kernel, plus the searches' rounds of
dependent loads -- per wave one load of the counts / t0 and, per search, ceil(log64(T)) probes, each an HBM miss of about 900
cycles at 2.4 GHz (the idle-chip figure), with the waves of the batch going through the chip in groups of as many as are
resident (256 CUs x 8 waves).  Then the MEASUREMENT: HIP events on the handle's stream around --calls back-to-back calls, a
warm-up first, median of --samples with min and max, per call (every call ends in the library's wait for its stream: it is the
call's time, not the bare kernel's).  Beside both, a device-to-device hipMemcpyAsync of the OUTPUT's byte count timed the
same way.  A sample of the windows is compared with the host call.

Then one planning cycle (window -> plan, warm -> track) on --cycle-scenes generated scenes with 1501-sample recordings, wall
clock, two ways: with the window cut on the device from the resident recordings (t0 and the start states are all that is
uploaded), and with the host shifting the time column of its own copy of the windows and uploading them again (the cutting
itself, which the host would also have to do, is not charged).  Nobody had measured any of this before; the numbers are what
they are, no threshold is set on them.  One JSON line is printed and written to --out (default
profiles/r16_scene_window.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

from cilqr_amd import api, scenario, scene_io  # noqa: E402

STREAM_BYTES_PER_S = 4.41e12      # profiles/r11_resample.json, shared_axis_5x
MISS_S = 900 / 2.4e9              # one dependent HBM miss, idle chip
RESIDENT_WAVES = 256 * 8


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), samples=len(a))


def _timed(fn, samples, calls):
    torch.cuda.synchronize()      # the library runs on the handle's stream: what torch queued before must be done
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return _spread(ms)


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def resident_batch(n, D, S, dt, seed, dev):
    """(trajectories [n,D,S,4], counts [n,D], t0 [n]) made on the device: recordings that start within a second of 0 at the
    rate 1 / dt, every scene somewhere in the first two thirds of its recording"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    traj = torch.empty((n, D, S, 4), dtype=torch.float64, device=dev)
    k = torch.arange(S, dtype=torch.float64, device=dev)
    step = max(1, 2048 * 9 * 1501 // (D * S))
    for b in range(0, n, step):
        m = min(step, n - b)
        off = torch.rand((m, D, 1), generator=g, dtype=torch.float64, device=dev)
        traj[b:b + m, :, :, 0] = off + k * dt
        traj[b:b + m, :, :, 1] = 20.0 + 4.0 * k * dt + off
        traj[b:b + m, :, :, 2] = off - 0.5
        traj[b:b + m, :, :, 3] = 0.1 * off
    counts = torch.full((n, D), S, dtype=torch.int32, device=dev)
    t0 = torch.rand((n,), generator=g, dtype=torch.float64, device=dev) * (S * dt * 2.0 / 3.0 - 5.0)
    return traj, counts, t0


def estimate(n, D, S, window):
    moved = n * D * (2 * window * 32 + 8) + n * 12
    rounds = max(1, math.ceil(math.log(max(S, 2), 64)))
    chain = 1 + 2 * rounds
    groups = math.ceil(n * D / RESIDENT_WAVES)
    stream_s, chain_s = moved / STREAM_BYTES_PER_S, groups * chain * MISS_S
    return dict(bytes_moved=moved, rounds_per_search=rounds, dependent_loads_per_wave=chain, groups_of_resident_waves=groups,
                stream_ms=1e3 * stream_s, dependent_loads_ms=1e3 * chain_s, estimate_ms=1e3 * (stream_s + chain_s))


def window_at_scale(opt, n, D, S, dt, out_samples, span, seed, samples, calls):
    dev = torch.device("cuda", 0)
    traj, counts, t0 = resident_batch(n, D, S, dt, seed, dev)
    packed = dict(batch=n, center=np.zeros((2, 7)), max_static=0, max_dynamic=D, max_vertices=4, max_samples=S)
    packed["center"][1, 0] = 1.0
    poly = torch.zeros((n, D, 4, 2), dtype=torch.float64, device=dev)
    pcnt = torch.full((n, D), 4, dtype=torch.int32, device=dev)
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, static_points=None, static_counts=None, dynamic_polygon_points=poly.data_ptr(),
                                dynamic_polygon_counts=pcnt.data_ptr(), dynamic_trajectories=traj.data_ptr(),
                                dynamic_trajectory_counts=counts.data_ptr())
    window = int(round(span / dt)) + 2      # the samples within the span and one either side
    est = estimate(n, D, S, window)         # before anything runs
    out = torch.zeros((n, D, out_samples, 4), dtype=torch.float64, device=dev)
    ocnt = torch.zeros((n, D), dtype=torch.int32, device=dev)
    ok = torch.zeros((n,), dtype=torch.int32, device=dev)
    twin = torch.empty((n, D, window, 4), dtype=torch.float64, device=dev)
    src_like = torch.empty_like(twin)
    info = {}

    def call():
        rc, info["n_overflow"] = opt.window_scenes_raw(sb, t0.data_ptr(), span, out_samples, out.data_ptr(), ocnt.data_ptr(), ok.data_ptr())
        _chk(rc, "in cilqr_window_scenes_batch")

    def copy():
        twin.copy_(src_like, non_blocking=True)       # hipMemcpyAsync device to device, the windows' byte count
        torch.cuda.current_stream().synchronize()

    t = _timed(call, samples, calls)
    c = _timed(copy, samples, calls)
    got_counts = ocnt.cpu().numpy()
    written = int(got_counts.clip(min=0).sum()) * 32
    pick = np.linspace(0, n - 1, min(n, 16)).astype(int)
    same = True
    for b in pick:
        flat = dict(center=packed["center"], static_points=np.zeros((0, 2)), static_counts=np.zeros(0, np.int32),
                    dynamic_polygon_points=np.zeros((4 * D, 2)), dynamic_polygon_counts=np.full(D, 4, np.int32),
                    dynamic_trajectories=traj[b].cpu().numpy().reshape(-1, 4), dynamic_trajectory_counts=np.full(D, S, np.int32))
        rows, cnt, _ = api.window_scene(flat, float(t0[b].item()), span, out_samples)
        same = same and np.array_equal(cnt, got_counts[b]) and np.array_equal(rows.view(np.uint64), out[b].cpu().numpy().view(np.uint64))
    return dict(scenes=n, dynamic=D, source_samples=S, sample_period_s=dt, span_s=span, out_samples=out_samples,
                resident_source_bytes=int(traj.numel() * 8), window_samples_by_shape=window,
                window_samples_measured=dict(min=int(got_counts.min()), max=int(got_counts.max())), n_overflow=info["n_overflow"],
                estimate=est, call=t, bytes_read_plus_written=2 * written,
                bytes_per_s=2 * written / (1e-3 * t["median_ms"]), call_over_estimate=t["median_ms"] / est["estimate_ms"],
                memcpy_d2d_of_output=dict(bytes=int(twin.numel() * 8), **c), call_over_memcpy=t["median_ms"] / c["median_ms"],
                sampled_scenes_equal_host_call=bool(same))


def _recording(traj, S, dt):
    t = np.arange(S) * dt
    span = max(traj[-1, 0] - traj[0, 0], dt)
    v = (traj[-1, 1:3] - traj[0, 1:3]) / span
    return np.stack([t, traj[0, 1] + v[0] * t, traj[0, 2] + v[1] * t, np.full_like(t, traj[0, 3])], axis=1)


def cycle(n, S, dt, seed, repeats, workers):
    """one planning cycle at scene time 0.5 s after a first cold cycle, the window cut on the device vs shifted and uploaded"""
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, workers=workers)
    sf = scene_io.from_generator(sc)
    scenes = [dataclasses.replace(s, dynamic=[scene_io.DynamicObstacle(d.polygon, _recording(d.trajectory, S, dt)) for d in s.dynamic])
              for s in sf.scenes]
    packed = scene_io.pack_scene_batch(sf.center, scenes)
    K, n_drive = spec.n_steps + 1, 6
    span = spec.n_steps * spec.dt
    out_samples = int(round(span / dt)) + 3
    dp_cfg, cor_cfg = api.default_dp_config(tf=span, delta_t=spec.dt), api.default_corridor_config()
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    D = packed["max_dynamic"]
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    win, wcnt, wok = z(n, D, out_samples, 4), z(n, D, dt=torch.int32), z(n, dt=torch.int32)
    sb_src = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    ptrs = {k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS}
    ptrs.update(dynamic_trajectories=win.data_ptr(), dynamic_trajectory_counts=wcnt.data_ptr())
    sb_win = api.scene_batch_struct(dict(packed, max_samples=out_samples), api.MEM_DEVICE, **ptrs)
    rec = dict(scenes=n, source_samples=S, sample_period_s=dt, out_samples=out_samples, n_drive=n_drive,
               scene_batch_bytes=int(sum(packed[k].nbytes for k in api._SCENE_BATCH_ARRAYS)),
               window_bytes=int(n * D * out_samples * 32))
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=n, cmax=spec.cmax, max_lane_segments=256) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = opt.cfg.max_iter
        traj, hist, prev = z(n, K, 10), z(n, M + 1, 5), z(n, K, 10)
        n_cost, status, outcome, shift, tok = (z(n, dt=torch.int32) for _ in range(5))
        driven = z(n, n_drive, 10)
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(), None, None, None)
        start_h = np.ascontiguousarray(sc["start"], dtype=np.float64)

        def plan_and_track(t_start4, t_start6, warm):
            rc, _, _ = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb_win, t_start4.data_ptr(), K, sol, None, None, outcome.data_ptr(), warm=warm)
            _chk(rc, "in cilqr_plan_scenes_batch_warm")
            rc, _ = opt.track_raw(n, api.ROWS_TRAJ, traj.data_ptr(), K, t_start6.data_ptr(), n_drive, driven.data_ptr(), tok.data_ptr(), api.MEM_DEVICE)
            _chk(rc, "in cilqr_track_rows_batch")

        # cycle 0, cold, at t0 = 0: what both variants start from
        t0 = z(n)
        torch.cuda.synchronize()
        rc, _ = opt.window_scenes_raw(sb_src, t0.data_ptr(), span, out_samples, win.data_ptr(), wcnt.data_ptr(), wok.data_ptr())
        _chk(rc, "in cilqr_window_scenes_batch")
        s4 = torch.from_numpy(start_h).to(dev)
        s6 = torch.cat([s4, z(n, 2)], dim=1).contiguous()
        torch.cuda.synchronize()
        plan_and_track(s4, s6, None)
        prev.copy_(traj)
        shift.copy_(torch.where(outcome == 0, n_drive - 1, -1).to(torch.int32))
        last = driven[:, n_drive - 1].cpu().numpy()
        next6, next_t0 = np.ascontiguousarray(last[:, 1:7]), np.ascontiguousarray(last[:, 0] - driven[:, 0, 0].cpu().numpy())
        warm = api.WarmStart(api.MEM_DEVICE, api.ROWS_TRAJ, prev.data_ptr(), shift.data_ptr())
        host_windows = win.cpu().numpy()          # the host's own copy of the windows at t0 = 0: what it shifts
        host_counts = wcnt.cpu().numpy()
        rec["cycle0"] = dict(planned=int((outcome == 0).sum().item()), tracked=int(tok.sum().item()))

        def on_device():
            d_t0 = torch.from_numpy(next_t0).to(dev)
            d6 = torch.from_numpy(next6).to(dev)
            d4 = d6[:, :4].contiguous()
            torch.cuda.synchronize()
            rc, _ = opt.window_scenes_raw(sb_src, d_t0.data_ptr(), span, out_samples, win.data_ptr(), wcnt.data_ptr(), wok.data_ptr())
            _chk(rc, "in cilqr_window_scenes_batch")
            plan_and_track(d4, d6, warm)

        def reupload():
            shifted = host_windows.copy()
            shifted[:, :, :, 0] -= next_t0[:, None, None]
            win.copy_(torch.from_numpy(shifted))
            wcnt.copy_(torch.from_numpy(host_counts))
            d6 = torch.from_numpy(next6).to(dev)
            d4 = d6[:, :4].contiguous()
            torch.cuda.synchronize()
            plan_and_track(d4, d6, warm)

        for name, fn in (("window_on_device", on_device), ("host_shift_and_upload", reupload)):
            fn()
            torch.cuda.synchronize()
            wall = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - a))
            rec[name] = dict(wall=_spread(wall), planned=int((outcome == 0).sum().item()), tracked=int(tok.sum().item()))
        rec["uploaded_bytes_per_cycle"] = dict(window_on_device=int(n * 8 + n * 48), host_shift_and_upload=int(rec["window_bytes"] + n * D * 4 + n * 48))
        rec["host_shift_over_window_on_device"] = rec["host_shift_and_upload"]["wall"]["median_ms"] / rec["window_on_device"]["wall"]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", type=int, default=65536)
    ap.add_argument("--dynamic", type=int, default=9)
    ap.add_argument("--source-samples", type=int, default=1501)
    ap.add_argument("--span", type=float, default=5.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4, help="back-to-back calls per sample")
    ap.add_argument("--cycle-scenes", type=int, default=2048, help="scenes of the planning-cycle comparison (0: skip it)")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_scene_window.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_window_bench: no GPU; nothing is measured without one")
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/scene_window_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), stream_bytes_per_s_assumed=STREAM_BYTES_PER_S, dependent_miss_s_assumed=MISS_S,
               calls_per_sample=a.calls)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=1, cmax=16) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        for name, dt, out_samples in (("rate_10ms", 0.01, 512), ("rate_100ms", 0.1, 64)):
            rec[name] = window_at_scale(opt, a.scenes, a.dynamic, a.source_samples, dt, out_samples, a.span, a.seed, a.samples, a.calls)
            torch.cuda.empty_cache()
    if a.cycle_scenes > 0:
        rec["cycle"] = cycle(a.cycle_scenes, a.source_samples, 0.01, a.seed, 3, a.workers)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
