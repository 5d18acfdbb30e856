#!/usr/bin/env python3
"""cilqr_track_rows_batch (kernels_track.hip) at bench scale, beside the kernel it shares its steps with: 65536 distinct
mix11 coarse trajectories of 51 knots, resident in HBM.

    python tools/track_bench.py
    python tools/track_bench.py --plans 4096 --out /tmp/x.json

Recorded, each as the call's time (launch to the library's wait for its stream, wall clock around the call: every figure is
tens of milliseconds) -- one warm-up call, then --samples calls, median, min and max:
  (a) init_guess   cilqr_stage_init_guess on a CILQR_INIT_TRACKER handle loaded with the same trajectories (chord stations):
                   k_init_guess_tracker, the yardstick
  (b) track_full   cilqr_track_rows_batch on them as CILQR_ROWS_COARSE rows (stations = the chord lengths), start6 = (start,
                   0, 0), n_drive = 51: the same simulation, plus the gather pre-pass and the rows out
  (c) track_cycle  the same with n_drive = 6: one 0.5 s cycle
  (d) prepass      the same with n_drive = 1: the gather pre-pass and a tracking kernel that records the start and stops --
                   the pre-pass has no entry point of its own
  (e) host         cilqr_track_rows on 16 threads over the first --host-plans plans, scaled to --plans
and b_over_a, the ratio the expectation (within 1.25) is about.  The driven rows of (b) are compared with X / U of (a) bit for
bit.  One JSON line is printed and written to --out (default profiles/r15_track.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

from cilqr_amd import api, scenario  # noqa: E402

CMAX = 4


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), samples=len(a))


def _timed(fn, samples):
    fn()
    ms = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return _spread(ms)


def make_inputs(n, seed, workers):
    chunk = 4096
    parts = [scenario.generate("mix11", min(chunk, n - c0), seed=seed, first_problem=c0, workers=workers) for c0 in range(0, n, chunk)]
    start = np.ascontiguousarray(np.concatenate([p["start"] for p in parts]))
    coarse = np.ascontiguousarray(np.concatenate([p["coarse"] for p in parts]))
    return start, coarse, parts[0]["left"], parts[0]["right"], float(parts[0]["dt"])


def box_corridors(coarse, half=10.0):
    """a plain box around every knot: the corridor a load needs (the init guess does not read it)"""
    B, K = coarse.shape[:2]
    th = coarse[:, :, 2]
    n = np.stack([np.stack([np.cos(th), np.sin(th)], -1), np.stack([-np.cos(th), -np.sin(th)], -1),
                  np.stack([-np.sin(th), np.cos(th)], -1), np.stack([np.sin(th), -np.cos(th)], -1)], 2)
    cor = np.zeros((B, K, CMAX, 3))
    cor[:, :, :, :2] = n
    cor[:, :, :, 2] = (n * coarse[:, :, None, :2]).sum(-1) + half
    return cor, np.full((B, K), 4, np.int32)


def chord_stations(coarse):
    """[B,K] by the rule's hypot, all plans at once (cilqr_amd/track.py: hypot_ref, vectorised)"""
    dx, dy = np.abs(np.diff(coarse[:, :, 0], axis=1)), np.abs(np.diff(coarse[:, :, 1], axis=1))
    ax, ay = np.maximum(dx, dy), np.minimum(dx, dy)
    with np.errstate(all="ignore"):
        h = np.sqrt(ax * ax + ay * ay)
        near = h <= 2.0 * ay
        d1, d2 = h - ay, h - ax
        t1 = np.where(near, ax * (2.0 * d1 - ax), 2.0 * d2 * (ax - 2.0 * ay))
        t2 = np.where(near, (d1 - 2.0 * (ax - ay)) * d1, (4.0 * d2 - ay) * ay + d2 * d2)
        h = np.where(ax >= ay * 2.0 ** 54, ax + ay, h - (t1 + t2) / (2.0 * h))
    s = np.zeros(coarse.shape[:2])
    for k in range(1, coarse.shape[1]):      # summed knot by knot, as the rule does
        s[:, k] = s[:, k - 1] + h[:, k - 1]
    return s


def run(n, seed, samples, host_plans, threads):
    dev = torch.device("cuda", 0)
    start, coarse, left, right, dt = make_inputs(n, seed, threads)
    K = coarse.shape[1]
    rec = dict(plans=n, knots=K, family="mix11", seed=seed, distinct=int(len(np.unique(coarse.reshape(n, -1), axis=0))))
    # ---- (a) the init guess of a solve
    cfg = api.default_config(K - 1, init_guess=api.INIT_TRACKER, dt=dt)
    cor, cnt = box_corridors(coarse)
    sc = dict(start=start, coarse=coarse, corridor=cor, ccount=cnt, left=left, right=right, n_steps=K - 1, cmax=CMAX)
    with api.BatchIlqrOptimizer(cfg, batch_capacity=n, cmax=CMAX, max_lane_segments=64) as opt:
        opt.stage_load(sc)
        rec["init_guess"] = _timed(opt.stage_init_guess, samples)
        X, U = opt.read(api.T_X), opt.read(api.T_U)
        del cor, cnt, sc
        # ---- (b) (c) (d) the same trajectories as rows
        rows_h = np.zeros((n, K, api.COARSE_FIELDS))
        rows_h[:, :, 0] = np.array([dt * i for i in range(K)])
        rows_h[:, :, 1] = chord_stations(coarse)
        rows_h[:, :, 2:5], rows_h[:, :, 6:9] = coarse[:, :, :3], coarse[:, :, 3:6]
        start6_h = np.concatenate([start, np.zeros((n, 2))], axis=1)
        rows, start6 = torch.from_numpy(rows_h).to(dev), torch.from_numpy(np.ascontiguousarray(start6_h)).to(dev)
        driven = torch.zeros((n, K, 10), dtype=torch.float64, device=dev)
        ok = torch.zeros(n, dtype=torch.int32, device=dev)
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        failed = {}

        def call(n_drive):
            def fn():
                rc, failed[n_drive] = opt.track_raw(n, api.ROWS_COARSE, rows.data_ptr(), K, start6.data_ptr(), n_drive,
                                                    driven.data_ptr(), ok.data_ptr(), api.MEM_DEVICE)
                if rc != api.OK:
                    raise api.CilqrError(rc, "in cilqr_track_rows_batch")
            return fn

        for name, n_drive in (("prepass", 1), ("track_cycle", 6), ("track_full", K)):
            rec[name] = dict(n_drive=n_drive, **_timed(call(n_drive), samples), failed=failed[n_drive])
        torch.cuda.synchronize()
        d = driven.cpu().numpy()
        rec["track_full"]["equals_init_guess_bit_for_bit"] = bool(
            np.array_equal(d[:, :, 1:7].view(np.int64), np.ascontiguousarray(X).view(np.int64)) and
            np.array_equal(d[:, :-1, 8:10].view(np.int64), np.ascontiguousarray(U).view(np.int64)))
        opt.set_stream(0)
        rec["handle_device_bytes"] = opt.device_bytes()   # arenas of a 65536-problem handle and the track call's blocks
    rec["b_over_a"] = rec["track_full"]["median_ms"] / rec["init_guess"]["median_ms"]
    rec["expectation"] = "b_over_a <= 1.25"
    # ---- (e) the host call
    m = min(host_plans, n)
    hcfg = api.default_config(K - 1, dt=dt)
    tcfg = api.TrackerConfig()
    api.lib().cilqr_default_tracker_config(C.byref(tcfg))

    def one(b):
        return api.track_rows(hcfg, tcfg, rows_h[b], api.ROWS_COARSE, start6_h[b])[0]

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(min(m, 64))))
        t0 = time.perf_counter()
        host = list(pool.map(one, range(m)))
        t_host = time.perf_counter() - t0
    worst = max(float(np.abs(host[b] - d[b]).max()) for b in range(m))
    rec["host"] = dict(threads=threads, plans=m, ms=1e3 * t_host, scaled_to_all_plans_ms=1e3 * t_host * n / m,
                       largest_distance_to_the_kernel=worst)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plans", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--host-plans", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_track.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: no GPU; nothing is measured without one")
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/track_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.plans, a.seed, a.samples, a.host_plans, a.threads))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
