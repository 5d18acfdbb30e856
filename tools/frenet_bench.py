#!/usr/bin/env python3
"""cilqr_frenet_rows_batch / cilqr_cartesian_points_batch (kernels_frenet.hip) at bench scale, on scenario.build_road()
(1952 centre points), everything resident in HBM:
  (a) 65536 CILQR_ROWS_PLAN trajectories of 51 knots projected onto the centre line -- 65536 x 51 x 1952 squared distances;
  (b) 65536 single points in CILQR_ROWS_POINTS layout: the start states of a planning cycle;
  (c) the inverse for 65536 x 51 (station, lateral) pairs;
  (d) the host call on (a), 16 threads, timed on 1024 trajectories and scaled to the batch.

    python tools/frenet_bench.py
    python tools/frenet_bench.py --plans 4096 --out /tmp/x.json

Timing: two HIP events on the handle's stream around --calls back-to-back calls, one warm-up call first, --samples samples;
median, min and max per call.  Every call uploads the centre line's tables and ends in the library's wait for its stream,
so a sample is the call's time, not the bare kernel's.  There is no pass / fail time.  Beside (a) stands an estimate that is
issue-slot counting only, not a measurement: 8 full-rate fp64 vector instructions per (query, centre point), 16 lanes per
SIMD and clock, 1024 SIMDs at 2.4 GHz; the record holds the measured time, the estimate and their ratio.  A sample of the
timed outputs is compared with the host call in the same run.  One JSON line is printed and written to --out (default
profiles/r12_frenet.json).
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

EST_INSTRUCTIONS, EST_LANES_PER_SIMD_CLOCK, EST_SIMDS, EST_CLOCK_HZ = 8, 16, 1024, 2.4e9
HOST_THREADS, HOST_PLANS = 16, 1024


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), samples=len(a))


def _timed(fn, samples, calls):
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


def road_center():
    road = scenario.build_road()
    n = len(road.s)
    return road, np.ascontiguousarray(np.stack([road.s, road.x, road.y, road.theta, road.kappa, np.full(n, scenario.LEFT_BOUND),
                                                np.full(n, scenario.RIGHT_BOUND)], 1))


def make_plans(road, n, K, dt, seed):
    """n plausible plans [n,K,11] along the road: time s x y theta kappa velocity a delta jerk delta_rate"""
    rng = np.random.default_rng(seed)
    plan = np.zeros((n, K, api.PLAN_FIELDS))
    v = rng.uniform(2.0, 12.0, (n, 1)) + np.cumsum(rng.uniform(-0.1, 0.1, (n, K)), axis=1)
    s = rng.uniform(0.0, max(1.0, road.length - 13.0 * K * dt), (n, 1)) + np.cumsum(v * dt, axis=1)
    lat = rng.uniform(-1.5, 1.5, (n, 1)) + np.cumsum(rng.uniform(-0.03, 0.03, (n, K)), axis=1)
    x, y = road.cartesian(s, lat)
    _, _, th, kap = road.eval(s)
    plan[:, :, 0], plan[:, :, 1], plan[:, :, 2], plan[:, :, 3] = np.arange(K) * dt, s - s[:, :1], x, y
    plan[:, :, 4], plan[:, :, 5], plan[:, :, 6] = th, kap, v
    plan[:, :, 7:] = rng.uniform(-1.0, 1.0, (n, K, 4))
    return plan


def _same_frenet(got, want):
    """the kernel's contract: seven columns and |lateral| as bits (the sign of lateral is the lean sin / cos's)"""
    cols = [0, 2, 3, 4, 5, 6, 7]
    return bool(np.array_equal(got[..., cols].view(np.uint64), np.ascontiguousarray(want[..., cols]).view(np.uint64)) and
                np.array_equal(np.abs(got[..., 1]).view(np.uint64), np.abs(want[..., 1]).view(np.uint64)) and
                np.array_equal(np.signbit(got[..., 1]), np.signbit(want[..., 1])))


def run(n, K, dt, seed, samples, calls):
    dev = torch.device("cuda", 0)
    road, center = road_center()
    nc = len(center)
    plan_h = make_plans(road, n, K, dt, seed)
    plan = torch.from_numpy(plan_h).to(dev)
    rec = dict(plans=n, knots=K, n_center=nc, calls_per_sample=calls)
    pick = np.linspace(0, n - 1, min(n, 64)).astype(int)
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=1, cmax=16) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)

        def check(rc, what):
            if rc != api.OK:
                raise api.CilqrError(rc, what)

        # (a) the plans
        fr = torch.empty((n, K, api.FRENET_FIELDS), dtype=torch.float64, device=dev)
        t = _timed(lambda: check(opt.frenet_raw(center, n, api.ROWS_PLAN, plan.data_ptr(), K, fr.data_ptr(), api.MEM_DEVICE),
                                 "in cilqr_frenet_rows_batch"), samples, calls)
        got = fr[pick].cpu().numpy()
        same = all(_same_frenet(got[j], api.frenet_rows(center, plan_h[b], api.ROWS_PLAN)) for j, b in enumerate(pick))
        pairs = n * K * nc
        est_ms = 1e3 * EST_INSTRUCTIONS * pairs / (EST_LANES_PER_SIMD_CLOCK * EST_SIMDS * EST_CLOCK_HZ)
        rec["plan_rows"] = dict(layout="CILQR_ROWS_PLAN", queries=n * K, distance_evaluations=pairs, call=t,
                                distance_evaluations_per_s=pairs / (1e-3 * t["median_ms"]),
                                estimate=dict(ms=est_ms, fp64_instructions_per_evaluation=EST_INSTRUCTIONS,
                                              lanes_per_simd_and_clock=EST_LANES_PER_SIMD_CLOCK, simds=EST_SIMDS, clock_hz=EST_CLOCK_HZ,
                                              note="issue-slot counting only, not a measurement"),
                                measured_over_estimate=t["median_ms"] / est_ms, sampled_plans_equal_host_call=bool(same))
        # (b) one point per plan: the cycle's start states
        pts_h = np.ascontiguousarray(plan_h[:, 0, 2:4])
        pts = torch.from_numpy(pts_h).to(dev)
        fr1 = torch.empty((n, 1, api.FRENET_FIELDS), dtype=torch.float64, device=dev)
        t = _timed(lambda: check(opt.frenet_raw(center, n, api.ROWS_POINTS, pts.data_ptr(), 1, fr1.data_ptr(), api.MEM_DEVICE),
                                 "in cilqr_frenet_rows_batch"), samples, calls)
        same = _same_frenet(fr1[pick, 0].cpu().numpy(), api.frenet_rows(center, pts_h[pick], api.ROWS_POINTS))
        rec["single_points"] = dict(layout="CILQR_ROWS_POINTS", queries=n, distance_evaluations=n * nc, call=t,
                                    distance_evaluations_per_s=n * nc / (1e-3 * t["median_ms"]), sampled_points_equal_host_call=bool(same))
        # (c) the inverse of (a)'s result
        sl = fr[:, :, :2].contiguous()
        xyt = torch.empty((n, K, 3), dtype=torch.float64, device=dev)
        t = _timed(lambda: check(opt.cartesian_raw(center, n * K, sl.data_ptr(), xyt.data_ptr(), api.MEM_DEVICE),
                                 "in cilqr_cartesian_points_batch"), samples, calls)
        got, sl_h = xyt[pick].cpu().numpy(), sl[pick].cpu().numpy()
        want = np.stack([api.cartesian_points(center, sl_h[j]) for j in range(len(pick))])
        rec["cartesian"] = dict(pairs=n * K, call=t, pairs_per_s=n * K / (1e-3 * t["median_ms"]),
                                sampled_theta_equals_host_call=bool(np.array_equal(got[..., 2].view(np.uint64), want[..., 2].view(np.uint64))),
                                sampled_xy_max_abs_difference_to_host_call=float(np.max(np.abs(got[..., :2] - want[..., :2]))),
                                round_trip_max_distance_m=float(torch.hypot(xyt[..., 0] - plan[..., 2], xyt[..., 1] - plan[..., 3]).max()))
    # (d) the host call, HOST_THREADS threads (the C call releases the interpreter lock), on the first HOST_PLANS plans
    m = min(n, HOST_PLANS)
    chunks = np.array_split(np.arange(m), HOST_THREADS)
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        def work(idx):
            return api.frenet_rows(center, plan_h[idx].reshape(-1, api.PLAN_FIELDS), api.ROWS_PLAN)
        list(pool.map(work, chunks))
        t0 = time.perf_counter()
        list(pool.map(work, chunks))
        host_ms = 1e3 * (time.perf_counter() - t0)
    rec["host_call"] = dict(threads=HOST_THREADS, plans_timed=m, ms_timed=host_ms, ms_scaled_to_batch=host_ms * n / m,
                            over_gpu_call=host_ms * n / m / rec["plan_rows"]["call"]["median_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plans", type=int, default=65536)
    ap.add_argument("--knots", type=int, default=51)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per sample")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_frenet.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frenet_bench: no GPU; nothing is measured without one")
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/frenet_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.plans, a.knots, a.dt, a.seed, a.samples, a.calls))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
