#!/usr/bin/env python3
"""cilqr_resample_rows_batch (kernels_resample.hip) at bench scale: 65536 plans of 51 knots in CILQR_ROWS_PLAN layout,
resident in HBM, resampled (a) at five times the rate on one shared axis, M = 251, and (b) at one time per plan, M = 1 with
per-problem queries -- the next cycle's start state.

    python tools/resample_bench.py
    python tools/resample_bench.py --plans 4096 --out /tmp/x.json

The kernel moves memory, so the figure is bytes over time: the rows and the queries read once plus the rows written
(computed from the shapes), over the call's time between two HIP events on the handle's stream -- one warm-up call per
shape, then --samples samples of --calls back-to-back calls each (a single call is a fraction of a millisecond), median,
min and max per call.  Every call ends in the library's wait for its stream, so a sample includes --calls launch and wait
round trips: it is the call's time, not the bare kernel's.  Beside it, as the practical ceiling for a kernel that mostly
writes, a device-to-device hipMemcpyAsync of the OUTPUT's byte count timed the same way in the same run, and the share of
the 8 TB/s peak.  One JSON line is printed and written to --out (default profiles/r11_resample.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

from cilqr_amd import api  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


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


def make_plans(n, K, dt, seed):
    """n plausible plans [n,K,11]: time s x y theta kappa velocity a delta jerk delta_rate"""
    rng = np.random.default_rng(seed)
    plan = np.zeros((n, K, api.PLAN_FIELDS))
    plan[:, :, 0] = np.arange(K) * dt
    v = rng.uniform(2.0, 12.0, (n, 1)) + np.cumsum(rng.uniform(-0.1, 0.1, (n, K)), axis=1)
    th = rng.uniform(-3.0, 3.0, (n, 1)) + np.cumsum(rng.uniform(-0.02, 0.02, (n, K)), axis=1)
    plan[:, :, 1] = np.cumsum(v * dt, axis=1)
    plan[:, :, 2], plan[:, :, 3] = np.cumsum(v * dt * np.cos(th), axis=1), np.cumsum(v * dt * np.sin(th), axis=1)
    plan[:, :, 4], plan[:, :, 6] = th, v
    plan[:, :, 5] = rng.uniform(-0.1, 0.1, (n, K))
    plan[:, :, 7:] = rng.uniform(-1.0, 1.0, (n, K, 4))
    return plan


def run(n, K, dt, seed, samples, calls):
    F = api.PLAN_FIELDS
    dev = torch.device("cuda", 0)
    plan_h = make_plans(n, K, dt, seed)
    plan = torch.from_numpy(plan_h).to(dev)
    rec = dict(plans=n, knots=K, layout="CILQR_ROWS_PLAN", key="CILQR_KEY_TIME", peak_bytes_per_s=PEAK_BYTES_PER_S,
               calls_per_sample=calls)
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=1, cmax=16) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M5 = 5 * (K - 1) + 1
        shapes = (("shared_axis_5x", torch.from_numpy(np.arange(M5) * dt / 5).to(dev), M5, False),
                  ("per_problem_one_time", torch.from_numpy(np.random.default_rng(seed + 1).uniform(0.0, dt, (n, 1))).to(dev), 1, True))
        for name, q, M, per in shapes:
            out = torch.empty((n, M, F), dtype=torch.float64, device=dev)
            twin = torch.empty_like(out)

            def call():
                rc = opt.resample_raw(n, api.ROWS_PLAN, plan.data_ptr(), K, api.KEY_TIME, q.data_ptr(), M, per, out.data_ptr(),
                                      api.MEM_DEVICE)
                if rc != api.OK:
                    raise api.CilqrError(rc, "in cilqr_resample_rows_batch")

            def copy():
                twin.copy_(out, non_blocking=True)     # hipMemcpyAsync device to device, the output's byte count
                torch.cuda.current_stream().synchronize()

            t = _timed(call, samples, calls)
            c = _timed(copy, samples, calls)
            # the result is the host call's (a sample of the plans: the host loop is not what is measured)
            pick = np.linspace(0, n - 1, min(n, 64)).astype(int)
            got, q_h = out[pick].cpu().numpy(), q.cpu().numpy()
            same = all(np.array_equal(got[j].view(np.uint64),
                                      api.resample_rows(plan_h[b], api.ROWS_PLAN, q_h[b] if per else q_h, api.KEY_TIME).view(np.uint64))
                       for j, b in enumerate(pick))
            read, written = n * K * F * 8 + q.numel() * 8, n * M * F * 8
            rate = (read + written) / (1e-3 * t["median_ms"])
            rec[name] = dict(queries_per_plan=M, per_problem=per, bytes_read=read, bytes_written=written, call=t,
                             bytes_per_s=rate, share_of_peak=rate / PEAK_BYTES_PER_S,
                             memcpy_d2d_of_output=dict(bytes=written, **c, bytes_per_s_read_plus_written=2 * written / (1e-3 * c["median_ms"])),
                             call_over_memcpy=t["median_ms"] / c["median_ms"], sampled_plans_equal_host_call=bool(same))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plans", type=int, default=65536)
    ap.add_argument("--knots", type=int, default=51)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per sample")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_resample.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: no GPU; nothing is measured without one")
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/resample_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.plans, a.knots, a.dt, a.seed, a.samples, a.calls))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
