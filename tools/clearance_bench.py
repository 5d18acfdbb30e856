#!/usr/bin/env python3
"""Clearance behind the scene pipeline (cilqr_clearance_rows_batch) on DISTINCT scenes of a family at bench scale:
cilqr_plan_scenes_batch plans the batch, the call then reads the pipeline's `plan` rows where they lie in HBM -- at the
knots (51 rows) and resampled on the device at five times the rate (251 rows).  Beside it, in the same run and on the same
rows, the collision audit (cilqr_check_collisions_batch).

    python tools/clearance_bench.py                          # 65536 mix11 scenes
    python tools/clearance_bench.py --scenes 4096 --out /tmp/x.json

The device time is HIP events on the handle's stream around --burst back-to-back calls (arrays in HBM, an otherwise idle
GPU, one warm-up call), divided by the burst; median, min and max over --calls such measurements.  The estimate is made
from counts alone, before anything is timed (estimate(): the segment distances at 100 fp64 instructions each on a quarter
of the chip's non-FMA fp64 rate, plus the dependent loads of the time bisections, 0.8 us each, one chain per round of a
workgroup, two workgroups per CU); the record carries it and the ratio measured / estimated.  The census answers how close
the trajectories of each solver status come: quantiles of min_clearance and the count below 0; `blind_spot` counts the
scenes and knots with a negative clearance where the audit's mask (collision_buffer 0) is 0.  One JSON line is printed and
written to --out (default profiles/r13_clearance.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

from cilqr_amd import api, scenario, scene_io  # noqa: E402

STATUS_NAMES = {0: "status_0", 1: "converged_1", 2: "converged_2", 3: "converged_3", 4: "status_4", 5: "status_5", 6: "no_corridor"}
FP64_LANE_OPS_PER_S = 39.3e12      # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz: one non-fused fp64 instruction per lane and cycle
CUS, WORKGROUPS_PER_CU, LANES = 256, 2, 256


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), measurements=len(a))


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def estimate(packed, n_rows):
    """From counts alone: (segment distances, bisection loads, estimated ms)."""
    B = int(packed["batch"])
    live_dyn = (packed["dynamic_polygon_counts"] > 0) & (packed["dynamic_trajectory_counts"] > 0)
    edges = int(packed["static_counts"].sum()) + int((packed["dynamic_polygon_counts"] * live_dyn).sum())
    segment_distances = 2 * n_rows * edges      # two discs; an absent obstacle costs nothing, which this ignores
    depth = max(1, math.ceil(math.log2(int(packed["max_samples"]) + 1)))
    bisection_loads = n_rows * int(live_dyn.sum()) * (depth + 2)
    group = 1 << max(0, int(packed["max_dynamic"]) - 1).bit_length()
    rounds = math.ceil(n_rows * group / LANES)
    compute_s = segment_distances * 100 / (0.25 * FP64_LANE_OPS_PER_S)
    latency_s = B / (CUS * WORKGROUPS_PER_CU) * rounds * (depth + 2) * 0.8e-6
    return segment_distances, bisection_loads, 1e3 * (compute_s + latency_s)


def _census(min_clearance, status):
    out = {}
    for s in np.unique(status):
        v = min_clearance[status == s]
        f = v[np.isfinite(v)]
        q = {f"p{p:02d}": float(np.percentile(f, p)) for p in (1, 5, 25, 50, 75, 95, 99)} if len(f) else {}
        out[STATUS_NAMES.get(int(s), f"status_{int(s)}")] = dict(scenes=int(len(v)), no_obstacle_met=int(np.isinf(v).sum()),
                                                                 below_zero=int((v < 0).sum()), min=float(f.min()) if len(f) else None, **q)
    return out


def run(family, n, seed, calls, burst, workers):
    spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, workers=workers)
    sf = scene_io.from_generator(sc)
    K, cmax = spec.n_steps + 1, spec.cmax
    dp_cfg, cor_cfg = api.default_dp_config(tf=spec.n_steps * spec.dt, delta_t=spec.dt), api.default_corridor_config()
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    Q = 5 * (K - 1) + 1
    rec = dict(family=family, scenes=n, layout="CILQR_ROWS_PLAN",
               **{k: packed[k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples")})
    estimates = {rows: estimate(packed, rows) for rows in (K, Q)}      # before anything runs
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    t_start4 = torch.from_numpy(np.ascontiguousarray(sc["start"])).to(dev)
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=n, cmax=cmax, max_lane_segments=256) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = opt.cfg.max_iter
        traj, hist, plan = z(n, K, 10), z(n, M + 1, 5), z(n, K, api.PLAN_FIELDS)
        n_cost, status, outcome = (z(n, dt=torch.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(), None, None, None)
        rc, n_dp, n_cor = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb, t_start4.data_ptr(), K, sol, plan.data_ptr(), None, outcome.data_ptr())
        _chk(rc, "in cilqr_plan_scenes_batch")
        rec["plan_scenes"] = dict(dp_failed=n_dp, corridor_failed=n_cor)
        fine = z(n, Q, api.PLAN_FIELDS)
        queries = torch.from_numpy(np.ascontiguousarray(np.arange(Q) * (spec.dt / 5.0))).to(dev)
        _chk(opt.resample_raw(n, api.ROWS_PLAN, plan.data_ptr(), K, api.KEY_TIME, queries.data_ptr(), Q, False, fine.data_ptr(),
                              api.MEM_DEVICE), "in cilqr_resample_rows_batch")
        h_status = status.cpu().numpy()

        def timed(call):
            call()
            ms = []
            for _ in range(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(burst):
                    call()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b) / burst)
            return _spread(ms)

        for rows_t, n_rows in ((plan, K), (fine, Q)):
            clearance, nearest = z(n, n_rows, 4), z(n, n_rows, 4, dt=torch.int32)
            lowest, knot = z(n), z(n, dt=torch.int32)
            mask, first, n_hit = z(n, n_rows, dt=torch.uint8), z(n, dt=torch.int32), z(n, dt=torch.int32)
            info = {}

            def measure():
                rc, info["n_below"] = opt.clearance_raw(dp_cfg, sb, api.ROWS_PLAN, rows_t.data_ptr(), n_rows, clearance.data_ptr(),
                                                        nearest.data_ptr(), lowest.data_ptr(), knot.data_ptr(), 0.0)
                _chk(rc, "in cilqr_clearance_rows_batch")

            def lean():
                _chk(opt.clearance_raw(dp_cfg, sb, api.ROWS_PLAN, rows_t.data_ptr(), n_rows, None, None, lowest.data_ptr(),
                                       knot.data_ptr(), 0.0)[0], "in cilqr_clearance_rows_batch")

            def audit():
                rc, info["n_colliding"] = opt.check_collisions_raw(dp_cfg, sb, api.ROWS_PLAN, rows_t.data_ptr(), n_rows, 0.0,
                                                                   mask.data_ptr(), first.data_ptr(), n_hit.data_ptr())
                _chk(rc, "in cilqr_check_collisions_batch")

            segment_distances, bisection_loads, est_ms = estimates[n_rows]
            s_all, s_lean, s_audit = timed(measure), timed(lean), timed(audit)
            measure()
            torch.cuda.synchronize()
            h_clear, h_low, h_mask, h_first = clearance.cpu().numpy(), lowest.cpu().numpy(), mask.cpu().numpy(), first.cpu().numpy()
            knot_below = (h_clear < 0).any(axis=2)
            rec[f"rows_{n_rows}"] = dict(
                rows=n_rows, burst=burst, clearance=s_all, clearance_minimum_only=s_lean, collision_audit_same_rows=s_audit,
                estimate=dict(segment_distances=segment_distances, bisection_loads=bisection_loads, estimated_ms=est_ms,
                              measured_over_estimated=s_all["median_ms"] / est_ms),
                scenes_per_s=n / (1e-3 * s_all["median_ms"]), rows_per_s=n * n_rows / (1e-3 * s_all["median_ms"]),
                bytes_read_at_most=int(n * n_rows * api.PLAN_FIELDS * 8 + sum(packed[k].nbytes for k in api._SCENE_BATCH_ARRAYS)),
                bytes_written=int(n * n_rows * 4 * 12 + n * 12),
                n_below_zero=info["n_below"], n_colliding=info["n_colliding"], by_solver_status=_census(h_low, h_status),
                blind_spot=dict(scenes_below_zero_with_no_audit_hit=int(((h_low < 0) & (h_first == -1)).sum()),
                                knots_below_zero_with_mask_zero=int((knot_below & (h_mask == 0)).sum()),
                                knots_below_zero=int(knot_below.sum()), knots_with_a_mask=int((h_mask != 0).sum())))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", default="mix11")
    ap.add_argument("--scenes", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--burst", type=int, default=4, help="back-to-back calls inside one pair of events")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_clearance.json"))
    a = ap.parse_args()
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/clearance_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.family, a.scenes, a.seed, a.calls, a.burst, a.workers))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
