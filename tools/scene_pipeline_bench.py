#!/usr/bin/env python3
"""Scene batch -> trajectories in one call (cilqr_plan_scenes_batch) and its new link, the obstacle points per knot on
the GPU (cilqr_scene_points_batch), on DISTINCT scenes of a family at bench scale; beside them the way the same
thing was done before: scene_io.environment_points on a pool of threads, the upload of its array, and the three device
calls cilqr_dp_plan_batch -> cilqr_build_corridors -> cilqr_solve_batch.

    python tools/scene_pipeline_bench.py                          # 65536 mix11 scenes
    python tools/scene_pipeline_bench.py --scenes 4096 --host-scenes 512 --out /tmp/x.json

Device times are HIP events on the handle's stream around each call (arrays in HBM, the handle's work space grown by
the warm-up calls), median and spread over --calls calls; plan_scenes is also given as wall time.  The points kernel's
bytes are the live points it stores (16 B each) plus the counts; its fraction of the 8 TB/s HBM peak follows from the
event time of the whole call (the kernel, the 408-byte upload of the knot times and the stream wait).  The host
generator is wall time on --host-scenes scenes (default: all of them), scaled linearly to the batch where fewer were
run -- the record says which.  One JSON line is printed and written to --out (default profiles/r08_scene_pipeline.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

from cilqr_amd import api, scenario, scene_io  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), calls=len(a))


def _timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms, wall = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(a.elapsed_time(b))
    return ms, wall


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def run(family, n, seed, calls, warmup, workers, host_scenes):
    spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, workers=workers)
    sf = scene_io.from_generator(sc)
    K, cmax = spec.n_steps + 1, spec.cmax
    dp_cfg, cor_cfg = api.default_dp_config(tf=spec.n_steps * spec.dt, delta_t=spec.dt), api.default_corridor_config()
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    P = (packed["max_static"] + packed["max_dynamic"]) * packed["max_vertices"]
    times = np.arange(K) * spec.dt
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    t_start4 = torch.from_numpy(np.ascontiguousarray(sc["start"])).to(dev)
    t_start3 = torch.from_numpy(np.ascontiguousarray(sc["start"][:, :3])).to(dev)
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    left, right = api.road_barriers(sf.center)
    left = api.lane_constraints(left, cor_cfg.lane_segment_length, True)
    right = api.lane_constraints(right, cor_cfg.lane_segment_length, False)
    rec = dict(family=family, scenes=n, knots=K, max_points=P, scene_batch_bytes=int(sum(packed[k].nbytes for k in api._SCENE_BATCH_ARRAYS)),
               **{k: packed[k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples")})
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=n, cmax=cmax, max_lane_segments=256) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = opt.cfg.max_iter
        pts, pcnt = z(n, K, P, 2), z(n, K, dt=torch.int32)
        traj, hist, plan = z(n, K, 10), z(n, M + 1, 5), z(n, K, api.PLAN_FIELDS)
        n_cost, status, outcome = (z(n, dt=torch.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(), None, None, None)

        # ---- the points kernel
        def points():
            _chk(opt.scene_points_raw(sb, K, times, False, P, pts.data_ptr(), pcnt.data_ptr()), "in cilqr_scene_points_batch")

        ms, _ = _timed(points, calls, warmup)
        live = int(pcnt.sum().item())
        written = live * 16 + n * K * 4
        s = _spread(ms)
        rec["points"] = dict(device=s, live_points=live, bytes_written=written, dense_output_bytes=n * K * P * 16,
                             written_bytes_per_s=written / (1e-3 * s["median_ms"]),
                             fraction_of_hbm_peak=written / (1e-3 * s["median_ms"]) / HBM_PEAK_BYTES_PER_S)

        # ---- the whole pipeline in one call
        info = {}

        def pipeline():
            rc, info["dp_failed"], info["corridor_failed"] = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb, t_start4.data_ptr(), K, sol,
                                                                                  plan.data_ptr(), None, outcome.data_ptr())
            _chk(rc, "in cilqr_plan_scenes_batch")

        ms, wall = _timed(pipeline, calls, max(1, warmup))
        rec["plan_scenes"] = dict(device=_spread(ms), wall=_spread(wall), **info,
                                  status_histogram=np.bincount(status.cpu().numpy(), minlength=7).tolist(),
                                  scenes_per_s=n / (1e-3 * float(np.median(wall))), handle_device_bytes=opt.device_bytes())

        # ---- before: the host generator + the upload + the three device calls
        m = min(n, host_scenes) if host_scenes > 0 else n
        t0 = time.perf_counter()
        with ThreadPoolExecutor(workers) as pool:
            outs = list(pool.map(lambda q: scene_io.environment_points(q, times), sf.scenes[:m]))
        host_s = time.perf_counter() - t0
        del outs
        h_pts, h_cnt = pts.cpu().numpy(), pcnt.cpu().numpy()       # the same layout as the host's array, for the upload
        ups = []
        for _ in range(max(2, calls // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_pts, d_cnt = torch.from_numpy(h_pts).to(dev), torch.from_numpy(h_cnt).to(dev)
            torch.cuda.synchronize()
            ups.append(1e3 * (time.perf_counter() - t0))
        coarse, knots, found = z(n, K, 6), z(n, K, 3), z(n, dt=torch.int32)
        cor, ccnt = z(n, K, cmax, 3), z(n, K, dt=torch.int32)
        prob = opt.make_problem(n, t_start4.data_ptr(), coarse.data_ptr(), cor.data_ptr(), ccnt.data_ptr(), cmax,
                                left.ctypes.data, right.ctypes.data, left.shape[0], right.shape[0], api.MEM_DEVICE)

        def three_calls():
            rc, _ = opt.dp_plan_batch_raw(dp_cfg, sb, t_start3.data_ptr(), K, None, coarse.data_ptr(), knots.data_ptr(), None, found.data_ptr())
            _chk(rc, "in cilqr_dp_plan_batch")
            rc, _ = opt.build_corridors_raw(cor_cfg, n, K, knots.data_ptr(), d_pts.data_ptr(), d_cnt.data_ptr(), P, cor.data_ptr(),
                                            ccnt.data_ptr(), cmax, api.MEM_DEVICE)
            _chk(rc, "in cilqr_build_corridors")
            _chk(opt.solve_raw(prob, sol), "in cilqr_solve_batch")

        ms, wall = _timed(three_calls, calls, max(1, warmup))
        host_scaled = host_s * n / m
        rec["before"] = dict(host_threads=workers, host_points_scenes_measured=m, host_points_s_measured=host_s,
                             host_points_s_scaled_to_batch=host_scaled, upload_bytes=int(h_pts.nbytes + h_cnt.nbytes),
                             upload=_spread(ups), three_device_calls=_spread(ms), three_device_calls_wall=_spread(wall),
                             total_s=host_scaled + 1e-3 * float(np.median(ups)) + 1e-3 * float(np.median(wall)))
        rec["speedup_of_plan_scenes_over_before"] = rec["before"]["total_s"] / (1e-3 * rec["plan_scenes"]["wall"]["median_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", default="mix11")
    ap.add_argument("--scenes", type=int, default=65536)
    ap.add_argument("--host-scenes", type=int, default=0, help="scenes the host generator is run on (0: all)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_scene_pipeline.json"))
    a = ap.parse_args()
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/scene_pipeline_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.family, a.scenes, a.seed, a.calls, a.warmup, a.workers, a.host_scenes))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
