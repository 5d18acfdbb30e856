#!/usr/bin/env python3
"""The collision audit behind the scene pipeline (cilqr_check_collisions_batch) on DISTINCT scenes of a family at bench
scale: cilqr_plan_scenes_batch plans the batch, the audit then reads the pipeline's `plan` rows where they lie in HBM.
Beside it the way the same verdicts were to be had before: the rows downloaded and cilqr_check_collisions called per
scene on a pool of host threads.

    python tools/collision_audit_bench.py                          # 65536 mix11 scenes
    python tools/collision_audit_bench.py --scenes 4096 --host-scenes 512 --out /tmp/x.json

The device time is HIP events on the handle's stream around the call (arrays in HBM, an otherwise idle GPU, one warm-up
call), median, min and max over --calls calls.  Bytes: the rows, the scene batch (an upper bound: the trajectories are
searched by bisection, not streamed) and the barrier table read; the mask and the two counts per scene written.  The
histogram answers how many trajectories of each solver status touch something, and what: scenes, colliding scenes and,
per mask bit, the knots and the scenes that carry it.  The host loop is wall time on --host-scenes scenes, scaled
linearly to the batch -- the record says so.  One JSON line is printed and written to --out (default
profiles/r09_collision_audit.json).
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

BIT_NAMES = ("rear_static", "rear_barrier", "rear_dynamic", "front_static", "front_barrier", "front_dynamic")
STATUS_NAMES = {0: "status_0", 1: "converged_1", 2: "converged_2", 3: "converged_3", 4: "status_4", 5: "status_5", 6: "no_corridor"}


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), calls=len(a))


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def _histogram(mask, first_hit, status):
    out = {}
    for s in np.unique(status):
        sel = status == s
        m = mask[sel]
        out[STATUS_NAMES.get(int(s), f"status_{int(s)}")] = dict(
            scenes=int(sel.sum()), colliding_scenes=int((first_hit[sel] >= 0).sum()), colliding_knots=int((m != 0).sum()),
            knots_by_bit={n: int(((m >> i) & 1).sum()) for i, n in enumerate(BIT_NAMES)},
            scenes_by_bit={n: int((((m >> i) & 1).any(axis=1)).sum()) for i, n in enumerate(BIT_NAMES)})
    return out


def run(family, n, seed, calls, workers, host_scenes, buffer):
    spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, workers=workers)
    sf = scene_io.from_generator(sc)
    K, cmax = spec.n_steps + 1, spec.cmax
    dp_cfg, cor_cfg = api.default_dp_config(tf=spec.n_steps * spec.dt, delta_t=spec.dt), api.default_corridor_config()
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    t_start4 = torch.from_numpy(np.ascontiguousarray(sc["start"])).to(dev)
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    scene_bytes = int(sum(packed[k].nbytes for k in api._SCENE_BATCH_ARRAYS))
    rec = dict(family=family, scenes=n, knots=K, collision_buffer=buffer, layout="CILQR_ROWS_PLAN",
               **{k: packed[k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples")})
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=n, cmax=cmax, max_lane_segments=256) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = opt.cfg.max_iter
        traj, hist, plan = z(n, K, 10), z(n, M + 1, 5), z(n, K, api.PLAN_FIELDS)
        n_cost, status, outcome = (z(n, dt=torch.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(), None, None, None)
        t0 = time.perf_counter()
        rc, n_dp, n_cor = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb, t_start4.data_ptr(), K, sol, plan.data_ptr(), None, outcome.data_ptr())
        _chk(rc, "in cilqr_plan_scenes_batch")
        torch.cuda.synchronize()
        rec["plan_scenes"] = dict(wall_ms_first_call=1e3 * (time.perf_counter() - t0), dp_failed=n_dp, corridor_failed=n_cor)

        # ---- the audit, where the rows lie
        mask, first, n_hit = z(n, K, dt=torch.uint8), z(n, dt=torch.int32), z(n, dt=torch.int32)
        info = {}

        def audit():
            rc, info["n_colliding"] = opt.check_collisions_raw(dp_cfg, sb, api.ROWS_PLAN, plan.data_ptr(), K, buffer, mask.data_ptr(),
                                                               first.data_ptr(), n_hit.data_ptr())
            _chk(rc, "in cilqr_check_collisions_batch")

        audit()
        ms, wall = [], []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            a.record()
            audit()
            b.record()
            b.synchronize()
            wall.append(1e3 * (time.perf_counter() - w0))
            ms.append(a.elapsed_time(b))
        n_barrier = 2 * (int((sf.center[-1, 0] - sf.center[0, 0]) / 0.1) + 1)
        read = n * K * api.PLAN_FIELDS * 8 + scene_bytes + n_barrier * 16
        written = n * K + 2 * n * 4
        s = _spread(ms)
        h_mask, h_first, h_status = mask.cpu().numpy(), first.cpu().numpy(), status.cpu().numpy()
        rec["audit"] = dict(device=s, wall=_spread(wall), n_colliding=info["n_colliding"], rows_bytes=n * K * api.PLAN_FIELDS * 8,
                            scene_batch_bytes=scene_bytes, barrier_points=n_barrier, bytes_read_at_most=read, bytes_written=written,
                            scenes_per_s=n / (1e-3 * s["median_ms"]), knots_per_s=n * K / (1e-3 * s["median_ms"]))
        rec["by_solver_status"] = _histogram(h_mask, h_first, h_status)

        # ---- before: the rows downloaded, the host call per scene on a pool of threads
        m = min(n, host_scenes) if host_scenes > 0 else n
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = plan.cpu().numpy()
        download_s = time.perf_counter() - t0
        flats = [scene_io.flatten_scene(sf.center, q) for q in sf.scenes[:m]]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(workers) as pool:
            outs = list(pool.map(lambda b: api.check_collisions(flats[b], rows[b], api.ROWS_PLAN, dp_cfg, buffer), range(m)))
        host_s = time.perf_counter() - t0
        same = sum(int(np.array_equal(o[0], h_mask[b])) for b, o in enumerate(outs))
        host_scaled = host_s * n / m
        rec["host_loop"] = dict(host_threads=workers, scenes_measured=m, seconds_measured=host_s, seconds_scaled_to_batch=host_scaled,
                                download_bytes=int(rows.nbytes), download_s=download_s, scenes_with_the_devices_mask=same)
        rec["device_call_over_host_loop"] = (host_scaled + download_s) / (1e-3 * float(np.median(wall)))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", default="mix11")
    ap.add_argument("--scenes", type=int, default=65536)
    ap.add_argument("--host-scenes", type=int, default=4096, help="scenes the host loop is run on (0: all)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--buffer", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_collision_audit.json"))
    a = ap.parse_args()
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/collision_audit_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.family, a.scenes, a.seed, a.calls, a.workers, a.host_scenes, a.buffer))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
