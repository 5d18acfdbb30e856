#!/usr/bin/env python3
"""Scene -> coarse trajectory -> corridors -> trajectories with every per-problem array resident on the device:
cilqr_dp_plan_batch -> cilqr_build_corridors -> cilqr_solve_batch on DISTINCT scenes of a family, and the batched
planner alone next to the host planner (cilqr_dp_plan on a pool of threads) on the same scenes.

    python tools/dp_batch_bench.py                       # all three families at 2048 scenes + the chain at 65536 mix11
    python tools/dp_batch_bench.py --families mix11 --scenes 512 --chain-scenes 4096 --out /tmp/x.json

Device times are HIP events on the handle's stream around each call (arrays in HBM, the handle's work space grown by
the warm-up calls), median and spread over --calls calls; the host planner is wall time.  One JSON line is printed and
written to --out (default profiles/r07_dp_batch.json).  The obstacle points per knot time -- the `points` input of the
corridor producer -- depend on the scene and the knot times only and are prepared on the host before the clock starts.
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

def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]),
                p10_ms=float(a[int(0.1 * (len(a) - 1))]), p90_ms=float(a[int(round(0.9 * (len(a) - 1)))]), calls=len(a))


def _timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


class DeviceScenes:
    """The scenes of one generator call on the device, and the outputs of the three stages."""

    def __init__(self, family, n, seed, workers, with_points):
        spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
        self.spec, self.n = spec, n
        self.sc = scenario.generate(spec, n, seed=seed, scenarios=True, obstacle_points=with_points, workers=workers)
        self.sf = scene_io.from_generator(self.sc)
        self.K = spec.n_steps + 1
        self.cfg = api.default_dp_config(tf=spec.n_steps * spec.dt, delta_t=spec.dt)
        self.packed = scene_io.pack_scene_batch(self.sf.center, self.sf.scenes)
        dev = torch.device("cuda", 0)
        self.t = {k: torch.from_numpy(np.ascontiguousarray(self.packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
        self.t["start3"] = torch.from_numpy(np.ascontiguousarray(self.sc["start"][:, :3])).to(dev)
        self.t["start4"] = torch.from_numpy(np.ascontiguousarray(self.sc["start"])).to(dev)
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
        self.o = dict(coarse=z(n, self.K, 6), knots=z(n, self.K, 3), station=z(n, self.K), found=z(n, dt=torch.int32))
        self.sb = api.scene_batch_struct(self.packed, api.MEM_DEVICE, **{k: self.t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
        if with_points:
            self.t["pts"] = torch.from_numpy(np.ascontiguousarray(self.sc["obstacle_points"])).to(dev)
            self.t["pcnt"] = torch.from_numpy(np.ascontiguousarray(self.sc["obstacle_count"])).to(dev)

    def plan(self, opt):
        rc, nnf = opt.dp_plan_batch_raw(self.cfg, self.sb, self.t["start3"].data_ptr(), self.K, None, self.o["coarse"].data_ptr(),
                                        self.o["knots"].data_ptr(), self.o["station"].data_ptr(), self.o["found"].data_ptr())
        if rc != api.OK:
            raise api.CilqrError(rc, "in cilqr_dp_plan_batch")
        return nnf

    def host_plan(self, workers):
        def one(b):
            return api.dp_plan(scene_io.flatten_scene(self.sf.center, self.sf.scenes[b]), self.sc["start"][b, :3], self.cfg)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(workers) as pool:
            outs = list(pool.map(one, range(self.n)))
        return time.perf_counter() - t0, np.array([o[0] for o in outs], dtype=bool)


def planner_alone(family, n, seed, calls, warmup, workers):
    d = DeviceScenes(family, n, seed, workers, with_points=False)
    with api.BatchIlqrOptimizer(n_steps=d.K - 1, batch_capacity=1, cmax=d.spec.cmax) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        nnf = d.plan(opt)
        ms = _timed(lambda: d.plan(opt), calls, warmup)
        found = d.o["found"].cpu().numpy() != 0
    host_s, host_found = d.host_plan(workers)
    s = _spread(ms)
    return dict(family=family, scenes=n, knots=d.K, **{k: d.packed[k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples")},
                device=s, device_us_per_scene=1e3 * s["median_ms"] / n, not_found=nnf, found_equal_to_host=bool(np.array_equal(found, host_found)),
                host_threads=workers, host_s=host_s, host_ms_per_scene_per_thread=1e3 * host_s * workers / n,
                speedup_over_threaded_host=1e3 * host_s / s["median_ms"])


def chain(family, n, seed, calls, warmup, workers):
    d = DeviceScenes(family, n, seed, workers, with_points=True)
    dev = torch.device("cuda", 0)
    K, cmax, P = d.K, d.spec.cmax, d.sc["obstacle_points"].shape[2]
    left, right = np.ascontiguousarray(d.sc["left"]), np.ascontiguousarray(d.sc["right"])
    ccfg = api.default_corridor_config()
    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=n, cmax=cmax) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = opt.cfg.max_iter
        cor = torch.zeros((n, K, cmax, 3), dtype=torch.float64, device=dev)
        ccnt = torch.zeros((n, K), dtype=torch.int32, device=dev)
        traj = torch.zeros((n, K, 10), dtype=torch.float64, device=dev)
        hist = torch.zeros((n, M + 1, 5), dtype=torch.float64, device=dev)
        n_cost, status = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        prob = opt.make_problem(n, d.t["start4"].data_ptr(), d.o["coarse"].data_ptr(), cor.data_ptr(), ccnt.data_ptr(), cmax,
                                left.ctypes.data, right.ctypes.data, left.shape[0], right.shape[0], api.MEM_DEVICE)
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                                None, None, None)
        info = {}

        def corridors():
            rc, nf = opt.build_corridors_raw(ccfg, n, K, d.o["knots"].data_ptr(), d.t["pts"].data_ptr(), d.t["pcnt"].data_ptr(),
                                             P, cor.data_ptr(), ccnt.data_ptr(), cmax, api.MEM_DEVICE)
            if rc != api.OK:
                raise api.CilqrError(rc, "in cilqr_build_corridors")
            info["corridors_failed"] = nf

        def solve():
            rc = opt.solve_raw(prob, sol)
            if rc != api.OK:
                raise api.CilqrError(rc, "in cilqr_solve_batch")

        def all_three():
            info["not_found"] = d.plan(opt)
            corridors()
            solve()

        all_three()
        parts = dict(dp=_spread(_timed(lambda: d.plan(opt), calls, warmup)), corridors=_spread(_timed(corridors, calls, warmup)),
                     solve=_spread(_timed(solve, calls, warmup)), dp_corridors_solve=_spread(_timed(all_three, calls, warmup)))
        hist_st = np.bincount(status.cpu().numpy(), minlength=7).tolist()
    return dict(family=family, scenes=n, knots=K, **parts, status_histogram=hist_st, **info)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--families", default="mix11,demo80,dyn20")
    ap.add_argument("--scenes", type=int, default=2048)
    ap.add_argument("--chain-scenes", type=int, default=65536, help="0: skip the chain")
    ap.add_argument("--chain-family", default="mix11")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--chain-calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_dp_batch.json"))
    a = ap.parse_args()
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/dp_batch_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), planner=[], chain=None)
    for fam in [f for f in a.families.split(",") if f]:
        rec["planner"].append(planner_alone(fam, a.scenes, a.seed, a.calls, a.warmup, a.workers))
        print("#", json.dumps(rec["planner"][-1]), file=sys.stderr, flush=True)
    if a.chain_scenes > 0:
        rec["chain"] = chain(a.chain_family, a.chain_scenes, a.seed + 1, a.chain_calls, 1, a.workers)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
