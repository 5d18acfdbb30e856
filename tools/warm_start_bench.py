#!/usr/bin/env python3
"""What a warm start (cilqr_solve_batch_warm) is worth on the bench workload: 65536 mix11 scenes, device-resident.

    python tools/warm_start_bench.py                          # every leg, profiles/r10_warm_start.json
    python tools/warm_start_bench.py --scenes 4096 --out /tmp/x.json

Legs, each the median of --calls solves with [min ... max], timed with HIP events on the handle's stream around the call
(arrays in HBM, an otherwise idle GPU, one warm-up solve):
  cold            cilqr_solve_batch
  warm_self       the same problems from their own solutions (shift 0)
  tight_cold      every corridor plane tightened by 5 cm (c -= 0.05 hypot(a, b)), cold
  tight_warm      the tightened problems from the UNTIGHTENED problems' solutions
Per leg: ms per solve, the sum of n_iter and the histogram of the solver status.  `first_iterate` times the kernels that make
the first iterate, through the stage entry points on the same batch: cilqr_stage_init_guess after a plain load (the configured
init-guess kernel) and after a warm load (the rollout kernel), and the load with and without the gather kernel.

The GPU work runs in child processes, one per group of legs, each under its own time limit (--limit seconds); the first
that fails or runs out of time ends the run and the record says which.  One JSON line is printed and written to --out.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = ("same", "tight", "first_iterate")


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), calls=len(a))


def _tightened(corridor, by=0.05):
    cor = corridor.copy()
    cor[..., 2] -= by * np.hypot(cor[..., 0], cor[..., 1])
    return cor


def child(group, family, n, seed, calls, workers):
    import torch  # (one HIP runtime per process: torch before libcilqr_hip.so)

    from cilqr_amd import api, scenario
    sc = scenario.generate(family, n, seed=seed, workers=workers)
    N, cmax = sc["n_steps"], sc["cmax"]
    K = N + 1
    dev = torch.device("cuda", 0)
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)   # noqa: E731
    left, right = np.ascontiguousarray(sc["left"]), np.ascontiguousarray(sc["right"])
    t = dict(start=up(sc["start"]), coarse=up(sc["coarse"]), corridor=up(sc["corridor"]), ccount=up(sc["ccount"], np.int32))
    if group == "tight":
        t["tight"] = up(_tightened(sc["corridor"]))
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    rec = {}
    with api.BatchIlqrOptimizer(n_steps=N, batch_capacity=n, cmax=cmax, max_lane_segments=256) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = opt.cfg.max_iter
        traj, prev, hist = z(n, K, 10), z(n, K, 10), z(n, M + 1, 5)
        n_cost, status, n_iter = (z(n, dt=torch.int32) for _ in range(3))
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                                n_iter.data_ptr(), None, None)

        def problem(corridor):
            return api.ProblemBatch(n, K, cmax, api.MEM_DEVICE, t["start"].data_ptr(), t["coarse"].data_ptr(), corridor.data_ptr(),
                                    t["ccount"].data_ptr(), left.shape[0], right.shape[0], left.ctypes.data, right.ctypes.data)

        def timed(fn):
            fn()
            ms = []
            for _ in range(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return _spread(ms)

        def leg(prob, warm):
            def solve():
                rc = opt.solve_raw(prob, sol, warm)
                if rc != api.OK:
                    raise api.CilqrError(rc, "in cilqr_solve_batch(_warm)")
            s = timed(solve)
            st = status.cpu().numpy()
            return dict(**s, solves_per_s=n / (1e-3 * s["median_ms"]), sum_n_iter=int(n_iter.sum().item()),
                        status_histogram={str(int(k)): int(v) for k, v in zip(*np.unique(st, return_counts=True))})

        warm = api.WarmStart(api.MEM_DEVICE, api.ROWS_TRAJ, prev.data_ptr(), None)   # no shift array: 0 for every problem
        base = problem(t["corridor"])
        if group == "same":
            rec["cold"] = leg(base, None)
            prev.copy_(traj)
            rec["warm_self"] = leg(base, warm)
        elif group == "tight":
            rc = opt.solve_raw(base, sol)
            if rc != api.OK:
                raise api.CilqrError(rc, "in cilqr_solve_batch")
            torch.cuda.synchronize()
            prev.copy_(traj)
            tight = problem(t["tight"])
            rec["tight_cold"] = leg(tight, None)
            rec["tight_warm"] = leg(tight, warm)
        else:
            rc = opt.solve_raw(base, sol)
            if rc != api.OK:
                raise api.CilqrError(rc, "in cilqr_solve_batch")
            torch.cuda.synchronize()
            prev.copy_(traj)

            def call(f, *a):
                def run():
                    rc = f(opt.h, *a)
                    if rc != api.OK:
                        raise api.CilqrError(rc, "in a stage call")
                return run
            L = api.lib()
            rec["load"] = timed(call(L.cilqr_stage_load, C.byref(base)))
            rec["init_guess"] = timed(call(L.cilqr_stage_init_guess))
            rec["load_with_gather"] = timed(call(L.cilqr_stage_load_warm, C.byref(base), C.byref(warm)))
            rec["warm_rollout"] = timed(call(L.cilqr_stage_init_guess))
            rec["gather_ms_by_difference"] = rec["load_with_gather"]["median_ms"] - rec["load"]["median_ms"]
    print("WARM_START_BENCH " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", default="mix11")
    ap.add_argument("--scenes", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds every child process may take")
    ap.add_argument("--group", default=None, choices=GROUPS, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_warm_start.json"))
    a = ap.parse_args()
    if a.group:
        child(a.group, a.family, a.scenes, a.seed, a.calls, a.workers)
        return
    rec = dict(tool="tools/warm_start_bench.py", family=a.family, scenes=a.scenes, seed=a.seed, calls=a.calls)
    for g in GROUPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--group", g, "--family", a.family, "--scenes", str(a.scenes),
               "--calls", str(a.calls), "--workers", str(a.workers), "--seed", str(a.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            rec["stopped"] = f"{g}: no result within {a.limit} s"
            break
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("WARM_START_BENCH ")]
        if r.returncode != 0 or not lines:
            rec["stopped"] = f"{g}: exit {r.returncode}: {r.stderr.strip()[-400:]}"
            break   # nothing more is started on the GPU after a failure
        got = json.loads(lines[-1][len("WARM_START_BENCH "):])
        rec.update({"first_iterate": got} if g == "first_iterate" else got)
        print(f"[{g}] done", file=sys.stderr, flush=True)
    from cilqr_amd import api
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec.update(abi=L.cilqr_abi_version(), build_id=L.cilqr_build_id().decode())
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    sys.exit(1 if "stopped" in rec else 0)


if __name__ == "__main__":
    main()
