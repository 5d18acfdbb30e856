#!/usr/bin/env python3
"""Constraint margins behind a solve (cilqr_constraint_margins_batch) at bench scale: the bench workload (BASELINE
configs[2]: 65536 mix11 problems, K = 51, cmax = 16, the generator's lane tables) is solved once with every array resident
in HBM, the call then reads the solve's inputs and its `traj` where they lie -- with the per-knot outputs (margins, which)
and without them.

    python tools/margins_bench.py                          # 65536 mix11 problems
    python tools/margins_bench.py --problems 4096 --out /tmp/x.json

The device time is HIP events on the handle's stream around --burst back-to-back calls (an otherwise idle GPU, one warm-up
call), divided by the burst; median, min and max over --calls such measurements.

THE ESTIMATE is made from counts alone, before anything is timed (estimate()), as the sum of two terms that are taken not
to overlap:
  * the bytes the call must move -- the raw planes (B K cmax 24 B: 1.28 GB), the counts, the rows and what it writes --
    at the rate profiles/r11_resample.json measured for a streaming kernel of this library (shared_axis_5x: 4.41 TB/s read
    plus written);
  * the segment distances of the lane scans -- B K D (n_left + n_right), every disc against every segment of both tables --
    at the rate profiles/r12_frenet.json shows for squared distances out of LDS (3.79e12 per second).
The record carries both terms, the measured time and measured / estimated.  No threshold: the call is new.

The census is the reason for the feature: per solver status, how many problems have each bit of `violated` set at
tol = 0 and at tol = 1e-3 in every family, with the smallest margin of each family.  One JSON line is printed and written
to --out (default profiles/r14_margins.json).
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

from cilqr_amd import api, scenario  # noqa: E402

STATUS_NAMES = {0: "status_0", 1: "converged_1", 2: "converged_2", 3: "converged_3", 4: "status_4", 5: "status_5", 6: "no_corridor"}
STREAM_BYTES_PER_S = 4.41e12          # profiles/r11_resample.json, shared_axis_5x.bytes_per_s
SQUARED_DISTANCES_PER_S = 3.79e12     # profiles/r12_frenet.json, plan_rows.distance_evaluations_per_s


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), measurements=len(a))


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def estimate(B, K, cmax, D, n_left, n_right, per_knot):
    """From counts alone: dict(bytes_read, bytes_written, segment_distances, memory_ms, scan_ms, estimated_ms)."""
    bytes_read = B * K * cmax * 24 + B * K * 4 + B * K * api.ROWS_FIELDS[api.ROWS_TRAJ] * 8
    bytes_written = B * (api.MARGIN_FIELDS * 12 + 4)
    if per_knot:
        bytes_written += B * K * (api.MARGIN_FIELDS * 8 + api.MARGIN_WHICH_FIELDS * 4)
    segment_distances = B * K * D * (n_left + n_right)
    memory_ms = 1e3 * (bytes_read + bytes_written) / STREAM_BYTES_PER_S
    scan_ms = 1e3 * segment_distances / SQUARED_DISTANCES_PER_S
    return dict(bytes_read=int(bytes_read), bytes_written=int(bytes_written), segment_distances=int(segment_distances),
                memory_ms=memory_ms, scan_ms=scan_ms, estimated_ms=memory_ms + scan_ms)


def _census(violated, min_margin, status):
    out = {}
    for s in np.unique(status):
        sel = status == s
        fam = {}
        for f, name in enumerate(api.MARGIN_NAMES):
            v = min_margin[sel, f]
            fam[name] = dict(violated_tol_0=int(((violated[0][sel] >> f) & 1).sum()), violated_tol_1e_3=int(((violated[1][sel] >> f) & 1).sum()),
                             smallest_margin=float(v.min()))
        out[STATUS_NAMES.get(int(s), f"status_{int(s)}")] = dict(problems=int(sel.sum()), any_bit_tol_0=int((violated[0][sel] != 0).sum()),
                                                                 any_bit_tol_1e_3=int((violated[1][sel] != 0).sum()), families=fam)
    return out


def run(family, n, seed, calls, burst, workers):
    sc = scenario.generate(family, n, seed=seed, workers=workers)
    K, cmax = sc["n_steps"] + 1, sc["cmax"]
    nl, nr = len(sc["left"]), len(sc["right"])
    cfg = api.default_config(sc["n_steps"])
    rec = dict(family=family, problems=n, knots=K, cmax=cmax, n_left=nl, n_right=nr, layout="CILQR_ROWS_TRAJ")
    estimates = {flag: estimate(n, K, cmax, cfg.num_of_disc, nl, nr, flag) for flag in (True, False)}      # before anything runs
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in ("start", "coarse", "corridor", "ccount")}
    left, right = api._f64(sc["left"]), api._f64(sc["right"])
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    with api.BatchIlqrOptimizer(cfg, batch_capacity=n, cmax=cmax, max_lane_segments=max(nl, nr)) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = cfg.max_iter
        traj, hist = z(n, K, 10), z(n, M + 1, 5)
        n_cost, status, n_iter = (z(n, dt=torch.int32) for _ in range(3))
        prob = opt.make_problem(n, t["start"].data_ptr(), t["coarse"].data_ptr(), t["corridor"].data_ptr(), t["ccount"].data_ptr(),
                                cmax, api._ptr(left), api._ptr(right), nl, nr, api.MEM_DEVICE)
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                                n_iter.data_ptr(), None, None, None)
        _chk(opt.solve_raw(prob, sol), "in cilqr_solve_batch")
        torch.cuda.synchronize()
        h_status = status.cpu().numpy()
        margins, which = z(n, K, api.MARGIN_FIELDS), z(n, K, api.MARGIN_WHICH_FIELDS, dt=torch.int32)
        lowest, knot = z(n, api.MARGIN_FIELDS), z(n, api.MARGIN_FIELDS, dt=torch.int32)
        violated = z(n, dt=torch.int32)
        info = {}

        def call(per_knot, tol=None):
            rc, info["n_violating"] = opt.constraint_margins_raw(prob, api.ROWS_TRAJ, traj.data_ptr(), margins.data_ptr() if per_knot else None,
                                                                 which.data_ptr() if per_knot else None, lowest.data_ptr(), knot.data_ptr(),
                                                                 api._ptr(tol), violated.data_ptr())
            _chk(rc, "in cilqr_constraint_margins_batch")

        def timed(per_knot):
            call(per_knot)
            ms = []
            for _ in range(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(burst):
                    call(per_knot)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b) / burst)
            return _spread(ms)

        for per_knot, name in ((True, "with_per_knot_outputs"), (False, "minima_only")):
            s = timed(per_knot)
            e = estimates[per_knot]
            rec[name] = dict(burst=burst, call=s, estimate=dict(e, measured_over_estimated=s["median_ms"] / e["estimated_ms"]),
                             problems_per_s=n / (1e-3 * s["median_ms"]),
                             bytes_per_s=(e["bytes_read"] + e["bytes_written"]) / (1e-3 * s["median_ms"]))
        masks, counts = [], []
        for tol in (None, np.full(api.MARGIN_FIELDS, 1e-3)):
            call(True, tol)
            torch.cuda.synchronize()
            masks.append(violated.cpu().numpy().astype(np.uint32))
            counts.append(info["n_violating"])
        h_low = lowest.cpu().numpy()
        rec["n_violating_tol_0"], rec["n_violating_tol_1e_3"] = counts
        rec["by_solver_status"] = _census(masks, h_low, h_status)
        # a sample of the batch against the host call: the bound families bit for bit, the plane families to 1e-9 m
        take = np.linspace(0, n - 1, num=min(n, 64), dtype=np.int64)
        sub = dict(corridor=sc["corridor"][take], ccount=sc["ccount"][take], left=left, right=right)
        h = api.constraint_margins(cfg, sub, traj.cpu().numpy()[take], api.ROWS_TRAJ)
        d = margins.cpu().numpy()[take]
        both = np.isfinite(h["margins"]) & np.isfinite(d)
        rec["sample_against_host_call"] = dict(
            problems=int(len(take)), bound_families_equal=bool(np.array_equal(h["margins"][..., 3:], d[..., 3:])),
            plane_families_max_abs_difference_m=float(np.abs(np.where(both, h["margins"] - d, 0.0))[..., :3].max()))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", default="mix11")
    ap.add_argument("--problems", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--burst", type=int, default=4, help="back-to-back calls inside one pair of events")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_margins.json"))
    a = ap.parse_args()
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/margins_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.family, a.problems, a.seed, a.calls, a.burst, a.workers))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
