#!/usr/bin/env python3
"""cilqr_carry_rows_batch (kernels_carry.hip) and cilqr_plan_scenes_batch_carry at bench scale: 65536 mix11 scenes resident
in HBM, cycle 2 of an episode with an advance of 0.5 s.

    python tools/carry_bench.py
    python tools/carry_bench.py --scenes 4096 --out /tmp/x.json

Cycle 1 is the cold pipeline at scene time 0; the tracker drives six rows (0.5 s); the scenes are windowed at 0.5 s.  Cycle 2
is then planned twice on the same arrays in the same run: with cilqr_plan_scenes_batch_warm -- unchanged code, the DP
planner for every scene: the figure to compare with -- and with cilqr_plan_scenes_batch_carry on the `plan` rows of cycle 1.

Before anything is timed the tool writes down ESTIMATES.  The carry kernel moves (n_rows fields + 19 n_knots) 8 bytes per
scene; at the 4.41 TB/s profiles/r11_resample.json records for the resample kernel that is estimate_ms.  The pipeline is
estimated as carry + audit + share x dp + rest from the parts the README records for 65536 scenes (audit 4 to 7 ms: 5.5;
k_dp_plan 4.55 s; the rest -- points, corridors, the solve, the rows -- 4.62 s - 4.55 s), scaled to the batch, with share =
the listed scenes / all scenes as one untimed call reports it.  Then the MEASUREMENTS: HIP events around --calls
back-to-back calls for the kernel (every call ends in the library's wait for its stream: it is the call's time), wall clock
around whole pipeline calls, a warm-up first, median of --samples with min and max.  Beside them the census: scenes per
`source` value, and status and final cost of the kept scenes beside the same scenes planned through the DP planner.  Nobody
had measured any of this before; no threshold is set.  One JSON line is printed and written to --out (default
profiles/r17_carry.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

from cilqr_amd import api, scenario, scene_io  # noqa: E402

STREAM_BYTES_PER_S = 4.41e12      # profiles/r11_resample.json, shared_axis_5x
README_SCENES = 65536             # what the README's parts were measured on
README_MS = dict(audit=5.5, dp=4550.0, rest=4620.0 - 4550.0)
MACHINE_SPREAD = 0.03             # between the pool's machines (README)
ADVANCE, N_DRIVE = 0.5, 6


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), samples=len(a))


def _events(fn, samples, calls):
    torch.cuda.synchronize()
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


def _wall(fn, samples):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(samples):
        torch.cuda.synchronize()
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - a))
    return _spread(ms)


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def _census(status, n_cost, hist, pick):
    """status histogram and the median of the last live cost row over the scenes `pick`"""
    if not pick.any():
        return dict(scenes=0)
    st = status[pick]
    rows = hist[pick, np.maximum(n_cost[pick], 1) - 1]
    return dict(scenes=int(pick.sum()), status={str(int(v)): int((st == v).sum()) for v in np.unique(st)},
                iterations_mean=float(n_cost[pick].mean() - 1), last_cost_row_median=[float(v) for v in np.median(rows, axis=0)],
                last_cost_rows_not_finite=int((~np.isfinite(rows).all(axis=1)).sum()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8, help="back-to-back calls per sample of the carry kernel")
    ap.add_argument("--max-start-offset", type=float, default=1.0)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_carry.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("carry_bench: no GPU; nothing is measured without one")
    n = a.scenes
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/carry_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), scenes=n, advance_s=ADVANCE, stream_bytes_per_s_assumed=STREAM_BYTES_PER_S,
               readme_parts_ms_at_65536=README_MS)
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=a.seed, scenarios=True, workers=a.workers)
    sf = scene_io.from_generator(sc)
    packed = scene_io.pack_scene_batch(sf.center, list(sf.scenes))
    K, span = spec.n_steps + 1, spec.n_steps * spec.dt
    dp_cfg, cor_cfg = api.default_dp_config(tf=span, delta_t=spec.dt), api.default_corridor_config()
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
    D, S = packed["max_dynamic"], packed["max_samples"]
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    win, wcnt, wok = z(n, D, S, 4), z(n, D, dt=torch.int32), z(n, dt=torch.int32)
    sb_src = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
    ptrs = {k: t[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS}
    ptrs.update(dynamic_trajectories=win.data_ptr(), dynamic_trajectory_counts=wcnt.data_ptr())
    sb_win = api.scene_batch_struct(packed, api.MEM_DEVICE, **ptrs)
    rec["scene_batch_bytes"] = int(sum(packed[k].nbytes for k in api._SCENE_BATCH_ARRAYS))

    with api.BatchIlqrOptimizer(n_steps=K - 1, batch_capacity=n, cmax=spec.cmax, max_lane_segments=256) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        M = opt.cfg.max_iter
        traj, hist, plan = z(n, K, 10), z(n, M + 1, 5), z(n, K, api.PLAN_FIELDS)
        n_cost, status, outcome, tok, source = (z(n, dt=torch.int32) for _ in range(5))
        dp9, driven = z(n, K, 9), z(n, N_DRIVE, 10)
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(), None, None, None)

        # ---- cycle 1: cold, at scene time 0; six driven rows; the window at 0.5 s
        t0 = z(n)
        rc, _ = opt.window_scenes_raw(sb_src, t0.data_ptr(), span, S, win.data_ptr(), wcnt.data_ptr(), wok.data_ptr())
        _chk(rc, "in cilqr_window_scenes_batch")
        s4 = torch.from_numpy(np.ascontiguousarray(sc["start"], dtype=np.float64)).to(dev)
        s6 = torch.cat([s4, z(n, 2)], dim=1).contiguous()
        torch.cuda.synchronize()
        rc, _, _ = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb_win, s4.data_ptr(), K, sol, plan.data_ptr(), None, outcome.data_ptr())
        _chk(rc, "in cilqr_plan_scenes_batch")
        rc, _ = opt.track_raw(n, api.ROWS_TRAJ, traj.data_ptr(), K, s6.data_ptr(), N_DRIVE, driven.data_ptr(), tok.data_ptr(), api.MEM_DEVICE)
        _chk(rc, "in cilqr_track_rows_batch")
        prev_plan, prev_traj = plan.clone(), traj.clone()
        asked = (outcome == 0) & (tok != 0)
        last = driven[:, N_DRIVE - 1]
        start2 = torch.where(asked[:, None], last[:, 1:5], s4).contiguous()
        advance = torch.where(asked, last[:, 0] - driven[:, 0, 0], torch.full_like(t0, -1.0)).contiguous()
        t0_2 = torch.where(asked, last[:, 0] - driven[:, 0, 0], t0).contiguous()
        shift = torch.where(asked, N_DRIVE - 1, -1).to(torch.int32).contiguous()
        rc, _ = opt.window_scenes_raw(sb_src, t0_2.data_ptr(), span, S, win.data_ptr(), wcnt.data_ptr(), wok.data_ptr())
        _chk(rc, "in cilqr_window_scenes_batch")
        rec["cycle1"] = dict(planned=int((outcome == 0).sum().item()), tracked=int(tok.sum().item()), asked=int(asked.sum().item()))
        warm = api.WarmStart(api.MEM_DEVICE, api.ROWS_TRAJ, prev_traj.data_ptr(), shift.data_ptr())
        cy = api.Carry(api.MEM_DEVICE, api.ROWS_PLAN, K, 0, prev_plan.data_ptr(), advance.data_ptr(), 1.0, a.max_start_offset, 0.0)

        # ---- the carry kernel alone: the estimate first
        moved = n * ((K * api.PLAN_FIELDS + 19 * K) * 8 + 12)
        kernel = dict(bytes_moved=moved, estimate_ms=1e3 * moved / STREAM_BYTES_PER_S)
        c9, c6, k3, stn, state = z(n, K, 9), z(n, K, 6), z(n, K, 3), z(n, K), z(n, dt=torch.int32)
        info = {}

        def carry_call():
            rc, info["n_kept"] = opt.carry_raw(n, api.ROWS_PLAN, prev_plan.data_ptr(), K, advance.data_ptr(), 1.0, K, spec.dt,
                                               c9.data_ptr(), c6.data_ptr(), k3.data_ptr(), stn.data_ptr(), state.data_ptr(),
                                               api.MEM_DEVICE)
            _chk(rc, "in cilqr_carry_rows_batch")

        kernel["call"] = _events(carry_call, a.samples, a.calls)
        kernel["bytes_per_s"] = moved / (1e-3 * kernel["call"]["median_ms"])
        kernel["call_over_estimate"] = kernel["call"]["median_ms"] / kernel["estimate_ms"]
        kernel["kept"] = info["n_kept"]
        pick = np.linspace(0, n - 1, min(n, 32)).astype(int)
        h_rows, h_adv, g9, gst = prev_plan[pick].cpu().numpy(), advance[pick].cpu().numpy(), c9[pick].cpu().numpy(), state[pick].cpu().numpy()
        same = True
        for i in range(len(pick)):
            want = api.carry_rows(h_rows[i], api.ROWS_PLAN, h_adv[i], 1.0, K, spec.dt)
            both_nan = np.isnan(want["coarse9"]) & np.isnan(g9[i])
            same = same and want["state"] == gst[i] and bool(((want["coarse9"].view(np.uint64) == g9[i].view(np.uint64)) | both_nan).all())
        kernel["sampled_scenes_equal_host_call"] = bool(same)
        rec["carry_kernel"] = kernel

        # ---- cycle 2 both ways
        def with_carry():
            res = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb_win, start2.data_ptr(), K, sol, plan.data_ptr(), dp9.data_ptr(),
                                      outcome.data_ptr(), warm=warm, carry=cy, source_ptr=source.data_ptr())
            _chk(res[0], "in cilqr_plan_scenes_batch_carry")
            info["n_kept_pipeline"], info["failed_carry"] = res[3], (res[1], res[2])

        def with_dp():
            res = opt.plan_scenes_raw(dp_cfg, cor_cfg, sb_win, start2.data_ptr(), K, sol, plan.data_ptr(), dp9.data_ptr(),
                                      outcome.data_ptr(), warm=warm)
            _chk(res[0], "in cilqr_plan_scenes_batch_warm")
            info["failed_dp"] = (res[1], res[2])

        with_carry()      # untimed: the share of listed scenes, which the estimate needs
        torch.cuda.synchronize()
        src = source.cpu().numpy()
        kept = src == 0
        share = float((~kept).mean())
        scale = n / README_SCENES
        parts = dict(carry=kernel["estimate_ms"], audit=README_MS["audit"] * scale, dp=share * README_MS["dp"] * scale,
                     rest=README_MS["rest"] * scale)
        pipe = dict(share_listed=share, estimate_parts_ms=parts, estimate_ms=float(sum(parts.values())),
                    source_census={str(v): int((src == v).sum()) for v in range(5)}, n_kept=info["n_kept_pipeline"])
        carried = dict(status=status.cpu().numpy(), n_cost=n_cost.cpu().numpy(), hist=hist.cpu().numpy(), outcome=outcome.cpu().numpy())
        pipe["carry"] = _wall(with_carry, a.samples)
        pipe["warm_dp_for_all"] = _wall(with_dp, a.samples)
        through_dp = dict(status=status.cpu().numpy(), n_cost=n_cost.cpu().numpy(), hist=hist.cpu().numpy(), outcome=outcome.cpu().numpy())
        pipe["carry_over_warm"] = pipe["carry"]["median_ms"] / pipe["warm_dp_for_all"]["median_ms"]
        pipe["carry_over_estimate"] = pipe["carry"]["median_ms"] / pipe["estimate_ms"]
        pipe["failed_dp_corridor"] = dict(carry=info["failed_carry"], warm_dp_for_all=info["failed_dp"])
        pipe["kept_scenes"] = dict(carried=_census(carried["status"], carried["n_cost"], carried["hist"], kept),
                                   through_dp=_census(through_dp["status"], through_dp["n_cost"], through_dp["hist"], kept),
                                   planned_carried=int((carried["outcome"][kept] == 0).sum()),
                                   planned_through_dp=int((through_dp["outcome"][kept] == 0).sum()))
        miss = pipe["carry_over_estimate"] - 1.0
        if abs(miss) > MACHINE_SPREAD:      # say which part: what the measurement leaves for share x dp once the others are taken as estimated
            left = pipe["carry"]["median_ms"] - parts["carry"] - parts["audit"] - parts["rest"]
            pipe["miss"] = dict(relative=miss, dp_part_ms_if_the_others_hold=left, dp_part_estimated_ms=parts["dp"],
                                warm_pipeline_measured_ms=pipe["warm_dp_for_all"]["median_ms"],
                                warm_pipeline_by_readme_ms=(README_MS["dp"] + README_MS["rest"]) * scale)
        rec["pipeline"] = pipe
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
