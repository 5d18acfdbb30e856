#!/usr/bin/env python3
"""Braking along the path (cilqr_stop_rows_batch, cilqr_stop_scenes_batch) at bench scale: the bench workload (BASELINE
configs[2]: 65536 mix11 problems, K = 51) is solved once with every array resident in HBM; the solver's trajectories
(CILQR_ROWS_TRAJ) are then braked where they lie -- M = 1, 4, 8 profiles with rows and with the summaries alone, 51 rows
delta_t apart -- and cilqr_stop_scenes_batch chooses among M = 4 profiles against the scenes the plans were made in.

    python tools/stop_bench.py                          # 65536 mix11 problems
    python tools/stop_bench.py --problems 4096 --out /tmp/x.json

The device time is HIP events on the handle's stream around --burst back-to-back calls (an otherwise idle GPU, one warm-up
call per shape), divided by the burst; median, min and max over --calls such measurements.  Every call ends in the library's
wait for its stream: it is the call's time, not the bare kernel's.

THE ESTIMATES are made from counts and from figures this repository has on record, before anything is timed (estimate_*):
  * stop_rows: the bytes -- the rows read once, the plan rows and summaries written -- at the 4.41 TB/s of the resample kernel
    (profiles/r11_resample.json), PLUS the speed chain: one lane per (trajectory, profile) runs n_out - 1 dependent steps
    while the rest of its workgroup waits, taken as CHAIN_CYCLES_PER_STEP = 150 cycles a step (a guess: about a dozen
    dependent fp64 operations and three LDS stores) at 2.4 GHz, once per round of resident workgroups (the launch plan of
    kernels_stop.hip restated in launch_plan: 32 KiB of LDS a workgroup at the most, 160 KiB a CU, 256 CUs);
  * stop_scenes: that for M = 4 with rows, plus M x the 4.32 ms of the collision audit (profiles/r19_policy.json's batch,
    README), plus the gather's bytes (one slice read, one written) at the same 4.41 TB/s.
Beside every stop_rows figure with rows: a device-to-device copy of the output's byte count alone, timed the same way in the
same run.  The ratios are reported as measured; none is a pass mark.

The census is descriptive and asserts nothing, with nothing tuned to it: the statuses of all chains, and, of the plans the
audit (buffer 0) calls hit, how many receive each choice.  One JSON line is printed and written to --out (default
profiles/r20_stop.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

from cilqr_amd import api, scenario, scene_io  # noqa: E402

STREAM_BYTES_PER_S = 4.41e12          # profiles/r11_resample.json, shared_axis_5x.bytes_per_s
AUDIT_MS_PER_65536 = 4.32             # cilqr_check_collisions_batch on 65536 mix11 plans of 51 knots
CHAIN_CYCLES_PER_STEP = 150.0         # a guess, see above
CLOCK_HZ, CUS, LDS_PER_CU = 2.4e9, 256, 160 * 1024
USUAL_SPREAD = 1.3
PROFILES = {1: [(-2.0, -4.0)],
            4: [(-1.0, -2.0), (-2.0, -4.0), (-4.0, -10.0), (-6.0, -20.0)],
            8: [(-0.5, -1.0), (-1.0, -2.0), (-1.5, -3.0), (-2.0, -4.0), (-3.0, -8.0), (-4.0, -10.0), (-5.0, -15.0), (-6.0, -20.0)]}


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), measurements=len(a))


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def launch_plan(B, K, F, M, N, lds_kb=32, chunk=12):
    """kernels_stop.hip: launch_stop, restated -- trajectories per workgroup, image rows, LDS bytes, workgroups"""
    fixed, row = K * (F + 1), M * 11
    budget = max(lds_kb * 1024 // 8, fixed + row * 4)
    nc = min(chunk, N)
    ni = nc + 1 if nc < N else N
    if fixed + row * ni > budget:
        ni = (budget - fixed) // row
    run = min(16, budget // (fixed + row * ni))
    return dict(run=run, image_rows=ni, lds_bytes=(fixed + row * ni) * run * 8, workgroups=-(-B // run))


def estimate_stop(B, K, F, M, N, with_rows):
    plan = launch_plan(B, K, F, M, N)
    read = B * K * F * 8
    written = (M * B * N * 88 if with_rows else 0) + M * B * 16
    resident = CUS * max(1, min(8, LDS_PER_CU // plan["lds_bytes"]))
    rounds = math.ceil(plan["workgroups"] / resident)
    chain_ms = 1e3 * rounds * (N - 1) * CHAIN_CYCLES_PER_STEP / CLOCK_HZ
    memory_ms = 1e3 * (read + written) / STREAM_BYTES_PER_S
    return dict(launch_plan=plan, bytes_read=read, bytes_written=written, memory_ms=memory_ms, rounds_of_workgroups=rounds,
                chain_ms=chain_ms, estimated_ms=memory_ms + chain_ms)


def estimate_scenes(B, K, F, M, N):
    stop = estimate_stop(B, K, F, M, N, True)
    parts = dict(stop_rows_ms=stop["estimated_ms"], audits_ms=M * AUDIT_MS_PER_65536 * B / 65536.0,
                 gather_ms=1e3 * 2 * B * N * 88 / STREAM_BYTES_PER_S)
    return dict(parts=parts, estimated_ms=float(sum(parts.values())))


def timed(call, calls, burst):
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


def _verdict(measured, estimated):
    r = measured / estimated
    return dict(measured_over_estimated=r, within_usual_spread=bool(1 / USUAL_SPREAD <= r <= USUAL_SPREAD))


def run(n, seed, calls, burst, workers, variants):
    spec = scenario.SPECS["mix11"]
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, workers=workers)
    K, cmax, F = sc["n_steps"] + 1, sc["cmax"], api.ROWS_FIELDS[api.ROWS_TRAJ]
    N = K
    nl, nr = len(sc["left"]), len(sc["right"])
    cfg = api.default_config(sc["n_steps"])
    rec = dict(family="mix11", problems=n, knots=K, n_out=N, delta_t=cfg.dt, layout="CILQR_ROWS_TRAJ", profiles={str(m): p for m, p in PROFILES.items()},
               stream_bytes_per_s_assumed=STREAM_BYTES_PER_S, audit_ms_per_65536_assumed=AUDIT_MS_PER_65536,
               chain_cycles_per_step_assumed=CHAIN_CYCLES_PER_STEP)
    shapes = [(M, rows) for M in (1, 4, 8) for rows in (True, False)]
    est = {s: estimate_stop(n, K, F, s[0], N, s[1]) for s in shapes}                            # before anything runs
    est_scenes = estimate_scenes(n, K, F, 4, N)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in ("start", "coarse", "corridor", "ccount")}
    left, right = api._f64(sc["left"]), api._f64(sc["right"])
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    with api.BatchIlqrOptimizer(cfg, batch_capacity=n, cmax=cmax, max_lane_segments=max(nl, nr)) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        iters = cfg.max_iter
        traj, hist = z(n, K, 10), z(n, iters + 1, 5)
        n_cost, status, n_iter = (z(n, dt=torch.int32) for _ in range(3))
        prob = opt.make_problem(n, t["start"].data_ptr(), t["coarse"].data_ptr(), t["corridor"].data_ptr(), t["ccount"].data_ptr(),
                                cmax, api._ptr(left), api._ptr(right), nl, nr, api.MEM_DEVICE)
        sol = api.SolutionBatch(api.MEM_DEVICE, 0, traj.data_ptr(), hist.data_ptr(), n_cost.data_ptr(), status.data_ptr(),
                                n_iter.data_ptr(), None, None, None)
        _chk(opt.solve_raw(prob, sol), "in cilqr_solve_batch")
        torch.cuda.synchronize()

        # ---- stop_rows
        out = z(8, n, N, 11)
        twin = torch.empty_like(out)
        st, knot, travel = z(8, n, dt=torch.int32), z(8, n, dt=torch.int32), z(8, n)
        rec["stop_rows"] = {}
        for M, with_rows in shapes:
            prof = np.array(PROFILES[M])

            def call():
                _chk(opt.stop_rows_raw(n, api.ROWS_TRAJ, traj.data_ptr(), K, prof, None, cfg.dt, N, out.data_ptr() if with_rows else None,
                                       st.data_ptr(), knot.data_ptr(), travel.data_ptr(), api.MEM_DEVICE), "in cilqr_stop_rows_batch")
            c = timed(call, calls, burst)
            e = est[(M, with_rows)]
            r = dict(profiles=M, rows_written=with_rows, burst=burst, call=c, estimate=dict(e, **_verdict(c["median_ms"], e["estimated_ms"])),
                     chains_per_s=M * n / (1e-3 * c["median_ms"]), bytes_per_s=(e["bytes_read"] + e["bytes_written"]) / (1e-3 * c["median_ms"]))
            if with_rows:
                nbytes = M * n * N * 88
                src, dst = out.view(-1)[:nbytes // 8], twin.view(-1)[:nbytes // 8]

                def copy():
                    dst.copy_(src, non_blocking=True)       # hipMemcpyAsync device to device, the output's byte count
                    torch.cuda.current_stream().synchronize()
                m = timed(copy, calls, burst)
                r["memcpy_d2d_of_output"] = dict(bytes=nbytes, **m)
                r["call_over_memcpy"] = c["median_ms"] / m["median_ms"]
            codes = st[:M].flatten().cpu().numpy()
            r["status_census"] = {name: int((codes == v).sum()) for name, v in
                                  (("stopped", api.STOP_STOPPED), ("moving", api.STOP_MOVING), ("overrun", api.STOP_OVERRUN), ("refused", api.STOP_REFUSED))}
            rec["stop_rows"][f"M{M}_{'rows' if with_rows else 'summaries'}"] = r
        # ---- the launch plan's two hooks (kernels_stop.hip: launch_stop), rows written
        rec["plan_variants"] = {}
        for M in (1, 4, 8):
            prof = np.array(PROFILES[M])
            for kb, chunk in variants:
                os.environ["CILQR_STOP_LDS_KB"], os.environ["CILQR_STOP_CHUNK"] = str(kb), str(chunk)

                def call():
                    _chk(opt.stop_rows_raw(n, api.ROWS_TRAJ, traj.data_ptr(), K, prof, None, cfg.dt, N, out.data_ptr(), st.data_ptr(),
                                           knot.data_ptr(), travel.data_ptr(), api.MEM_DEVICE), "in cilqr_stop_rows_batch")
                c = timed(call, calls, burst)
                rec["plan_variants"][f"M{M}_lds{kb}_chunk{chunk}"] = dict(call=c, over_default=c["median_ms"] / rec["stop_rows"][f"M{M}_rows"]["call"]["median_ms"])
        os.environ.pop("CILQR_STOP_LDS_KB", None)
        os.environ.pop("CILQR_STOP_CHUNK", None)
        del twin

        # ---- stop_scenes, M = 4
        sf = scene_io.from_generator(sc)
        packed = scene_io.pack_scene_batch(sf.center, list(sf.scenes))
        ts = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
        sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: ts[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
        dp_cfg = api.default_dp_config(tf=(K - 1) * cfg.dt, delta_t=cfg.dt)
        prof4 = np.array(PROFILES[4])
        chosen, choice = z(n, N, 11), z(n, dt=torch.int32)
        s4, f4 = z(4, n, dt=torch.int32), z(4, n, dt=torch.int32)
        none = [0]

        def scenes_call():
            rc, none[0] = opt.stop_scenes_raw(dp_cfg, sb, api.ROWS_TRAJ, traj.data_ptr(), K, prof4, None, cfg.dt, N, 0.0, chosen.data_ptr(),
                                              choice.data_ptr(), s4.data_ptr(), f4.data_ptr())
            _chk(rc, "in cilqr_stop_scenes_batch")
        c = timed(scenes_call, calls, max(1, burst // 4))
        rec["stop_scenes"] = dict(profiles=4, collision_buffer=0.0, call=c, n_none=int(none[0]),
                                  estimate=dict(est_scenes, **_verdict(c["median_ms"], est_scenes["estimated_ms"])))

        # ---- census (descriptive): the plans the audit calls hit, by the choice they receive
        first = z(n, dt=torch.int32)
        rc, hit = opt.check_collisions_raw(dp_cfg, sb, api.ROWS_TRAJ, traj.data_ptr(), K, 0.0, None, first.data_ptr(), None)
        _chk(rc, "in cilqr_check_collisions_batch")
        torch.cuda.synchronize()
        is_hit = (first != -1).cpu().numpy()
        ch = choice.cpu().numpy()
        rec["census"] = dict(plans=n, audit_hit=int(hit), choice_of_hit_plans={str(v): int(((ch == v) & is_hit).sum()) for v in (-1, 0, 1, 2, 3)},
                             choice_of_all_plans={str(v): int((ch == v).sum()) for v in (-1, 0, 1, 2, 3)},
                             hit_plans_hit_at_knot_0=int(((first == 0).cpu().numpy() & is_hit).sum()))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=5, help="measurements per shape")
    ap.add_argument("--burst", type=int, default=8, help="back-to-back calls per measurement")
    ap.add_argument("--variants", nargs="*", default=[], help="also time the calls with rows under LDS_KB:CHUNK (CILQR_STOP_LDS_KB, CILQR_STOP_CHUNK)")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_stop.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stop_bench: no GPU; nothing is measured without one")
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/stop_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.problems, a.seed, a.calls, a.burst, a.workers, [tuple(int(x) for x in v.split(':')) for v in a.variants]))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
