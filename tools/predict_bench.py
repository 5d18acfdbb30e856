#!/usr/bin/env python3
"""cilqr_predict_scenes_batch (kernels_scene_predict.hip) at bench scale, and what planning on predictions changes.

    python tools/predict_bench.py
    python tools/predict_bench.py --scenes 4096 --episode-scenes 256 --out /tmp/x.json

(a) The call on the resident recordings of tools/scene_window_bench.py -- 65536 scenes of 9 dynamic obstacles with 1501
samples each, at 10 ms and at 100 ms, every scene at its own t0 -- with 52 samples out (0.1 s apart: the smallest count that
reaches past a 5 s horizon), timed with HIP events as that tool times its call, beside cilqr_window_scenes_batch on the same
arrays in the same run.  Before anything runs the ESTIMATE is written down from the shapes alone: the bytes written (and the
counts, t0 and two samples read per obstacle) at the 4.41 TB/s of profiles/r11_resample.json, plus the window estimate's
latency term for ONE search instead of two.  The expectation is that the call is no slower than the window call at 100 ms
sampling (one search, two sample reads, the same order of bytes out); `predict_over_window` records what was found.

(b) --episode-scenes mix11 scenes with recordings, --cycles planning cycles with carry, three times: on the recordings' windows
(the planner is handed the future), on HOLD predictions and on CONSTANT_VELOCITY predictions.  Per run the census of `source`
over all later cycles and the number of scenes whose DRIVEN rows hit the RECORDED scene in some cycle
(cilqr_check_collisions_batch on the window of the truth).  First figures; nothing is tuned to them.

One JSON line is printed and written to --out (default profiles/r18_predict.json).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402  (one HIP runtime per process: torch before libcilqr_hip.so)

import scene_window_bench as swb  # noqa: E402
from cilqr_amd import api, episode, scenario, scene_io  # noqa: E402

CARRY = dict(max_advance=1.0, max_start_offset=1.0, collision_buffer=0.0, refresh_every=0)


def _note(*what):
    print("predict_bench:", *what, file=sys.stderr, flush=True)


def estimate(n, D, S, out_samples):
    moved = n * D * (out_samples * 32 + 2 * 32 + 8) + n * 12
    rounds = max(1, math.ceil(math.log(max(S, 2), 64)))
    chain = 1 + rounds + 1                       # counts / t0, one search, the two samples
    groups = math.ceil(n * D / swb.RESIDENT_WAVES)
    stream_s, chain_s = moved / swb.STREAM_BYTES_PER_S, groups * chain * swb.MISS_S
    return dict(bytes_moved=moved, rounds_per_search=rounds, dependent_loads_per_wave=chain, groups_of_resident_waves=groups,
                stream_ms=1e3 * stream_s, dependent_loads_ms=1e3 * chain_s, estimate_ms=1e3 * (stream_s + chain_s))


def call_at_scale(opt, n, D, S, dt, window_out, span, sample_dt, out_samples, seed, samples, calls):
    dev = torch.device("cuda", 0)
    est = estimate(n, D, S, out_samples)          # before anything runs
    traj, counts, t0 = swb.resident_batch(n, D, S, dt, seed, dev)
    packed = dict(batch=n, center=np.zeros((2, 7)), max_static=0, max_dynamic=D, max_vertices=4, max_samples=S)
    packed["center"][1, 0] = 1.0
    poly = torch.zeros((n, D, 4, 2), dtype=torch.float64, device=dev)
    pcnt = torch.full((n, D), 4, dtype=torch.int32, device=dev)
    sb = api.scene_batch_struct(packed, api.MEM_DEVICE, static_points=None, static_counts=None, dynamic_polygon_points=poly.data_ptr(),
                                dynamic_polygon_counts=pcnt.data_ptr(), dynamic_trajectories=traj.data_ptr(),
                                dynamic_trajectory_counts=counts.data_ptr())
    out = torch.zeros((n, D, out_samples, 4), dtype=torch.float64, device=dev)
    win = torch.zeros((n, D, window_out, 4), dtype=torch.float64, device=dev)
    ocnt, wcnt = (torch.zeros((n, D), dtype=torch.int32, device=dev) for _ in range(2))
    ok = torch.zeros((n,), dtype=torch.int32, device=dev)
    info = {}

    def predict():
        rc, info["n_refused"] = opt.predict_scenes_raw(sb, t0.data_ptr(), span, api.PREDICT_CONSTANT_VELOCITY, 0.5, sample_dt,
                                                       out_samples, out.data_ptr(), ocnt.data_ptr(), ok.data_ptr())
        swb._chk(rc, "in cilqr_predict_scenes_batch")

    def window():
        rc, info["n_overflow"] = opt.window_scenes_raw(sb, t0.data_ptr(), span, window_out, win.data_ptr(), wcnt.data_ptr(), ok.data_ptr())
        swb._chk(rc, "in cilqr_window_scenes_batch")

    # alternating: window, predict, window, predict
    tw1, tp1 = swb._timed(window, samples, calls), swb._timed(predict, samples, calls)
    tw2, tp2 = swb._timed(window, samples, calls), swb._timed(predict, samples, calls)
    tp = min((tp1, tp2), key=lambda t: t["median_ms"])
    tw = min((tw1, tw2), key=lambda t: t["median_ms"])
    got_counts = ocnt.cpu().numpy()
    pick = np.linspace(0, n - 1, min(n, 16)).astype(int)
    same = True
    for b in pick:
        flat = dict(center=packed["center"], static_points=np.zeros((0, 2)), static_counts=np.zeros(0, np.int32),
                    dynamic_polygon_points=np.zeros((4 * D, 2)), dynamic_polygon_counts=np.full(D, 4, np.int32),
                    dynamic_trajectories=traj[b].cpu().numpy().reshape(-1, 4), dynamic_trajectory_counts=np.full(D, S, np.int32))
        rows, cnt, _ = api.predict_scene(flat, float(t0[b].item()), span, api.PREDICT_CONSTANT_VELOCITY, 0.5, sample_dt, out_samples)
        same = same and np.array_equal(cnt, got_counts[b]) and np.array_equal(rows.view(np.uint64), out[b].cpu().numpy().view(np.uint64))
    written = int(got_counts.clip(min=0).sum()) * 32
    return dict(scenes=n, dynamic=D, source_samples=S, sample_period_s=dt, span_s=span, sample_dt=sample_dt, out_samples=out_samples,
                window_out_samples=window_out, estimate=est, predict_call=tp, predict_calls_both_rounds=[tp1, tp2],
                window_call=tw, window_calls_both_rounds=[tw1, tw2], n_refused=info["n_refused"], n_overflow=info["n_overflow"],
                predicted_obstacles=int((got_counts > 0).sum()), bytes_written=written,
                bytes_written_per_s=written / (1e-3 * tp["median_ms"]), call_over_estimate=tp["median_ms"] / est["estimate_ms"],
                predict_over_window=tp["median_ms"] / tw["median_ms"], sampled_scenes_equal_host_call=bool(same))


def episodes(n, cycles, seconds, seed, workers):
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, workers=workers)
    sf = scene_io.from_generator(sc)
    S = int(round(seconds / 0.01)) + 1
    scenes = [dataclasses.replace(s, dynamic=[scene_io.DynamicObstacle(d.polygon, swb._recording(d.trajectory, S, 0.01)) for d in s.dynamic])
              for s in sf.scenes]
    packed = scene_io.pack_scene_batch(sf.center, scenes)
    start = np.ascontiguousarray(sc["start"], dtype=np.float64)
    n_drive = 6
    span = spec.n_steps * spec.dt
    dp_cfg = api.default_dp_config(tf=span, delta_t=spec.dt)
    rec = dict(scenes=n, cycles=cycles, n_drive=n_drive, recording_samples=S, carry=CARRY, max_age=0.5)
    with api.BatchIlqrOptimizer(n_steps=spec.n_steps, batch_capacity=n, cmax=spec.cmax, max_lane_segments=256) as opt:
        for name, prediction in (("recordings", None), ("hold", dict(mode=api.PREDICT_HOLD, max_age=0.5)),
                                 ("constant_velocity", dict(mode=api.PREDICT_CONSTANT_VELOCITY, max_age=0.5))):
            _note("episodes,", name)
            ep = episode.run_episode(opt, packed, start, cycles, n_drive, carry=CARRY, prediction=prediction)
            census = {k: 0 for k in ("kept", "not_asked", "refused", "off_start", "hit")}
            hit_truth = np.zeros(n, dtype=bool)
            per_cycle = []
            for c, cyc in enumerate(ep["cycles"]):
                truth = opt.window_scenes(packed, cyc["t0"], span)
                if not truth["window_ok"].all():
                    truth = dict(truth, dynamic_trajectory_counts=np.maximum(truth["dynamic_trajectory_counts"], 0))
                first = opt.check_collisions(truth, cyc["driven"], api.ROWS_TRAJ, dp_cfg, 0.0)["first_hit"]
                was_alive = ep["cycles"][c - 1]["alive"] if c else np.ones(n, dtype=bool)
                hits = (first != -1) & was_alive
                hit_truth |= hits
                entry = dict(alive=int(cyc["alive"].sum()), planned=int((cyc["outcome"] == api.PLAN_OK).sum()), driven_hit_truth=int(hits.sum()))
                if c:
                    src = np.bincount(cyc["source"], minlength=5)
                    for k, v in zip(census, src):
                        census[k] += int(v)
                    entry["source"] = [int(v) for v in src]
                per_cycle.append(entry)
            asked = sum(census.values()) - census["not_asked"]
            rec[name] = dict(source_census_later_cycles=census, share_hit_of_asked=(census["hit"] / asked if asked else None),
                             share_kept_of_asked=(census["kept"] / asked if asked else None),
                             scenes_whose_driven_rows_hit_the_recorded_scene=int(hit_truth.sum()), alive_at_end=int(ep["alive"].sum()),
                             per_cycle=per_cycle)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", type=int, default=65536)
    ap.add_argument("--dynamic", type=int, default=9)
    ap.add_argument("--source-samples", type=int, default=1501)
    ap.add_argument("--span", type=float, default=5.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4, help="back-to-back calls per sample")
    ap.add_argument("--episode-scenes", type=int, default=2048, help="scenes of the episodes of (b) (0: skip them)")
    ap.add_argument("--cycles", type=int, default=6)
    ap.add_argument("--recording-seconds", type=float, default=9.0)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_predict.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_bench: no GPU; nothing is measured without one")
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    sample_dt = 0.1
    out_samples = scene_io.predict_out_samples(sample_dt, a.span)
    rec = dict(tool="tools/predict_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), stream_bytes_per_s_assumed=swb.STREAM_BYTES_PER_S,
               dependent_miss_s_assumed=swb.MISS_S, calls_per_sample=a.calls)
    with api.BatchIlqrOptimizer(n_steps=50, batch_capacity=1, cmax=16) as opt:
        opt.set_stream(torch.cuda.current_stream().cuda_stream)
        for name, dt, window_out in (("rate_10ms", 0.01, 512), ("rate_100ms", 0.1, 64)):
            _note("the call,", name)
            rec[name] = call_at_scale(opt, a.scenes, a.dynamic, a.source_samples, dt, window_out, a.span, sample_dt, out_samples,
                                      a.seed, a.samples, a.calls)
            torch.cuda.empty_cache()
    if a.episode_scenes > 0:
        rec["episodes"] = episodes(a.episode_scenes, a.cycles, a.recording_seconds, a.seed, a.workers)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
