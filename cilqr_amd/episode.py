"""Closed-loop episodes over a batch of recorded scenes: plan, drive a little, plan again.

This module is glue over public calls of BatchIlqrOptimizer -- window_scenes (or predict_scenes), plan_scenes and track -- and
adds no rule of its own: what a cycle computes is what those three calls compute, made in this order.  Host arrays throughout; a caller who
keeps the batch on the device chains window_scenes_raw, plan_scenes_raw (warm=...) and track_raw the same way, and then
nothing but t0 and the start states cross to the device per cycle ("Planning cycle after cycle").
"""
from __future__ import annotations

import numpy as np

from . import api


def run_episode(opt: "api.BatchIlqrOptimizer", packed: dict, start4, n_cycles: int, n_drive: int = 6,
                out_samples: "int | None" = None, dp_cfg: "api.DpConfig | None" = None,
                corridor_cfg: "api.CorridorConfig | None" = None, carry: "dict | None" = None,
                prediction: "dict | None" = None) -> dict:
    """n_cycles planning cycles on the scenes of `packed` (scene_io.pack_scene_batch; recordings of any length, absolute
    times), all scenes starting at scene time 0 in start4 [B,4] = x y theta v.  Per cycle:

      window   opt.window_scenes(packed, t0, dp_cfg.tf, out_samples): every scene on the clock of its own t0;
      plan     opt.plan_scenes on the window, warm from the previous cycle's `traj` with shift = n_drive - 1 (the controls
               that were not driven yet); the first cycle is cold, and a scene whose previous outcome was not PLAN_OK gets
               shift = -1 (cold);
      track    opt.track(traj, ROWS_TRAJ, start6, n_drive): the n_drive rows the vehicle really drives, from the six-state
               start = the previous cycle's last driven row (first cycle: start4 with a = delta = 0);
      advance  the next start4 is x y theta v of the last driven row (the solver's knot 0 keeps a = delta = 0, as the
               warm-start contract says), and t0 advances by that row's time minus row 0's time.

    carry = dict(max_advance, max_start_offset, collision_buffer, refresh_every): from the second cycle on the plan step is
    opt.plan_scenes(..., carry=...) -- the previous cycle's `plan` rows (ROWS_PLAN) with the time driven since as `advance`,
    so the DP planner runs only where those rows do not hold (cilqr_plan_scenes_batch_carry).  advance is -1 (plan with the
    DP planner) where the previous outcome was not PLAN_OK or the scene is not alive, and for every scene in every
    refresh_every-th cycle (0 or absent: never).  Each such cycle's dict gains source [B] and n_kept; the first cycle has
    source = CARRY_NOT_ASKED for all.  carry = None: the loop as above.

    prediction = dict(mode, max_age, sample_dt=None, out_samples=None): the scene of a cycle is not the recording's window but
    opt.predict_scenes(packed, t0, dp_cfg.tf, mode, max_age, sample_dt, out_samples) -- what the samples observed by t0 alone
    say (include/cilqr.h, "scene prediction"); sample_dt defaults to dp_cfg.delta_t and out_samples to the smallest value the
    call accepts for dp_cfg.tf.  The run_episode argument out_samples is the window's and is not read then.  A refused scene
    is handled as a window overflow is (window_ok = predict_ok).  It composes with carry=.  prediction = None: the window.

    A scene whose tracker failed (ok = 0) or whose window overflowed keeps its start and its t0, and its `alive` flag is 0
    for the rest of the episode.  It is still carried through the calls -- after an overflow with the counts of the
    obstacles that did not fit set to 0, because HOST arrays with a negative count refuse the whole batch -- and its
    outputs mean nothing.

    Returns dict(cycles=[per cycle: the dict of plan_scenes, plus driven [B,n_drive,10], track_ok [B] int32, window_ok [B]
    bool, t0 [B] (the scene times the cycle planned at), alive [B] bool (after the cycle)], t0, start4, alive: the state
    after the last cycle)."""
    dp_cfg = dp_cfg or api.default_dp_config(tf=opt.N * opt.cfg.dt, delta_t=opt.cfg.dt)
    corridor_cfg = corridor_cfg or api.default_corridor_config()
    B = int(packed["batch"])
    start = np.array(start4, dtype=np.float64).reshape(B, 4)
    start6 = np.concatenate([start, np.zeros((B, 2))], axis=1)
    t0, alive = np.zeros(B), np.ones(B, dtype=bool)
    prev, cycles = None, []
    driven_time = np.zeros(B)
    for cycle in range(int(n_cycles)):
        if prediction is None:
            win = opt.window_scenes(packed, t0, float(dp_cfg.tf), out_samples)
            window_ok = win["window_ok"]
        else:
            sample_dt = prediction.get("sample_dt")
            win = opt.predict_scenes(packed, t0, float(dp_cfg.tf), prediction["mode"], prediction["max_age"],
                                     float(dp_cfg.delta_t) if sample_dt is None else sample_dt, prediction.get("out_samples"))
            window_ok = win["predict_ok"]
        if not window_ok.all():
            win = dict(win, dynamic_trajectory_counts=np.maximum(win["dynamic_trajectory_counts"], 0))
        warm = None
        if prev is not None:
            shift = np.where(prev["outcome"] == api.PLAN_OK, n_drive - 1, -1).astype(np.int32)
            warm = (prev["traj"], shift, api.ROWS_TRAJ)
        if carry is None:
            plan = opt.plan_scenes(win, start, dp_cfg, corridor_cfg, warm=warm)
        elif prev is None:
            plan = opt.plan_scenes(win, start, dp_cfg, corridor_cfg, warm=warm)
            plan.update(source=np.full(B, api.CARRY_NOT_ASKED, np.int32), n_kept=0)
        else:
            refresh = int(carry.get("refresh_every", 0))
            asked = (prev["outcome"] == api.PLAN_OK) & alive & (refresh <= 0 or cycle % refresh != 0)
            plan = opt.plan_scenes(win, start, dp_cfg, corridor_cfg, warm=warm, carry=dict(
                rows=prev["plan"], layout=api.ROWS_PLAN, advance=np.where(asked, driven_time, -1.0),
                max_advance=carry["max_advance"], max_start_offset=carry["max_start_offset"],
                collision_buffer=carry.get("collision_buffer", 0.0)))
        driven, track_ok = opt.track(plan["traj"], api.ROWS_TRAJ, start6, n_drive)
        alive = alive & window_ok & (track_ok != 0)
        cycles.append(dict(plan, driven=driven, track_ok=track_ok, window_ok=window_ok, t0=t0.copy(), alive=alive.copy()))
        last = driven[:, n_drive - 1]
        start6 = np.where(alive[:, None], last[:, 1:7], start6)
        start = np.ascontiguousarray(start6[:, :4])
        driven_time = last[:, 0] - driven[:, 0, 0]
        t0 = np.where(alive, t0 + driven_time, t0)
        prev = plan
    return dict(cycles=cycles, t0=t0, start4=start, alive=alive)
