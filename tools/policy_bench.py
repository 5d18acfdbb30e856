#!/usr/bin/env python3
"""The closed-loop policy of a solve (cilqr_policy_gains_batch, cilqr_policy_rollout_batch) at bench scale: the bench workload
(BASELINE configs[2]: 65536 mix11 problems, K = 51) is solved once with every array resident in HBM; the gains call then
linearises the returned trajectories where they lie (lambda = 1), and the rollout runs S = 1, 8, 32 starts per plan under
those gains -- all rows, the six rows of one 0.5 s cycle, and the summaries alone.

    python tools/policy_bench.py                          # 65536 mix11 problems
    python tools/policy_bench.py --problems 4096 --out /tmp/x.json

The device time is HIP events on the handle's stream around --burst back-to-back calls (an otherwise idle GPU, one warm-up
call per shape), divided by the burst; median, min and max over --calls such measurements.  Every call ends in the library's
wait for its stream: it is the call's time, not the bare kernel's.

THE ESTIMATES are made from counts and from figures this repository has on record, before anything is timed (estimate_*):
  * rollout: the larger of (a) the arithmetic -- k_forward's bulk launch, 139 us for 65536 rollouts of 50 steps (one
    wavefront per SIMD, so taken to scale with the chains: no credit for several waves sharing a SIMD) -- and (b) the bytes
    -- nominal rows and gains once per problem, the starts, the rows and summaries written -- at the 4.41 TB/s of the resample
    kernel (profiles/r11_resample.json);
  * gains: the parts of the stage chain -- the load kernels as recorded per solve (profiles/r06_kernel_rooflines.json:
    k_load_corridor 0.654 + k_load_goals 0.113 ms; the lane grid is cached from the solve), the rows in and the three tensors
    out at 4.41 TB/s, k_backward's full-batch launch 0.233 ms (README), and 1.0 ms for ONE full-batch quadratisation (a guess:
    the record has 7.12 ms per solve over launches on shrinking sets), plus 5 waits of 20 us.
Beside every rollout figure: a device-to-device copy of the output's byte count alone, timed the same way in the same run.

The census is descriptive and asserts nothing: every plan started --offset metres to the left of its first pose, under its
gains (closed loop) and under Kfb = 0 (open loop: the nominal controls replayed) -- the share of plans whose closed-loop end
deviation is below the open-loop one; and the share of trajectories the collision audit (buffer 0) calls hit, for the nominal
plans and for the perturbed closed-loop rollouts.  One JSON line is printed and written to --out (default
profiles/r19_policy.json).
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

from cilqr_amd import api, scenario, scene_io  # noqa: E402

STREAM_BYTES_PER_S = 4.41e12          # profiles/r11_resample.json, shared_axis_5x.bytes_per_s
FORWARD_US_PER_65536x50 = 139.0       # k_forward's bulk launch (cilqr_amd/csrc/dev_model.hpp, closed_loop_step)
USUAL_SPREAD = 1.3


def _spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), measurements=len(a))


def _chk(rc, what):
    if rc != api.OK:
        raise api.CilqrError(rc, what)


def estimate_rollout(B, K, F, S, n_out, with_rows):
    steps = n_out - 1
    read = B * n_out * F * 8 + B * steps * 14 * 8 + S * B * 48
    written = (S * B * n_out * 80 if with_rows else 0) + S * B * 20
    arith_ms = 1e-3 * FORWARD_US_PER_65536x50 * (S * B / 65536.0) * (steps / 50.0)
    memory_ms = 1e3 * (read + written) / STREAM_BYTES_PER_S
    return dict(bytes_read=read, bytes_written=written, arithmetic_ms=arith_ms, memory_ms=memory_ms, estimated_ms=max(arith_ms, memory_ms))


def estimate_gains(B, K, F):
    N = K - 1
    scale = B / 65536.0
    moved = B * K * F * 8 + B * (K * 48 + N * 16) + 2 * B * N * 14 * 8 + 2 * B * 16
    parts = dict(load_ms=(0.654 + 0.113) * scale, rows_and_tensors_ms=1e3 * moved / STREAM_BYTES_PER_S, quadratize_ms=1.0 * scale,
                 backward_ms=0.233 * scale, waits_ms=0.1)
    return dict(bytes_moved_outside_the_three_kernels=moved, parts=parts, estimated_ms=float(sum(parts.values())))


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


def run(n, seed, calls, burst, workers, offset, samples, lds_variants):
    spec = scenario.SPECS["mix11"]
    sc = scenario.generate(spec, n, seed=seed, scenarios=True, workers=workers)
    K, cmax, F = sc["n_steps"] + 1, sc["cmax"], api.ROWS_FIELDS[api.ROWS_TRAJ]
    N = K - 1
    nl, nr = len(sc["left"]), len(sc["right"])
    cfg = api.default_config(sc["n_steps"])
    rec = dict(family="mix11", problems=n, knots=K, layout="CILQR_ROWS_TRAJ", gains_lambda=1.0, stream_bytes_per_s_assumed=STREAM_BYTES_PER_S,
               forward_us_per_65536x50_assumed=FORWARD_US_PER_65536x50)
    shapes = [(S, n_out, rows) for S in samples for (n_out, rows) in ((K, True), (6, True), (K, False))]
    est_gains = estimate_gains(n, K, F)                                                         # before anything runs
    est = {s: estimate_rollout(n, K, F, s[0], s[1], s[2]) for s in shapes}
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

        # ---- the gains call
        Kfb, kff, dV, ok = z(n, N, 2, 6), z(n, N, 2), z(n, 2), z(n, dt=torch.int32)
        lam = torch.ones(n, dtype=torch.float64, device=dev)

        def gains_call():
            _chk(opt.policy_gains_raw(prob, api.ROWS_TRAJ, traj.data_ptr(), lam.data_ptr(), Kfb.data_ptr(), kff.data_ptr(), dV.data_ptr(),
                                      ok.data_ptr()), "in cilqr_policy_gains_batch")
        g = timed(gains_call, calls, max(1, burst // 4))
        rec["gains"] = dict(call=g, estimate=dict(est_gains, **_verdict(g["median_ms"], est_gains["estimated_ms"])),
                            ok=int(ok.sum().item()), finite_problems=int(torch.isfinite(Kfb).all(dim=(1, 2, 3)).sum().item()))

        # ---- the rollouts: starts = the plans' own first states moved by fractions of --offset to the left of the heading
        S_max = max(samples)
        th = traj[:, 0, 3]
        side = torch.stack([-torch.sin(th), torch.cos(th)], dim=1)                              # [n, 2]
        frac = torch.linspace(-1.0, 1.0, S_max, dtype=torch.float64, device=dev) if S_max > 1 else torch.ones(1, dtype=torch.float64, device=dev)
        start = traj[None, :, 0, 1:7].repeat(S_max, 1, 1)
        start[:, :, 0:2] += offset * frac[:, None, None] * side[None]
        start = start.contiguous()
        out = z(S_max, n, K, 10)
        twin = torch.empty_like(out)
        mx, en, nc = z(S_max, n), z(S_max, n), z(S_max, n, dt=torch.int32)
        rec["rollout"] = {}
        for lds_kb, shape in [(None, s) for s in shapes] + [(kb, s) for kb in lds_variants for s in shapes if s[2] and s[1] == K]:
            S, n_out, with_rows = shape
            if lds_kb is None:
                os.environ.pop("CILQR_POLICY_LDS_KB", None)
            else:
                os.environ["CILQR_POLICY_LDS_KB"] = str(lds_kb)     # the tuning hook of kernels_policy.hip: same rows, another chunk

            def call():
                _chk(opt.policy_rollout_raw(n, api.ROWS_TRAJ, traj.data_ptr(), K, Kfb.data_ptr(), None, 0.0, S, start.data_ptr(), False,
                                            n_out, out.data_ptr() if with_rows else None, mx.data_ptr(), en.data_ptr(), nc.data_ptr(),
                                            api.MEM_DEVICE), "in cilqr_policy_rollout_batch")
            c = timed(call, calls, burst)
            e = est[shape]
            r = dict(samples_per_plan=S, n_out=n_out, rows_written=with_rows, burst=burst, call=c,
                     estimate=dict(e, **_verdict(c["median_ms"], e["estimated_ms"])),
                     rollouts_per_s=S * n / (1e-3 * c["median_ms"]), bytes_per_s=(e["bytes_read"] + e["bytes_written"]) / (1e-3 * c["median_ms"]))
            if lds_kb is not None:
                rec.setdefault("lds_kb_variants", {})[f"S{S}_rows_{n_out}_lds{lds_kb}"] = dict(call=c, over_default=c["median_ms"] / rec["rollout"][f"S{S}_rows_{n_out}"]["call"]["median_ms"])
                continue
            if with_rows:
                nbytes = S * n * n_out * 80
                src, dst = out.view(-1)[:nbytes // 8], twin.view(-1)[:nbytes // 8]

                def copy():
                    dst.copy_(src, non_blocking=True)       # hipMemcpyAsync device to device, the output's byte count
                    torch.cuda.current_stream().synchronize()
                m = timed(copy, calls, burst)
                r["memcpy_d2d_of_output"] = dict(bytes=nbytes, **m)
                r["call_over_memcpy"] = c["median_ms"] / m["median_ms"]
            rec["rollout"][f"S{S}_{'rows' if with_rows else 'summaries'}_{n_out}"] = r

        os.environ.pop("CILQR_POLICY_LDS_KB", None)
        # ---- census (descriptive): one start per plan, --offset to the left
        one = traj[None, :, 0, 1:7].clone()
        one[0, :, 0:2] += offset * side
        one = one.contiguous()
        closed_rows, zero_K = z(1, n, K, 10), torch.zeros_like(Kfb)
        c_end, o_end, c_max, o_max = z(1, n), z(1, n), z(1, n), z(1, n)
        _chk(opt.policy_rollout_raw(n, api.ROWS_TRAJ, traj.data_ptr(), K, Kfb.data_ptr(), None, 0.0, 1, one.data_ptr(), True, K,
                                    closed_rows.data_ptr(), c_max.data_ptr(), c_end.data_ptr(), nc.data_ptr(), api.MEM_DEVICE), "closed loop")
        clamped = int((nc[0] > 0).sum().item())
        _chk(opt.policy_rollout_raw(n, api.ROWS_TRAJ, traj.data_ptr(), K, zero_K.data_ptr(), None, 0.0, 1, one.data_ptr(), True, K,
                                    None, o_max.data_ptr(), o_end.data_ptr(), None, api.MEM_DEVICE), "open loop")
        torch.cuda.synchronize()
        fin = torch.isfinite(c_end[0]) & torch.isfinite(o_end[0])
        census = dict(lateral_offset_m=offset, clamp=True, plans=n, finite_both=int(fin.sum().item()),
                      closed_end_below_open_end=int(((c_end[0] < o_end[0]) & fin).sum().item()),
                      closed_end_below_offset=int(((c_end[0] < offset) & fin).sum().item()),
                      median_end_dev_closed=float(c_end[0][fin].median().item()), median_end_dev_open=float(o_end[0][fin].median().item()),
                      plans_with_a_clamped_step=clamped)
        sf = scene_io.from_generator(sc)
        packed = scene_io.pack_scene_batch(sf.center, list(sf.scenes))
        ts = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(dev) for k in api._SCENE_BATCH_ARRAYS}
        sb = api.scene_batch_struct(packed, api.MEM_DEVICE, **{k: ts[k].data_ptr() for k in api._SCENE_BATCH_ARRAYS})
        dp_cfg = api.default_dp_config(tf=N * cfg.dt, delta_t=cfg.dt)
        mask, first, n_hit = z(n, K, dt=torch.uint8), z(n, dt=torch.int32), z(n, dt=torch.int32)
        for name, rows in (("nominal", traj), ("perturbed_closed_loop", closed_rows)):
            rc, hit = opt.check_collisions_raw(dp_cfg, sb, api.ROWS_TRAJ, rows.data_ptr(), K, 0.0, mask.data_ptr(), first.data_ptr(),
                                               n_hit.data_ptr())
            _chk(rc, "in cilqr_check_collisions_batch")
            census[f"audit_hit_{name}"] = int(hit)
        rec["census"] = census
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=65536)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 8, 32], help="starts per plan")
    ap.add_argument("--lds-kb", type=int, nargs="*", default=[], help="also time the all-rows shapes with this much LDS planned per workgroup (CILQR_POLICY_LDS_KB)")
    ap.add_argument("--calls", type=int, default=5, help="measurements per shape")
    ap.add_argument("--burst", type=int, default=8, help="back-to-back calls per measurement")
    ap.add_argument("--offset", type=float, default=0.3, help="lateral offset of the census starts, metres")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--seed", type=int, default=19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_policy.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_bench: no GPU; nothing is measured without one")
    L = api.lib()
    L.cilqr_build_id.restype = C.c_char_p
    rec = dict(tool="tools/policy_bench.py", device=torch.cuda.get_device_name(0), abi=L.cilqr_abi_version(),
               build_id=L.cilqr_build_id().decode(), **run(a.problems, a.seed, a.calls, a.burst, a.workers, a.offset, a.samples, a.lds_kb))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
