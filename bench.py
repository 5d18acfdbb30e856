#!/usr/bin/env python
"""bench.py -- CILQR solves/sec on MI355X (BASELINE.json metric).

One "step" = one solve of the whole per-GPU batch through the C-ABI (inputs already resident in HBM):
load/prepare -> init guess -> lockstep iLQR iterations until every problem terminated -> export.
Workload (config.workload): BASELINE.json configs[2] -- batch 65536 per GPU, 50-step horizon,
6 pedestrians + 3 moving + 2 static vehicles ("mix11" scenes of cilqr_amd.scenario).  With
--gpus N every rank solves its own 65536 scenes (weak scaling, configs[3] at N=8) and the
results are gathered to rank 0 with one RCCL gather per step inside the timed region.

The K timed steps go round-robin through a pool of `--pipeline` = 2 solver handles (cilqr_pool_*), each with two solves in flight
(cilqr_submit / cilqr_wait, `--in-flight 2`): a handle iterates the bulk of one step in its main arena while
the last <= 8192 problems of its previous step -- the latency-bound part of a solve -- finish in its small
finishing arena on a second stream (include/cilqr.h, CILQR_OPT_FINISH_THRESHOLD); and the first stages of
the handles, which drift apart by themselves, fill each other's gaps (a backward pass or a rollout is
one lane per problem: a chain of N dependent steps that leaves most of the chip idle once the active set has
shrunk, exactly where another handle's cost kernels fit).  Every step is a complete, independent solve of
the batch; `value` = problems solved / wall time of the K steps.

A plain run (`--gpus N --steps K --warmup W`) does only what `value` needs: it generates the scenes, sets up the pool,
warms up, times the K steps, writes the last timed step's results when `--dump-outputs DIR` is given, and prints the
line; every figure below that is not `value`, `ms_per_step` or the per-rank / host records of the timed region is null
there.  `--full` adds everything else, each after the timed region: the calibration solve with HIP events around every
phase (`breakdown_ms_per_step`, `roofline`), `one_handle` (the same steps through one handle, half the memory),
`single_batch` (the strictly sequential call), the check that every solve in flight returned the same bits, the two
extra legs, the C-ABI gather comparison of a multi-rank run, the drop-in latency section and the CPU baseline.

`--dump-outputs DIR` (rank 0): DIR/<name>.npy, float64, of a fixed, seeded sample of the problems of the last timed step
(at most 48 MiB in all): traj [n][K][10], cost_hist [n][max_iter+1][5] (rows >= n_cost zeroed: the library leaves them
untouched in device memory), n_cost, status, n_iter [n], and problem_index [n], the sampled problems' rows in the batch.
The inputs depend on the arguments only (cilqr_amd.scenario: one RNG stream per problem), so two builds can be compared
output for output.

Under `--full`, two extra legs on rank 0 at N = 1 (never `value`; `--no-extras` skips them): `pcie_inclusive` -- the same stream of batches with
every input and output array in pageable HOST memory (CILQR_MEM_HOST through the pool: the library uploads the queued solve's
arrays beside the solves and downloads the results ragged), compared bit for bit with the device-resident result -- and
`end_to_end` -- obstacle points in HBM -> cilqr_build_corridors on a handle and stream of its own -> cilqr_pool_submit.
Multi-rank runs carry `per_rank`, `host.cores_busy_per_rank` and `gather_verified_ranks` (a checksum check of what rank 0
gathered); `--gather c_abi` lets cilqr_gather_results carry the per-step gather instead of torch.distributed.

Prints ONE JSON line on rank 0 (contract in the task statement); with `--full` it fills two extra objects:
  roofline     backward-pass kernel, every launch of the timed region (time-weighted) and the launches
               that cover the whole batch: algorithmic bytes ((N*110+44)*8 B per problem
               per launch) / HIP-event time, against the 8 TB/s HBM peak; `achieved` and `frac` are quoted on the
               HBM bytes the kernel really moves (PMC-counted per problem-step), which is
               <= 1 by construction; `achieved_algorithmic` / `frac_algorithmic` on the dense figure
  cpu_baseline the CPU oracle (single thread) on a bounded sample of the same scenes, plus
               mean / median / p95 per solve for each BASELINE config's scene family
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {("ped6", 4096): "configs[1]", ("mix11", 65536): "configs[2] (configs[3] when sharded over 8 GPUs)",
             ("dyn20", 65536): "configs[4]", ("dyn20x", 65536): "configs[4] (barriers active at the init guess)"}
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def cpu_quota_cores():
    """Cores' worth of CPU time this process tree may use: the cgroup's quota when there is one (the GPU boxes show 256
    logical CPUs and grant 16), else None."""
    try:
        q_, p_ = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q_ == "max" else max(0.01, int(q_) / int(p_))
    except Exception:   # noqa: BLE001
        return None


def scene_workers(world):
    """Worker processes for the scene generator of ONE rank: every rank generates at the same time, so the cores are shared
    out -- the quota's, not the logical CPUs' (256 workers under a 16-core quota only queue up)."""
    quota = cpu_quota_cores()
    cores = min(os.cpu_count() or 8, int(quota)) if quota else (os.cpu_count() or 8)
    return max(1, min(32, cores // max(1, world)))


def native_thread_count():
    try:
        for line in open("/proc/self/status"):
            if line.startswith("Threads:"):
                return int(line.split()[1])
    except Exception:   # noqa: BLE001
        pass
    return None


def thread_cpu_seconds():
    """{tid: (name, user + system CPU seconds)} of every native thread of this process (/proc/self/task/*/stat)."""
    out = {}
    try:
        tick = os.sysconf("SC_CLK_TCK")
        for tid in os.listdir("/proc/self/task"):
            try:
                raw = open(f"/proc/self/task/{tid}/stat").read()
            except OSError:
                continue
            name = raw[raw.index("(") + 1:raw.rindex(")")]
            f = raw[raw.rindex(")") + 2:].split()
            out[int(tid)] = (name, (int(f[11]) + int(f[12])) / tick)      # utime, stime
    except Exception:   # noqa: BLE001
        pass
    return out


def cpu_seconds():
    """user + system CPU seconds of this process, all threads (RUSAGE_SELF)."""
    import resource
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=65536, help="problems per GPU")
    ap.add_argument("--scene", default="mix11")
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure, after the timed region: calibration solve and "
                         "per-phase breakdown, roofline (with the rocprofv3 traffic passes), one_handle, single_batch, the identical-results "
                         "check, the extra legs, the C-ABI gather comparison, the latency section and the CPU baseline (the --no-* "
                         "options and --cpu-sample / --cpu-configs below select among them); off: only what `value` needs")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write a fixed, seeded sample of the last timed step's results to DIR/<name>.npy "
                         "(float64, at most 48 MiB in all; rank 0)")
    ap.add_argument("--cpu-sample", type=int, default=3072, help="problems timed on the CPU oracle (0 = skip); 3072 scenes = about 15 s on one core")
    ap.add_argument("--cpu-configs", type=int, default=256, help="scenes per BASELINE config for the per-solve CPU statistics (0 = skip)")
    ap.add_argument("--no-profile", action="store_true", help="do not record per-kernel HIP events")
    ap.add_argument("--compact-percent", type=int, default=-1, help="CILQR_OPT_COMPACTION value (tuning experiments)")
    ap.add_argument("--spec-threshold", type=int, default=-1, help="CILQR_OPT_SPEC_THRESHOLD value (tuning experiments)")
    ap.add_argument("--seq-rounds", type=int, default=-1, help="CILQR_OPT_SEQ_ROUNDS value (tuning experiments)")
    ap.add_argument("--team-threshold", type=int, default=-1, help="CILQR_OPT_TEAM_THRESHOLD value (tuning experiments)")
    ap.add_argument("--round-group", type=int, default=-1, help="CILQR_OPT_ROUND_GROUP value (tuning experiments)")
    ap.add_argument("--wave-threshold", type=int, default=-1, help="CILQR_OPT_WAVE_THRESHOLD value (tuning experiments)")
    ap.add_argument("--tail-threshold", type=int, default=-1, help="CILQR_OPT_TAIL_THRESHOLD value (tuning experiments; 0 = lockstep to the end)")
    ap.add_argument("--pipeline", type=int, default=2,
                    help="solver handles used round-robin in the timed region (each with its own arenas, streams and host threads): "
                         "the latency-bound launches of one handle's first stage run in the gaps of the others'; 1 = one handle "
                         "(also reported as `one_handle` when more are used)")
    ap.add_argument("--torch-streams", action="store_true",
                    help="give every handle a torch.cuda.Stream instead of the stream it created itself")
    ap.add_argument("--stagger-ms", type=float, default=0.0,
                    help="pause between the first submissions to the handles of an empty pool (inside the timed region): starts "
                         "their first stages out of phase with each other")
    ap.add_argument("--in-flight", type=int, default=2, choices=[1, 2, 3],
                    help="solves in flight per handle (cilqr_submit / cilqr_wait): 2 = the stragglers of one solve finish in the "
                         "handle's finishing arena while the next solve is iterated in its main arena; 1 = one after the other")
    ap.add_argument("--fast-lane-ties", action="store_true",
                    help="CILQR_OPT_EXACT_LANE_TIES = 0: nearest lane segments by squared distances alone (the opt-in fast rule; the "
                         "default is the reference's tie rule, ilqr_optimizer.cc:605-618)")
    ap.add_argument("--finish-threshold", type=int, default=-1, help="CILQR_OPT_FINISH_THRESHOLD value (tuning experiments)")
    ap.add_argument("--coarse", default="generator", choices=["generator", "dp"],
                    help="where the coarse trajectories come from: the generator's smooth best-clearance pick, or the DP coarse "
                         "planner (cilqr_dp_plan: the reference's own producer, kinked paths) with corridors built from the "
                         "obstacle points by cilqr_build_corridors; 512 distinct scenes tiled to the batch")
    ap.add_argument("--gather", default="torch", choices=["torch", "c_abi"],
                    help="what carries the per-step results gather of a multi-rank run inside the timed region: torch.distributed's "
                         "gather (RCCL) or cilqr_gather_results (the library's own grouped ncclSend / ncclRecv, no PyTorch in the "
                         "exchange); the other one is run once after the timed region and compared with it")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the two extra legs (never `value`): pcie_inclusive = the same stream of batches with every array in HOST "
                         "memory, end_to_end = obstacle points -> cilqr_build_corridors -> solve, both through the pool")
    ap.add_argument("--extra-steps", type=int, default=0, help="timed steps of each extra leg (0 = min(--steps, 24))")
    ap.add_argument("--traffic-file", default=os.path.join(ROOT, "profiles", "backward_traffic.json"))
    ap.add_argument("--no-traffic", action="store_true",
                    help="do not measure the backward kernels' HBM traffic (two rocprofv3 --pmc passes over a one-step run of this "
                         "script, about 25 s); roofline.traffic is then null and roofline.frac uses the bytes recorded under profiles/")
    ap.add_argument("--no-latency", action="store_true",
                    help="skip the drop-in latency section (planning::IlqrOptimizer::Plan with a batch of one, C++ program under tests/cpp)")
    ap.add_argument("--latency-scenes", type=int, default=256, help="scenes per family for the latency section")
    ap.add_argument("--multi", action="store_true",
                    help="ONE process drives the N GPUs of --gpus (the reference's caller is one process, planning_node.cc:9-31): "
                         "a thread per GPU with its own pool of handles and device-resident inputs, no process group, no RCCL; "
                         "results reach GPU 0 by peer copies over xGMI.  The second path next to one process per GPU")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch plumbing only, on CPU: the ranks rendezvous over gloo, exchange made-up results through the same "
                         "gather and rank 0 prints a line with \"dry_run\": true and no value (tests/test_host.py)")
    return ap.parse_args(argv)


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks here (one process per GPU, the environment
    torch.distributed.run would have set), pass rank 0's JSON line through, fail if any rank fails."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), CILQR_BENCH_SPAWNED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = []
    for r in range(args.gpus):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=e,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr.fileno()))
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()               # rank 0's pipe is drained while it runs
    failed = None
    pending = set(range(args.gpus))
    while pending and failed is None:
        for r in sorted(pending):
            rc = procs[r].poll()
            if rc is None:
                continue
            pending.discard(r)
            if rc != 0:
                failed = (r, rc)
        time.sleep(0.1)
    for p in procs:   # a failed rank leaves the others inside a collective: end exactly the processes started here
        if p.poll() is None:
            p.kill()
        p.wait()
    reader.join(30.0)
    out0 = b"".join(c for c in chunks if c)
    if failed is not None:
        sys.stderr.write(f"bench.py: rank {failed[0]} exited with code {failed[1]}\n")
        raise SystemExit(1)
    lines = [ln for ln in out0.decode().splitlines() if ln.strip()]
    if len(lines) != 1:
        sys.stderr.write(f"bench.py: expected one JSON line from rank 0, got {len(lines)}\n")
        raise SystemExit(1)
    rec = json.loads(lines[0])
    if rec.get("n_gpus") != args.gpus:
        sys.stderr.write(f"bench.py: asked for {args.gpus} GPUs, the line reports {rec.get('n_gpus')}\n")
        raise SystemExit(1)
    sys.stdout.write(lines[0] + "\n")
    sys.stdout.flush()


def measure_backward_traffic(args, problem_steps_per_solve):
    """HBM bytes the backward kernels move, from the PMC counters, as MI355X_MICROARCH.md prescribes: FETCH_SIZE and
    WRITE_SIZE in SEPARATE rocprofv3 --pmc passes (counters only, no trace), each over a one-step, one-batch-in-flight run
    of this script on the same workload; both in KiB; FETCH_SIZE x 2 on gfx950 (it tallies 64 B per 128 B request of the
    16 B/lane coalesced loads).  Returns HBM bytes per problem-step over all backward launches of the capture, or None."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None
    tmp = tempfile.mkdtemp(prefix="cilqr_pmc_", dir="/tmp")
    try:
        sums = {}
        full = {}
        solves = None
        for c in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, c)
            cmd = ["rocprofv3", "--pmc", c, "-d", d, "--", sys.executable, os.path.abspath(__file__), "--full", "--steps", "1", "--warmup", "0",
                   "--in-flight", "1", "--pipeline", "1", "--cpu-sample", "0", "--no-latency", "--no-traffic", "--no-extras", "--batch", str(args.batch),
                   "--scene", args.scene, "--seed", str(args.seed), "--coarse", args.coarse]
            for flag, val in (("--compact-percent", args.compact_percent), ("--team-threshold", args.team_threshold),
                              ("--wave-threshold", args.wave_threshold), ("--tail-threshold", args.tail_threshold)):
                if val >= 0:      # what decides which backward kernel runs on which slots
                    cmd += [flag, str(val)]
            if args.fast_lane_ties:
                cmd.append("--fast-lane-ties")
            env = dict(os.environ, TMPDIR="/tmp")
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
                env.pop(k, None)
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
            dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                return None
            con = sqlite3.connect(dbs[0])
            cols = [x[1] for x in con.execute("pragma table_info(counters_collection)")]
            kcol = "kernel_name" if "kernel_name" in cols else "name"
            sums[c] = con.execute(f"select sum(value) from counters_collection where {kcol} like '%k_backward%' and counter_name = ?", (c,)).fetchone()[0]
            # the launch over the whole batch: the first backward dispatch of a solve (largest grid, fewest bytes among those)
            gcol = "grid_size_x" if "grid_size_x" in cols else ("grid_size" if "grid_size" in cols else None)
            if gcol:
                # (the lane-per-problem kernel only: a wavefront-per-problem launch of 3072 problems has three times the
                # work-items of the launch over 65536 problems)
                per = con.execute(f"select sum(value), max({gcol}) from counters_collection where {kcol} like '%k_backward(%' and "
                                  f"counter_name = ? group by dispatch_id", (c,)).fetchall()
                gmax = max(p[1] for p in per)
                full[c] = min(p[0] for p in per if p[1] == gmax)
            n = con.execute(f"select count(distinct dispatch_id) from counters_collection where {kcol} like '%k_load_goals%'").fetchone()[0]
            solves = n if solves is None else min(solves, n)
            con.close()
        if not solves or not sums.get("FETCH_SIZE") or not sums.get("WRITE_SIZE"):
            return None
        hbm = sums["FETCH_SIZE"] * 1024.0 * 2.0 + sums["WRITE_SIZE"] * 1024.0
        return {"hbm_bytes_per_problem_step": hbm / (solves * problem_steps_per_solve), "solves_in_capture": int(solves),
                "fetch_size_kib": sums["FETCH_SIZE"], "write_size_kib": sums["WRITE_SIZE"],
                "full_batch_launch_hbm_bytes": (full["FETCH_SIZE"] * 2048.0 + full["WRITE_SIZE"] * 1024.0) if len(full) == 2 else None,
                "method": "rocprofv3 --pmc FETCH_SIZE and, separately, --pmc WRITE_SIZE over `bench.py --full --steps 1 --warmup 0 --in-flight 1` "
                          "of this workload; KiB; FETCH_SIZE x 2 (gfx950: 64 B tallied per 128 B request); k_backward + k_backward_team + "
                          "k_backward_wave dispatches"}
    except Exception:   # noqa: BLE001
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def plan_latency(scenario, families, n_scenes, seed, workers, batch=64):
    """Extra (never `value`): latency of the drop-in call.  tests/cpp/latency_bench.cc drives planning::IlqrOptimizer::Plan
    (include/cilqr/ilqr_optimizer.hpp: batch of ONE, the reference's containers in and out) and cilqr_solve_batch with
    `batch` scenes of host arrays, one call at a time, timed per call with steady_clock (ilqr_optimizer.cc:82-94)."""
    import shutil
    import subprocess
    import tempfile
    from cilqr_amd import api
    tmp = tempfile.mkdtemp(prefix="cilqr_latency_")
    out = {}
    try:
        exe = os.path.join(tmp, "latency_bench")
        lib_dir = os.path.dirname(api.LIB_PATH)
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "latency_bench.cc"), "-o", exe, "-L" + lib_dir, "-lcilqr_hip",
                               "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"], stdout=sys.stderr, stderr=sys.stderr)
        for fam in families:
            sc = scenario.generate(fam, n_scenes, seed=seed, workers=workers)
            K, cmax = sc["n_steps"] + 1, sc["cmax"]
            path = os.path.join(tmp, fam + ".bin")
            with open(path, "wb") as f:
                np.array([n_scenes, K, cmax, sc["left"].shape[0], sc["right"].shape[0]], np.int32).tofile(f)
                np.ascontiguousarray(sc["left"], np.float64).tofile(f)
                np.ascontiguousarray(sc["right"], np.float64).tofile(f)
                for b in range(n_scenes):
                    np.ascontiguousarray(sc["start"][b], np.float64).tofile(f)
                    np.ascontiguousarray(sc["coarse"][b], np.float64).tofile(f)
                    np.ascontiguousarray(sc["ccount"][b], np.int32).tofile(f)
                    np.ascontiguousarray(sc["corridor"][b], np.float64).tofile(f)
            r = subprocess.run([exe, path, str(batch)], stdout=subprocess.PIPE, stderr=sys.stderr, timeout=600)
            if r.returncode != 0:
                out[fam] = {"error": f"latency_bench exited with {r.returncode}"}
                continue
            out[fam] = json.loads(r.stdout.decode().strip().splitlines()[-1])
            out[fam]["_scene"] = sc
    except Exception as e:   # noqa: BLE001
        out["error"] = repr(e)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def dry_run(args, rank, world):
    """Launch plumbing without a GPU (see --dry-run): the rendezvous, the rank census and the per-step results gather of the
    timed region -- the SAME GatherThread (cilqr_amd/distributed.py), fed `steps` made-up results per rank through recycled
    slots -- over gloo.  Values encode (step, rank, problem); every problem has its own number of live Cost rows, so the
    ragged part of the payload is exercised too.  Rank 0 checks every gathered step: rank r's block sits at offset r * B, in
    problem order; steps arrive in the order they were put; the ragged rows unpack to the right problems."""
    import torch
    import torch.distributed as dist
    from cilqr_amd.distributed import GatherThread
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    one = torch.ones(1, dtype=torch.int32)
    if world > 1:
        dist.all_reduce(one)
    ranks = int(one.item())
    B, K, M = min(args.batch, 16), 6, 8
    steps = max(1, min(args.steps, 6))
    checks = {"rank_order": True, "step_order": True, "ragged_rows": True, "kappa_rebuilt": True}
    seen = []

    def make(step, slot):
        pid = (rank * B + torch.arange(B, dtype=torch.float64))                 # global problem index
        slot["traj"][:] = (1000.0 * step + pid)[:, None, None]
        slot["traj"][:, :, 6] = 0.01 * (1 + rank)                                 # delta: kappa = tan(delta) / L is rebuilt on the root
        slot["nc"][:] = (1 + (torch.arange(B) + rank + step) % M).to(torch.int32)  # live Cost rows: differ by problem, rank and step
        slot["hist"][:] = -1.0
        for b in range(B):
            n = int(slot["nc"][b])
            slot["hist"][b, :n, :] = (1000.0 * step + pid[b] + 0.001 * torch.arange(n, dtype=torch.float64))[:, None]
        slot["st"][:] = 1 + (rank + step) % 5

    def check(step, g):
        n = world * B
        want = 1000.0 * step + torch.arange(n, dtype=torch.float64)
        checks["rank_order"] &= bool(torch.equal(g["traj"][:, 0, 1], want))       # column 1 (x) travels as it is
        checks["kappa_rebuilt"] &= bool(torch.allclose(g["traj"][:, :, 7], torch.tan(g["traj"][:, :, 6]) / 1.0, rtol=0, atol=0)
                                        and torch.equal(g["traj"][:, 1, 0], torch.full((n,), 0.1, dtype=torch.float64)))
        nc = g["n_cost"].to(torch.int64)
        r_ = torch.arange(n)
        checks["ragged_rows"] &= bool(torch.equal(nc, 1 + (r_ % B + r_ // B + step) % M))
        first = torch.cumsum(nc, 0) - nc
        checks["ragged_rows"] &= bool(torch.equal(g["hist_rows"][first, 0], want) and g["hist_rows"].shape[0] == int(nc.sum())
                                      and torch.equal(g["hist_rows"][first + nc - 1, 0], want + 0.001 * (nc - 1).to(torch.float64)))
        checks["ragged_rows"] &= bool(torch.equal(g["status"], (1 + (r_ // B + step) % 5).to(g["status"].dtype)))

    free = [dict(traj=torch.zeros((B, K, 10), dtype=torch.float64), hist=torch.zeros((B, M + 1, 5), dtype=torch.float64),
                 nc=torch.zeros(B, dtype=torch.int32), st=torch.zeros(B, dtype=torch.int32)) for _ in range(2)]
    import threading
    cv = threading.Condition()
    gt = None

    def done(tag):
        step, slot = tag
        if rank == 0 and gt.last_tag is tag and gt.last is not None:
            seen.append(step)
            check(step, gt.last)
        with cv:
            free.append(slot)
            cv.notify_all()

    if world > 1:
        gt = GatherThread(device=None, dst=0, derive=(0.1, 1.0), on_done=done)
        for step in range(steps):
            with cv:
                while not free:
                    cv.wait(60.0)
                slot = free.pop(0)
            make(step, slot)
            gt.put((step, slot), slot["traj"], slot["hist"], slot["nc"], slot["st"])
        gt.drain()
        gt.close()
        checks["step_order"] = (seen == list(range(steps))) if rank == 0 else True
        dist.barrier()
        dist.destroy_process_group()
    if ranks != world:
        raise SystemExit(f"bench.py: {ranks} ranks answered the all-reduce, WORLD_SIZE is {world}")
    if rank == 0:
        ok = all(checks.values()) if world > 1 else None
        return {"metric": "CILQR solves/sec (dry run: launch plumbing only, nothing solved)", "value": None, "unit": "solves/s",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "dry_run": True, "ranks_reporting": ranks,
                "gather_in_rank_order": (checks["rank_order"] if world > 1 else None), "gathers": len(seen),
                "gathers_in_step_order": (checks["step_order"] if world > 1 else None),
                "ragged_history_rows_ok": (checks["ragged_rows"] if world > 1 else None),
                "time_and_kappa_rebuilt_on_root": (checks["kappa_rebuilt"] if world > 1 else None), "gather_checks_ok": ok,
                "mode": "multi" if getattr(args, "multi", False) else "ranks",
                "spawned_by_bench": os.environ.get("CILQR_BENCH_SPAWNED") == "1",
                # the host budget the real run would take: scene-generator workers per rank under the CPU quota
                "scene_workers_per_rank": scene_workers(world), "cpu_quota_cores": cpu_quota_cores(), "logical_cpus": os.cpu_count()}
    return None


class ThreadComm:
    """--multi: the N "ranks" are threads of one process.  barrier() / max_over_ranks() stand for the process group's."""

    def __init__(self, world):
        import threading
        self.world = world
        self.bar = threading.Barrier(world)
        self.vals = [0.0] * world
        self.peer = None          # PeerGather, made by rank 0
        self.failed = None

    def barrier(self):
        self.bar.wait(timeout=600.0)

    def max_over_ranks(self, rank, v):
        return max(self.all_ranks(rank, v))

    def all_ranks(self, rank, v):
        """every rank's value, in rank order (the process group's all_gather)"""
        self.vals[rank] = v
        self.barrier()
        out = list(self.vals)
        self.barrier()
        return out


def main():
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.multi:
        if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != 1:
            raise SystemExit("bench.py: --multi is ONE process for all GPUs; it was started under a launcher with "
                             f"WORLD_SIZE={os.environ['WORLD_SIZE']}")
        return main_multi(args)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_ranks(args)       # no launcher: be the launcher

    # stdout carries exactly one line (rank 0's JSON); everything else any library prints on fd 1
    # (RCCL's version banner, for one) is sent to stderr
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.dry_run:
        rec = dry_run(args, rank, world)
        if rank == 0:
            os.write(real_stdout, (json.dumps(rec) + "\n").encode())
        return
    run(args, rank, local_rank, world, None, real_stdout)


def main_multi(args):
    """One process, a thread per GPU (see --multi).  CILQR_BENCH_MULTI_DEVICES="0,0" maps the ranks onto listed devices
    (rehearsal on a 1-GPU box: two "GPUs" that are the same one)."""
    import threading
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    world = args.gpus
    comm = ThreadComm(world)
    if args.dry_run:
        rec = dry_run_multi(args, comm)
        os.write(real_stdout, (json.dumps(rec) + "\n").encode())
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path exists)")
    devices = [int(x) for x in os.environ.get("CILQR_BENCH_MULTI_DEVICES", ",".join(str(i) for i in range(world))).split(",")]
    if len(devices) != world or max(devices) >= torch.cuda.device_count():
        raise SystemExit(f"bench.py --multi: {world} GPUs asked for, devices {devices}, {torch.cuda.device_count()} visible")
    errors = []

    def worker(r):
        try:
            run(args, r, devices[r], world, comm, real_stdout)
        except BaseException as e:   # noqa: BLE001
            errors.append((r, e))
            comm.bar.abort()         # the other threads leave their barriers with an error instead of waiting forever

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        for r, e in errors:
            sys.stderr.write(f"bench.py --multi: rank {r}: {e!r}\n")
        raise SystemExit(1)


def dry_run_multi(args, comm):
    """--multi --dry-run: the thread plumbing without a GPU -- N threads, the barrier, the max over ranks and the per-step
    PeerGather (CPU tensors), checked on rank 0 like dry_run()."""
    import threading
    import torch
    from cilqr_amd.distributed import GatherThread, PeerGather
    world = comm.world
    B, K, M = min(args.batch, 16), 6, 8
    steps = max(1, min(args.steps, 6))
    ok = {"rank_order": True, "rows": True, "steps": []}
    errors = []

    def check_on_root(g):      # between the barriers of PeerGather: the root tensors hold exactly this job
        step = len(ok["steps"])
        n = world * B
        want = 1000.0 * step + torch.arange(n, dtype=torch.float64)
        ok["rank_order"] &= bool(torch.equal(g["traj"][:, 0, 1], want))
        r_ = torch.arange(n)
        nc = g["n_cost"].to(torch.int64)
        ok["rows"] &= bool(torch.equal(nc, 1 + (r_ % B + r_ // B + step) % M)
                           and torch.equal(g["cost_hist"][r_, nc - 1, 0], want)
                           and torch.equal(g["traj"][:, 1, 0], torch.full((n,), 0.1, dtype=torch.float64))
                           and torch.equal(g["status"], (1 + (r_ // B + step) % 5).to(g["status"].dtype)))
        ok["steps"].append(step)

    peer = PeerGather(world, B, K, M, root_device=None, derive=(0.1, 1.0), on_root=check_on_root)

    def worker(rank):
        try:
            free = [dict(traj=torch.zeros((B, K, 10), dtype=torch.float64), hist=torch.zeros((B, M + 1, 5), dtype=torch.float64),
                         nc=torch.zeros(B, dtype=torch.int32), st=torch.zeros(B, dtype=torch.int32)) for _ in range(2)]
            cv = threading.Condition()

            def done(tag):
                step, slot = tag
                with cv:
                    free.append(slot)
                    cv.notify_all()

            gt = GatherThread(device=None, on_done=done, gather_fn=peer.gather_fn(rank))
            for step in range(steps):
                with cv:
                    while not free:
                        cv.wait(60.0)
                    slot = free.pop(0)
                pid = rank * B + torch.arange(B, dtype=torch.float64)
                slot["traj"][:] = (1000.0 * step + pid)[:, None, None]
                slot["traj"][:, :, 6] = 0.01 * (1 + rank)
                slot["nc"][:] = (1 + (torch.arange(B) + rank + step) % M).to(torch.int32)
                slot["hist"][:] = (1000.0 * step + pid)[:, None, None]
                slot["st"][:] = 1 + (rank + step) % 5
                gt.put((step, slot), slot["traj"], slot["hist"], slot["nc"], slot["st"])
            gt.drain()
            gt.close()
            comm.max_over_ranks(rank, float(rank))
        except BaseException as e:   # noqa: BLE001
            errors.append((rank, e))
            comm.bar.abort()
            peer.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise SystemExit(f"bench.py --multi --dry-run: {errors[0]!r}")
    good = ok["rank_order"] and ok["rows"] and ok["steps"] == list(range(steps)) and max(comm.vals) == world - 1
    return {"metric": "CILQR solves/sec (dry run: launch plumbing only, nothing solved)", "value": None, "unit": "solves/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "dry_run": True, "ranks_reporting": world,
            "gather_in_rank_order": ok["rank_order"], "gathers": len(ok["steps"]), "gathers_in_step_order": ok["steps"] == list(range(steps)),
            "ragged_history_rows_ok": ok["rows"], "gather_checks_ok": good, "mode": "multi", "spawned_by_bench": False,
            "scene_workers_per_rank": scene_workers(world), "cpu_quota_cores": cpu_quota_cores(), "logical_cpus": os.cpu_count()}


def dump_outputs(out_dir, sl, B, K, M, budget_bytes=48 << 20):
    """--dump-outputs: the results of the last timed step (slot `sl`) of a fixed, seeded sample of the batch's problems, as
    float64 .npy files; the whole batch when it fits in `budget_bytes`."""
    import torch
    per_problem = (K * 10 + (M + 1) * 5 + 4) * 8
    n = min(B, max(1, budget_bytes // per_problem))
    idx = np.arange(B) if n == B else np.sort(np.random.default_rng(20240611).choice(B, n, replace=False))
    d_idx = torch.from_numpy(idx).to(sl.traj.device)
    nc = sl.nc[d_idx].cpu().numpy()
    hist = sl.hist[d_idx].cpu().numpy()
    hist[np.arange(M + 1)[None, :] >= nc[:, None]] = 0.0     # rows past n_cost: untouched by the library in device memory
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"traj": sl.traj[d_idx].cpu().numpy(), "cost_hist": hist, "n_cost": nc, "status": sl.st[d_idx].cpu().numpy(),
              "n_iter": sl.ni[d_idx].cpu().numpy(), "problem_index": idx}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    sys.stderr.write(f"bench.py: outputs of the last timed step, {n} of {B} problems, written to {out_dir}\n")


def run(args, rank, local_rank, world, comm, real_stdout):
    """One rank: a process under a launcher (comm is None: torch.distributed over RCCL when world > 1) or a thread of --multi
    (comm: ThreadComm)."""
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path exists)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # CILQR_BENCH_FORCE_DIST=1 exercises the RCCL path (process group, all-reduce, gather) even
    # with a single rank -- the only way to smoke-test it on a 1-GPU box
    use_rccl = comm is None and (world > 1 or os.environ.get("CILQR_BENCH_FORCE_DIST") == "1")
    use_dist = use_rccl or comm is not None        # results are gathered to rank 0 after every step
    rccl_ranks = 0
    if use_rccl:
        # keep RCCL's log lines off stdout (rank 0 prints exactly one JSON line there, last)
        os.environ.setdefault("NCCL_DEBUG_FILE", "/dev/stderr")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        # self-evidence of an N > 1 run: every rank contributes 1 through RCCL
        one = torch.ones(1, dtype=torch.int32, device=dev)
        dist.all_reduce(one)
        rccl_ranks = int(one.item())
        if rccl_ranks != world:
            raise SystemExit(f"bench.py: {rccl_ranks} ranks answered the RCCL all-reduce, WORLD_SIZE is {world}")

    from cilqr_amd import api, scenario
    from cilqr_amd.distributed import GatherThread, PeerGather

    spec = scenario.SPECS[args.scene]
    B, N, K, cmax = args.batch, spec.n_steps, spec.n_steps + 1, spec.cmax
    t0 = time.time()
    workers = scene_workers(world)
    dp_info = None
    if args.coarse == "dp":
        # second scene source: DP coarse planner -> corridor producer -> the same solve
        n_distinct = min(512, B)
        gdp = scenario.generate_dp(spec, n_distinct, seed=args.seed, first_problem=rank * n_distinct, workers=workers)
        keep = np.nonzero(gdp["found"])[0]
        small = api.BatchIlqrOptimizer(api.default_config(spec.n_steps), device=local_rank, batch_capacity=len(keep), cmax=spec.cmax)
        knots = np.ascontiguousarray(gdp["coarse"][keep][:, :, :3])
        cor, ccnt, nfail = small.build_corridors(knots, gdp["obstacle_points"][keep], gdp["obstacle_count"][keep], cmax=spec.cmax)
        small.close()
        good = keep[(ccnt >= 0).all(axis=1)]
        sel = np.isin(keep, good)
        reps = (B + len(good) - 1) // len(good)
        tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B])
        sc = dict(start=tile(gdp["start"][good]), coarse=tile(gdp["coarse"][good]), corridor=tile(cor[sel]), ccount=tile(ccnt[sel]),
                  left=gdp["left"], right=gdp["right"], n_steps=spec.n_steps, dt=spec.dt, cmax=spec.cmax)
        dp_info = {"distinct_scenes": int(len(good)), "dp_failed_or_standing": int(n_distinct - len(keep)),
                   "corridor_failed": int(len(keep) - len(good)), "mean_half_planes": round(float(ccnt[sel].mean()), 2)}
    else:
        sc = scenario.generate(spec, B, seed=args.seed, first_problem=rank * B, workers=workers)
    t_gen = time.time() - t0

    cfg = api.default_config(N)
    M = cfg.max_iter
    smax = max(sc["left"].shape[0], sc["right"].shape[0])
    P = max(1, args.pipeline)
    D = args.in_flight
    profiled = args.full and not args.no_profile     # HIP events feed the breakdown and the roofline only (--full)

    d_start = torch.from_numpy(sc["start"]).to(dev)
    d_coarse = torch.from_numpy(sc["coarse"]).to(dev)
    d_cor = torch.from_numpy(sc["corridor"]).to(dev)
    d_cnt = torch.from_numpy(sc["ccount"]).to(dev)
    left = np.ascontiguousarray(sc["left"])
    right = np.ascontiguousarray(sc["right"])

    class Slot:   # result buffers of one solve in flight
        def __init__(self):
            self.used = False
            self.traj = torch.zeros((B, K, 10), dtype=torch.float64, device=dev)
            self.hist = torch.zeros((B, M + 1, 5), dtype=torch.float64, device=dev)
            self.nc = torch.zeros(B, dtype=torch.int32, device=dev)
            self.st = torch.zeros(B, dtype=torch.int32, device=dev)
            self.ni = torch.zeros(B, dtype=torch.int32, device=dev)
            self.sol = api.SolutionBatch(api.MEM_DEVICE, 0, self.traj.data_ptr(), self.hist.data_ptr(), self.nc.data_ptr(),
                                         self.st.data_ptr(), self.ni.data_ptr(), None, None)

    # the handles live in ONE pool (cilqr_pool_*): the timed steps are submitted to the pool, which deals them out round-robin
    pool = api.HandlePool(cfg, device=local_rank, handles=P, batch_capacity=B, cmax=cmax, max_lane_segments=smax)

    class Ctx:   # one handle of the pool: its stream, options and the result buffers of the solves it keeps in flight
        def __init__(self, k):
            self.opt = pool.handle_at(k, batch_capacity=B, cmax=cmax)
            if args.torch_streams:   # a torch stream per handle instead of the handle's own (tuning experiments)
                self.stream = torch.cuda.Stream()
                self.opt.set_stream(self.stream.cuda_stream)
            o = self.opt
            if args.compact_percent >= 0:
                o.set_option(api.OPT_COMPACTION, args.compact_percent)
            if args.seq_rounds >= 1:
                o.set_option(api.OPT_SEQ_ROUNDS, args.seq_rounds)
            if args.spec_threshold >= 0:
                o.set_option(api.OPT_SPEC_THRESHOLD, args.spec_threshold)
            if args.team_threshold >= 0:
                o.set_option(api.OPT_TEAM_THRESHOLD, args.team_threshold)
            if args.tail_threshold >= 0:
                o.set_option(api.OPT_TAIL_THRESHOLD, args.tail_threshold)
            if args.round_group >= 1:
                o.set_option(api.OPT_ROUND_GROUP, args.round_group)
            if args.wave_threshold >= 0:
                o.set_option(api.OPT_WAVE_THRESHOLD, args.wave_threshold)
            if args.finish_threshold >= 0:
                o.set_option(api.OPT_FINISH_THRESHOLD, args.finish_threshold)
            if args.fast_lane_ties:
                o.set_option(api.OPT_EXACT_LANE_TIES, 0)
            self.slots = [Slot() for _ in range(D + (2 if use_dist else 1))]   # D in flight + the one(s) whose results are being gathered
            self.free = list(self.slots)
            self.fifo = []          # submitted, oldest first
            # the first slot doubles as the buffers of the synchronous calls below
            s0 = self.slots[0]
            self.traj, self.hist, self.nc, self.st, self.ni, self.sol = s0.traj, s0.hist, s0.nc, s0.st, s0.ni, s0.sol

    ctx = [Ctx(k) for k in range(P)]
    opt = ctx[0].opt
    prob = opt.make_problem(B, d_start.data_ptr(), d_coarse.data_ptr(), d_cor.data_ptr(), d_cnt.data_ptr(),
                            cmax, left.ctypes.data, right.ctypes.data, left.shape[0], right.shape[0],
                            api.MEM_DEVICE)
    thr_team, thr_wave = opt.get_option(api.OPT_TEAM_THRESHOLD)[0], opt.get_option(api.OPT_WAVE_THRESHOLD)[0]   # as the library holds them
    torch.cuda.synchronize()   # inputs uploaded and outputs zero-filled before the solvers' own streams start

    prof_acc = dict(bwd_ms=0.0, bwd_launches=0, bwd_steps=0, iters=0, full_ms=0.0, full_launches=0)
    last_gather = [None]   # [0]: result of the last gather; [-1]: the slot it gathered (when any)

    # The per-step results gather (one collective per job, rank r's block after rank r-1's) runs on a thread and a
    # stream of its own (cilqr_amd/distributed.py: GatherThread): packing, the length agreement (a host sync) and, on rank 0,
    # unpacking world x the payload never hold the loop that keeps the handles fed.  Every rank gathers its finished steps in
    # the order they finished, so the ranks' collectives pair up; a slot goes back to its handle's free list when its gather is done.
    import threading
    free_cv = threading.Condition()

    def slot_gathered(tag):
        c_, sl_ = tag
        with free_cv:
            c_.free.append(sl_)
            free_cv.notify_all()

    # 8 of the 10 trajectory columns travel (time and kappa are functions of the others)
    gatherer = None
    cabi_handle, cabi_out = None, None
    if use_rccl and args.gather == "c_abi":
        # cilqr_gather_results carries the timed region.  The communicator sits on a small handle of its own: a handle is
        # driven by one thread at a time, and its stream must not queue the exchange behind a solve's kernels.
        cabi_handle = api.BatchIlqrOptimizer(cfg, device=local_rank, batch_capacity=64, cmax=cmax, max_lane_segments=smax)
        ids = [api.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0)
        cabi_handle.comm_create(ids[0], rank, world)
        if rank == 0:
            cabi_out = dict(traj=torch.zeros((world * B, K, 10), dtype=torch.float64, device=dev),
                            hist=torch.zeros((world * B, M + 1, 5), dtype=torch.float64, device=dev),
                            nc=torch.zeros(world * B, dtype=torch.int32, device=dev), st=torch.zeros(world * B, dtype=torch.int32, device=dev))
            cabi_sol = api.SolutionBatch(api.MEM_DEVICE, 0, cabi_out["traj"].data_ptr(), cabi_out["hist"].data_ptr(),
                                         cabi_out["nc"].data_ptr(), cabi_out["st"].data_ptr(), None, None, None)

        def cabi_gather(traj_, hist_, nc_, st_):
            local = api.SolutionBatch(api.MEM_DEVICE, 0, traj_.data_ptr(), hist_.data_ptr(), nc_.data_ptr(), st_.data_ptr(), None, None, None)
            rc_ = cabi_handle.gather_results_raw(B, local, 0, cabi_sol if rank == 0 else None)
            if rc_ != api.OK:
                raise api.CilqrError(rc_, "in cilqr_gather_results (timed region)")
            return ({"traj": cabi_out["traj"], "n_cost": cabi_out["nc"], "status": cabi_out["st"], "cost_hist": cabi_out["hist"]}
                    if rank == 0 else None)

        torch.cuda.synchronize()
        gatherer = GatherThread(device=dev, on_done=slot_gathered, gather_fn=cabi_gather)
    elif use_rccl:
        gatherer = GatherThread(device=dev, dst=0, derive=(cfg.dt, cfg.wheel_base), on_done=slot_gathered)
    elif comm is not None:      # --multi: peer copies into tensors on rank 0's device
        if rank == 0:
            comm.peer = PeerGather(world, B, K, M, root_device=dev, derive=(cfg.dt, cfg.wheel_base))
        comm.barrier()
        gatherer = GatherThread(device=dev, on_done=slot_gathered, gather_fn=comm.peer.gather_fn(rank))

    def take_free(c):
        with free_cv:
            while not c.free:
                if not free_cv.wait(timeout=120.0):
                    raise RuntimeError("bench.py: no result slot came back from the gather thread within 120 s")
            return c.free.pop(0)

    def drain_gathers():
        if use_dist:
            gatherer.drain()
            if gatherer.last_tag is not None:
                last_gather[:] = [gatherer.last, gatherer.last_tag[1]]

    dealt = [0, 0]   # solves submitted to / collected from the pool so far: solve s runs on handle s % P, the oldest is collected first

    def wait_oldest(c, through_pool):
        # the oldest solve in flight: of the pool (it sits on handle c = ctx[collected % P]) or of handle c used alone
        rc = pool.wait() if through_pool else c.opt.wait()
        sl = c.fifo.pop(0)
        if rc != api.OK:
            raise api.CilqrError(rc, "in bench step")
        if through_pool:
            dealt[1] += 1
        return sl, ((pool.profile() if through_pool else c.opt.profile()) if profiled else None)

    last_timed = [None]   # the slot of the last timed step (steps finish oldest first)

    def finish(c, sl, p, timed):
        if timed:
            last_timed[0] = sl
        if timed and p is not None:
            prof_acc["bwd_ms"] += p.backward_ms
            prof_acc["bwd_launches"] += p.backward_launches
            prof_acc["bwd_steps"] += p.backward_problem_steps
            prof_acc["iters"] += p.iterations
            prof_acc["full_ms"] += p.backward_full_ms
            prof_acc["full_launches"] += p.backward_full_launches
        if use_dist:
            gatherer.put((c, sl), sl.traj, sl.hist, sl.nc, sl.st)      # the gather thread hands the slot back when the collective is done
        else:
            c.free.append(sl)

    def run_steps(n, timed, alone=None):
        # alone = None: the steps go to the POOL (cilqr_pool_submit / cilqr_pool_wait), at most P * D in flight;
        # alone = a handle of the (then empty) pool: cilqr_submit / cilqr_wait on it, at most D in flight.
        # A finished step is gathered AFTER the next one has been submitted (its buffers are a slot of their own), so no
        # handle is without work while the host packs and sends results.
        through_pool = alone is None
        for s_ in range(n):
            c = ctx[dealt[0] % P] if through_pool else alone       # the handle this step is dealt to
            oldest = ctx[dealt[1] % P] if through_pool else alone
            full = (dealt[0] - dealt[1] == P * D) if through_pool else (len(alone.fifo) == D)
            done = (oldest, wait_oldest(oldest, through_pool)) if full else None
            sl = take_free(c)
            sl.used = True
            rc = pool.submit_raw(prob, sl.sol) if through_pool else c.opt.submit_raw(prob, sl.sol)
            if rc != api.OK:
                raise api.CilqrError(rc, "in bench submit")
            if through_pool:
                dealt[0] += 1
                if args.stagger_ms > 0 and s_ + 1 < min(n, P) and dealt[0] - dealt[1] == s_ + 1:
                    time.sleep(args.stagger_ms * 1e-3)   # the pool was empty when this region began: offset the handles' phases
            c.fifo.append(sl)
            if done is not None:
                finish(done[0], done[1][0], done[1][1], timed)
        while (dealt[0] > dealt[1]) if through_pool else alone.fifo:
            oldest = ctx[dealt[1] % P] if through_pool else alone
            done = wait_oldest(oldest, through_pool)
            finish(oldest, done[0], done[1], timed)
        drain_gathers()      # a region ends when its last step's results are on rank 0

    def fence():
        if use_rccl:
            dist.barrier()
        elif comm is not None:
            torch.cuda.synchronize()
            comm.barrier()
        torch.cuda.synchronize()

    # One untimed solve on one handle (part of the warm-up); with --full a second one with HIP events around every phase of
    # every lockstep iteration: the per-phase breakdown, the single-batch (un-pipelined) time and the un-overlapped
    # duration of the full-batch backward launch.
    single = None
    rc = opt.solve_raw(prob, ctx[0].sol)   # first solve of the process: code objects, scratch and staging get allocated
    if rc != api.OK:
        raise api.CilqrError(rc, "in the first solve")
    if profiled:
        opt.set_profiling(1)
        rc = opt.solve_raw(prob, ctx[0].sol)
        if rc != api.OK:
            raise api.CilqrError(rc, "in calibration step")
        pc = opt.profile()
        single = dict(quad_ms=pc.quadratize_ms, bwd_ms=pc.backward_ms, ls_ms=pc.linesearch_ms, other_ms=pc.other_ms,
                      tail_ms=pc.tail_ms, tail_problems=pc.tail_problems, lockstep_launches=pc.backward_launches,
                      total_ms=pc.total_ms, iterations=pc.iterations, bwd_launches=pc.backward_launches,
                      bwd_problem_steps=pc.backward_problem_steps,
                      bwd_full_ms=(pc.backward_full_ms / pc.backward_full_launches) if pc.backward_full_launches else None)
        for c in ctx:
            c.opt.set_profiling(2)      # timed steps: events around the backward launches only (< 1 %)
    run_steps(args.warmup, False)
    fence()
    if use_dist:
        gatherer.reset_stats()
    cpu0 = cpu_seconds()
    thr0 = thread_cpu_seconds()
    t_start = time.perf_counter()
    run_steps(args.steps, True)
    fence()
    elapsed = time.perf_counter() - t_start
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_timed[0], B, K, M)
    # host CPU of the timed region: what one rank's threads -- the loop, the handles' solver workers, the
    # gather thread, RCCL's proxy -- burn per step, so that N ranks can be budgeted against the box's CPU quota
    cpu_rank = cpu_seconds() - cpu0
    n_threads = native_thread_count()
    thr1 = thread_cpu_seconds()
    by_thread = sorted(((name, round((c - thr0.get(tid, (name, 0.0))[1]) / max(elapsed, 1e-9), 3)) for tid, (name, c) in thr1.items()),
                       key=lambda t: -t[1])
    by_name = {}
    for name, cores in by_thread:     # threads of one kind (the handles' workers, RCCL's proxies ...) summed
        k = by_name.setdefault(name, [0, 0.0])
        k[0] += 1
        k[1] = round(k[1] + cores, 3)
    gather_timed = dict(busy_s=gatherer.busy_s, count=gatherer.count) if use_dist else None
    # First-contact insurance for runs this container cannot rehearse: the figures of EVERY rank on the
    # line, not only their maximum, and a check that block r of what rank 0 gathered IS rank r's result.
    def checksum(traj_, nc_, st_):
        """64-bit, position-dependent (wrapping int64 arithmetic), of the 8 travelling trajectory columns, n_cost and status."""
        t8 = traj_[:, :, [1, 2, 3, 4, 5, 6, 8, 9]].contiguous().view(torch.int64).reshape(-1)
        w = torch.arange(t8.numel(), dtype=torch.int64, device=t8.device) * 2 + 1
        ints = torch.cat([nc_.to(torch.int64), st_.to(torch.int64)])
        wi = torch.arange(ints.numel(), dtype=torch.int64, device=ints.device) * 2 + 0x9E3779B1
        return int(((t8 * w).sum() + (ints * wi).sum() * 31).item())

    my_sum = None
    if use_dist and last_gather[-1] is not None:
        sl_ = last_gather[-1]
        my_sum = checksum(sl_.traj, sl_.nc, sl_.st)
    if use_rccl:
        mine = torch.tensor([elapsed, cpu_rank, float(gatherer.busy_s)], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        per_rank = [[float(x) for x in e.tolist()] for e in every]
        sums = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(sums, torch.tensor([my_sum if my_sum is not None else 0], dtype=torch.int64, device=dev))
        rank_sums = [int(x.item()) for x in sums]
    elif comm is not None:
        per_rank = comm.all_ranks(rank, [elapsed, cpu_rank / world, float(gatherer.busy_s)])   # (one process: its CPU time shared out)
        rank_sums = comm.all_ranks(rank, my_sum if my_sum is not None else 0)
    else:
        per_rank, rank_sums = [[elapsed, cpu_rank, 0.0]], []
    elapsed = max(p_[0] for p_ in per_rank)
    cpu_max, cpu_sum = max(p_[1] for p_ in per_rank), sum(p_[1] for p_ in per_rank)
    gather_verified = None
    if use_dist and rank == 0 and last_gather[0] is not None:
        res_ = last_gather[0]
        gather_verified = 0
        for r_ in range(world):
            blk = slice(r_ * B, (r_ + 1) * B)
            gather_verified += int(checksum(res_["traj"][blk], res_["n_cost"][blk], res_["status"][blk]) == rank_sums[r_])
    quota = cpu_quota_cores()
    host = {
        "cpu_s_per_step_max_rank": round(cpu_max / args.steps, 5), "cpu_s_per_step_all_ranks": round(cpu_sum / args.steps, 5),
        "cores_busy_per_rank": [round(p_[1] / max(p_[0], 1e-9), 3) for p_ in per_rank],
        # cores kept busy by the timed region: CPU seconds / wall seconds, all ranks together, against the quota they share
        "cores_busy_all_ranks": round(cpu_sum / elapsed, 3), "cpu_quota_cores": quota, "logical_cpus": os.cpu_count(),
        "quota_fraction": (round(cpu_sum / elapsed / quota, 4) if quota else None),
        "native_threads_this_rank": n_threads, "scene_workers_per_rank": workers,
        # cores kept busy per KIND of thread of this rank's process over the timed region: [threads, cores]
        "cores_busy_by_thread_name": {k: v for k, v in sorted(by_name.items(), key=lambda kv: -kv[1][1])[:8] if v[1] > 0.0},
        "busiest_threads": [[name, cores] for name, cores in by_thread[:6] if cores > 0.0],
        "note": "resource.getrusage(RUSAGE_SELF) around the timed region, per rank (a process; with --multi the one process "
                "is measured once and divided by the ranks for the per-rank figure); threads = /proc/self/status",
    }

    # Extra (never `value`): the same gather through the C-ABI (cilqr_comm_* / cilqr_gather_results: librccl
    # called directly, no PyTorch), checked against the torch.distributed gather of the timed region.  Guarded
    # by a watchdog: a multi-rank send / recv cannot be rehearsed on a 1-GPU box.
    cabi = None
    hung = False
    if use_rccl and args.full and args.gather == "c_abi":
        # the timed region went through cilqr_gather_results: the torch.distributed gather of the same (last) step beside it
        from cilqr_amd.distributed import gather_results as torch_gather
        sl_ = last_gather[-1]
        tg = torch_gather(sl_.traj, sl_.hist, sl_.nc, sl_.st, dst=0, densify=False, derive=(cfg.dt, cfg.wheel_base))
        cabi = {"ok": True, "carried_the_timed_region": True}
        if rank == 0:
            g_ = last_gather[0]
            cols = [1, 2, 3, 4, 5, 6, 8, 9]
            cabi["ranks"] = world
            cabi["identical_to_torch_gather"] = bool(
                torch.equal(g_["traj"][:, :, cols], tg["traj"][:, :, cols]) and torch.equal(g_["n_cost"], tg["n_cost"])
                and torch.equal(g_["status"], tg["status"])
                and torch.equal(g_["cost_hist"][torch.arange(M + 1, device=dev)[None, :] < g_["n_cost"][:, None].long()], tg["hist_rows"])
                and bool(torch.allclose(g_["traj"][:, :, 7], tg["traj"][:, :, 7], rtol=1e-15, atol=0.0)))
            cabi["rank0_block_identical_to_local"] = bool(torch.equal(g_["traj"][:B], sl_.traj))
    elif use_rccl and args.full:
        import threading
        res = {}

        def run_cabi():
            try:
                ids = [api.comm_unique_id() if rank == 0 else None]
                dist.broadcast_object_list(ids, src=0)
                opt.comm_create(ids[0], rank, world)
                g = None
                if rank == 0:
                    g = dict(traj=torch.zeros((world * B, K, 10), dtype=torch.float64, device=dev),
                             hist=torch.zeros((world * B, M + 1, 5), dtype=torch.float64, device=dev),
                             nc=torch.zeros(world * B, dtype=torch.int32, device=dev),
                             st=torch.zeros(world * B, dtype=torch.int32, device=dev))
                    gsol = api.SolutionBatch(api.MEM_DEVICE, 0, g["traj"].data_ptr(), g["hist"].data_ptr(),
                                             g["nc"].data_ptr(), g["st"].data_ptr(), None, None, None)
                torch.cuda.synchronize()
                dist.barrier()
                times = []
                for _ in range(3):
                    t1 = time.perf_counter()
                    rc_ = opt.gather_results_raw(B, last_gather[-1].sol, 0, gsol if rank == 0 else None)
                    times.append(time.perf_counter() - t1)
                    if rc_ != api.OK:
                        raise api.CilqrError(rc_, "in cilqr_gather_results")
                res["ms"] = round(1e3 * min(times), 3)
                if rank == 0:
                    tg = last_gather[0]
                    res["ranks"] = world
                    # the torch path rebuilds kappa with torch.tan, the C-ABI with the device's tan (as the solver
                    # does): compare the 8 travelling columns bit for bit, kappa to an ulp
                    cols = [1, 2, 3, 4, 5, 6, 8, 9]
                    res["identical_to_torch_gather"] = bool(
                        torch.equal(g["traj"][:, :, cols], tg["traj"][:, :, cols]) and torch.equal(g["nc"], tg["n_cost"])
                        and torch.equal(g["st"], tg["status"])
                        and torch.equal(g["hist"][torch.arange(M + 1, device=dev)[None, :] < g["nc"][:, None].long()],
                                        tg["hist_rows"])
                        and bool(torch.allclose(g["traj"][:, :, 7], tg["traj"][:, :, 7], rtol=1e-15, atol=0.0)))
                    res["rank0_block_identical_to_local"] = bool(torch.equal(g["traj"][:B], last_gather[-1].traj))
                opt.comm_destroy()
                res["ok"] = True
            except Exception as e:   # noqa: BLE001
                res["ok"] = False
                res["error"] = repr(e)

        th = threading.Thread(target=run_cabi, daemon=True)
        th.start()
        th.join(120.0)
        cabi = dict(res) if not th.is_alive() else {"ok": False, "error": "no return within 120 s"}
        hung = th.is_alive()

    # the same steps through ONE of the handles (two solves in flight on it): what a caller with one handle's memory gets
    one_handle = None
    if world == 1 and P > 1 and args.full:
        run_steps(min(args.warmup, 4), False, ctx[0])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_steps(args.steps, False, ctx[0])
        torch.cuda.synchronize()
        t_one = (time.perf_counter() - t1) / args.steps
        one_handle = {"value": round(B / t_one, 1), "unit": "solves/s", "ms_per_step": round(t_one * 1e3, 3),
                      "batches_in_flight": D, "device_bytes": ctx[0].opt.device_bytes()}
    # sequential form: two more steps back to back on one handle, no events
    seq = None
    if world == 1 and P * D > 1 and args.full:
        opt.set_profiling(0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(2):
            if opt.solve_raw(prob, ctx[0].sol) != api.OK:
                raise api.CilqrError(-1, "in sequential step")
        torch.cuda.synchronize()
        seq = (time.perf_counter() - t1) / 2
    same = (all(bool(torch.equal(sl.traj, ctx[0].traj)) and bool(torch.equal(sl.nc, ctx[0].nc)) and
                bool(torch.equal(sl.st, ctx[0].st)) and bool(torch.equal(sl.ni, ctx[0].ni)) for c in ctx for sl in c.slots if sl.used)
            if args.full else None)

    # ---- Extra legs (never `value`): what a caller sees whose arrays are not already in HBM ("report both with
    # and without transfers").  Both run through the same pool as the timed region, with as many solves
    # submitted as it takes (cilqr_pool_depth: two in flight and one queued per handle).
    dev_bytes_timed = sum(c.opt.device_bytes() for c in ctx)      # (before the extra legs grow the host-array staging)
    extras = world == 1 and args.full and not args.no_extras
    n_extra = args.extra_steps if args.extra_steps > 0 else min(args.steps, 24)
    depth = pool.depth()

    def pooled(n, submit_one, collect_one):
        sub = col = 0
        for _ in range(n):
            if sub - col == depth:
                if pool.wait() != api.OK:
                    raise api.CilqrError(-1, "in an extra leg")
                collect_one(col)
                col += 1
            submit_one(sub)
            sub += 1
        while col < sub:
            if pool.wait() != api.OK:
                raise api.CilqrError(-1, "in an extra leg")
            collect_one(col)
            col += 1

    def host_cores(fn):
        c0, t0_ = cpu_seconds(), time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt_ = time.perf_counter() - t0_
        return dt_, (cpu_seconds() - c0) / dt_

    # (1) pcie_inclusive: every input and output array of every step in HOST memory (pageable numpy arrays, what
    # ilqr_optimizer.h:41-48 hands over and takes back): cilqr_pool_submit with CILQR_MEM_HOST.  The library uploads the queued
    # solve's arrays on a stream of its own while the solve in front iterates, downloads the trajectories straight into the
    # caller's array and the LIVE cost rows packed (include/cilqr.h, cilqr_submit).
    pcie = None
    if extras:
        try:
            opt.set_profiling(0)
            h_in = {k: np.ascontiguousarray(sc[k]) for k in ("start", "coarse", "corridor")}
            h_in["ccount"] = np.ascontiguousarray(sc["ccount"], dtype=np.int32)
            prob_h = opt.make_problem(B, h_in["start"].ctypes.data, h_in["coarse"].ctypes.data, h_in["corridor"].ctypes.data,
                                      h_in["ccount"].ctypes.data, cmax, left.ctypes.data, right.ctypes.data, left.shape[0], right.shape[0],
                                      api.MEM_HOST)

            class HostSlot:   # arrive dirty: the library owes zeros behind the live cost rows
                def __init__(self):
                    self.traj = np.full((B, K, 10), -1.0)
                    self.hist = np.full((B, M + 1, 5), -1.0)
                    self.nc, self.st, self.ni = (np.full(B, -1, np.int32) for _ in range(3))
                    self.sol = api.SolutionBatch(api.MEM_HOST, 0, self.traj.ctypes.data, self.hist.ctypes.data, self.nc.ctypes.data,
                                                 self.st.ctypes.data, self.ni.ctypes.data, None, None, None)

            hs = [HostSlot() for _ in range(depth)]

            def sub_h(i):
                if pool.submit_raw(prob_h, hs[i % depth].sol) != api.OK:
                    raise api.CilqrError(-1, "in pcie_inclusive submit")

            pooled(depth + 1, sub_h, lambda i: None)      # staging blocks allocated, the caller's pages touched
            dt_h, cores_h = host_cores(lambda: pooled(n_extra, sub_h, lambda i: None))
            ref_t, ref_nc = ctx[0].traj.cpu().numpy(), ctx[0].nc.cpu().numpy()
            live = np.arange(M + 1)[None, :] < ref_nc[:, None]
            ref_h = ctx[0].hist.cpu().numpy()
            same_h = all(bool(np.array_equal(x.traj, ref_t) and np.array_equal(x.nc, ref_nc) and np.array_equal(x.st, ctx[0].st.cpu().numpy())
                              and np.array_equal(x.ni, ctx[0].ni.cpu().numpy()) and np.array_equal(x.hist[live], ref_h[live])
                              and not x.hist[~live].any()) for x in hs[:2])
            # the synchronous call on the same arrays (what the drop-in adapter would do with a batch this size): nothing overlaps,
            # upload + solve + download one after the other
            t_sync = []
            for _ in range(3):
                t1 = time.perf_counter()
                if opt.solve_raw(prob_h, hs[0].sol) != api.OK:
                    raise api.CilqrError(-1, "in pcie_inclusive synchronous call")
                t_sync.append(time.perf_counter() - t1)
            in_b = sum(v.nbytes for v in h_in.values())
            pcie = {"value": round(B * n_extra / dt_h, 1), "unit": "solves/s", "ms_per_step": round(1e3 * dt_h / n_extra, 3), "steps": n_extra,
                    "memory": "pageable host arrays in and out (numpy), CILQR_MEM_HOST through cilqr_pool_submit",
                    "input_bytes_per_step": in_b, "output_bytes_per_step_dense": int(hs[0].traj.nbytes + hs[0].hist.nbytes + 3 * hs[0].nc.nbytes),
                    "output_bytes_per_step_travelling": int(hs[0].traj.nbytes + int(ref_nc.sum()) * 40 + 4 * B * 4),
                    "pcie_floor_ms_per_step_at_57_GBps": round(in_b / 57e9 * 1e3, 2),
                    "host_cores_busy": round(cores_h, 2), "submitted_at_once": depth,
                    "synchronous_call": {"value": round(B / min(t_sync[1:]), 1), "unit": "solves/s", "ms_per_step": round(1e3 * min(t_sync[1:]), 3),
                                         "note": "cilqr_solve_batch with the same host arrays, one batch at a time (round 5: 454 k)"},
                    "identical_to_device_resident": same_h, "device_bytes": pool.device_bytes()}
            del hs, h_in
        except Exception as e_:   # noqa: BLE001  (an extra leg must never cost the line its `value`)
            pcie = {"error": repr(e_)}
            while pool.wait() != api.ERR_STATE:      # whatever it left in flight on the pool (ERR_STATE: nothing is)
                pass

    # (2) end_to_end: the producer in front of the solve (corridor.cc:58-263, trajectory_planner.cpp:49-86):
    # obstacle corner points per knot -> cilqr_build_corridors -> solve, everything resident in HBM.  The corridors of step
    # n + 1 are built (on a handle and a stream of their own) while the pool iterates the steps before it.
    end_to_end = None
    if extras:
        try:
            sc_p = scenario.generate(spec, B, seed=args.seed, first_problem=rank * B, workers=workers, obstacle_points=True)
            P_ = sc_p["obstacle_points"].shape[2]
            d_knots = torch.from_numpy(np.ascontiguousarray(sc_p["coarse"][:, :, :3])).to(dev)
            d_pts = torch.from_numpy(sc_p["obstacle_points"]).to(dev)
            d_pcnt = torch.from_numpy(sc_p["obstacle_count"]).to(dev)
            ccfg = api.default_corridor_config()
            producer = api.BatchIlqrOptimizer(cfg, device=local_rank, batch_capacity=64, cmax=cmax, max_lane_segments=smax)

            class E2eSlot:
                def __init__(self):
                    self.cor = torch.zeros((B, K, cmax, 3), dtype=torch.float64, device=dev)
                    self.cnt = torch.zeros((B, K), dtype=torch.int32, device=dev)
                    self.traj = torch.zeros((B, K, 10), dtype=torch.float64, device=dev)
                    self.hist = torch.zeros((B, M + 1, 5), dtype=torch.float64, device=dev)
                    self.nc, self.st = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
                    self.prob = opt.make_problem(B, d_start.data_ptr(), d_coarse.data_ptr(), self.cor.data_ptr(), self.cnt.data_ptr(), cmax,
                                                 left.ctypes.data, right.ctypes.data, left.shape[0], right.shape[0], api.MEM_DEVICE)
                    self.sol = api.SolutionBatch(api.MEM_DEVICE, 0, self.traj.data_ptr(), self.hist.data_ptr(), self.nc.data_ptr(),
                                                 self.st.data_ptr(), None, None, None)

            es = [E2eSlot() for _ in range(depth)]
            torch.cuda.synchronize()
            t_cor, failed = [], [0]

            def sub_e(i):
                sl = es[i % depth]
                t1 = time.perf_counter()
                rc_, nf_ = producer.build_corridors_raw(ccfg, B, K, d_knots.data_ptr(), d_pts.data_ptr(), d_pcnt.data_ptr(), P_,
                                                        sl.cor.data_ptr(), sl.cnt.data_ptr(), cmax, api.MEM_DEVICE)
                t_cor.append(time.perf_counter() - t1)
                failed[0] = nf_
                if rc_ != api.OK or pool.submit_raw(sl.prob, sl.sol) != api.OK:
                    raise api.CilqrError(rc_, "in end-to-end step")

            pooled(depth + 1, sub_e, lambda i: None)
            torch.cuda.synchronize()
            # the two halves alone, one batch at a time (what round 5 reported as the whole figure)
            t1 = time.perf_counter()
            producer.build_corridors_raw(ccfg, B, K, d_knots.data_ptr(), d_pts.data_ptr(), d_pcnt.data_ptr(), P_, es[0].cor.data_ptr(),
                                         es[0].cnt.data_ptr(), cmax, api.MEM_DEVICE)
            torch.cuda.synchronize()
            t_cor_alone = time.perf_counter() - t1
            t1 = time.perf_counter()
            if opt.solve_raw(es[0].prob, es[0].sol) != api.OK:
                raise api.CilqrError(-1, "in end-to-end solve")
            torch.cuda.synchronize()
            t_solve_alone = time.perf_counter() - t1
            first = (es[0].traj.clone(), es[0].nc.clone(), es[0].st.clone())
            del t_cor[:]
            dt_e, cores_e = host_cores(lambda: pooled(n_extra, sub_e, lambda i: None))
            same_e = all(bool(torch.equal(x.traj, first[0]) and torch.equal(x.nc, first[1]) and torch.equal(x.st, first[2])) for x in es)
            e_status = np.bincount(es[0].st.cpu().numpy(), minlength=7).tolist()
            assert e_status[6] == 0 or failed[0] > 0   # a knot whose corridor could not be built takes its problem out of the solve (status 6)
            end_to_end = {"value": round(B * n_extra / dt_e, 1), "unit": "solves/s", "ms_per_step": round(1e3 * dt_e / n_extra, 3), "steps": n_extra,
                          "corridor_call_ms_beside_solves": round(1e3 * sum(t_cor) / max(1, len(t_cor)), 3),
                          "corridor_ms_alone": round(t_cor_alone * 1e3, 3), "solve_ms_alone": round(t_solve_alone * 1e3, 3),
                          "sequential_value": round(B / (t_cor_alone + t_solve_alone), 1),
                          "corridors_failed": failed[0], "status_histogram": e_status, "host_cores_busy": round(cores_e, 2),
                          "identical_across_steps_and_to_the_sequential_call": same_e,
                          "mean_obstacle_points": round(float(sc_p["obstacle_count"].mean()), 2),
                          "mean_half_planes": round(float(es[0].cnt.clamp(min=0).double().mean().item()), 2),
                          "note": "obstacle points in HBM -> k_build_corridors (sphere-flip construction, on a handle and stream of its own) -> "
                                  "cilqr_pool_submit; the corridors of a step are built while the pool iterates the steps before it.  Other "
                                  "corridors than the generator's simplified ones of the timed region: a larger feasible set, another "
                                  "iteration count"}
            producer.close()
            del es, d_pts, d_knots, d_pcnt, sc_p
            torch.cuda.empty_cache()
        except Exception as e_:   # noqa: BLE001  (an extra leg must never cost the line its `value`)
            end_to_end = {"error": repr(e_)}
            while pool.wait() != api.ERR_STATE:      # whatever it left in flight on the pool (ERR_STATE: nothing is)
                pass

    traffic = None
    if world == 1 and not args.no_traffic and profiled and single and single["bwd_problem_steps"] > 0:
        traffic = measure_backward_traffic(args, single["bwd_problem_steps"])
    latency = None
    if world == 1 and args.full and not args.no_latency:
        latency = plan_latency(scenario, ("ped6", "mix11", "dyn20"), args.latency_scenes, 100 + args.seed, workers)

    # sanity: every problem must have terminated with a valid status
    st = ctx[0].st.cpu().numpy()
    nc = ctx[0].nc.cpu().numpy()
    assert ((st >= 1) & (st <= 5)).all() and (nc >= 1).all(), "unterminated problems in the batch"

    if rank == 0:
        ms_per_step = 1e3 * elapsed / args.steps
        value = world * B * args.steps / elapsed
        roof = None
        if profiled and prof_acc["bwd_ms"] > 0:
            # ALGORITHMIC bytes: a launch over n problems moves n*(N*110+44)*8 B dense.
            # One solve launches the backward kernel once per lockstep iteration, over 65536 problems at
            # first and over a few stragglers at the end.  The top level aggregates ALL launches of the
            # timed region (sum of bytes / sum of HIP-event durations = bytes per launch / avg duration,
            # what `rocprofv3 --stats` reproduces); `full_batch` is the same over the launches that covered
            # the whole batch (the metric's "batch=65536" case).
            per_problem = (N * api.DENSE_DOUBLES_PER_STEP + api.DENSE_DOUBLES_TERMINAL) * 8.0
            n_act_sum = prof_acc["bwd_steps"] / N
            alg_bytes = n_act_sum * per_problem
            t_all = prof_acc["bwd_ms"] * 1e-3
            achieved = alg_bytes / t_all / 1e9
            # HBM bytes per problem-step as recorded with rocprofv3 PMC counters for this scene family
            # (separate --pmc passes, FETCH_SIZE x 2 on gfx950 + WRITE_SIZE; profiles/): a constant of the
            # kernel and the workload, NOT measured in this run -> `traffic` stays null
            rec = None
            try:
                with open(args.traffic_file) as f:
                    tf = json.load(f)
                rec = tf.get("by_workload", {}).get(f"{args.scene}_n{N}") or (tf if args.scene == "mix11" and N == 50 else None)
            except Exception:
                rec = None
            if traffic:   # measured for this run's workload (counter passes over a one-step run): supersedes the recorded figure
                rec = dict(rec or {}, hbm_bytes_per_problem_step_all_launches=traffic["hbm_bytes_per_problem_step"])
                if traffic.get("full_batch_launch_hbm_bytes"):
                    rec["full_batch_launch"] = {"hbm_bytes_per_problem_step": traffic["full_batch_launch_hbm_bytes"] / (B * N)}
            if rec is not None and "full_batch_launch" not in rec:
                rec = None if not traffic else dict(rec, full_batch_launch={"hbm_bytes_per_problem_step": rec["hbm_bytes_per_problem_step_all_launches"]})
            real_all = rec["hbm_bytes_per_problem_step_all_launches"] * prof_acc["bwd_steps"] if rec else None
            bps = rec["hbm_bytes_per_problem_step_all_launches"] if rec else None
            gbs = lambda nbytes, t: nbytes / t / 1e9                                   # noqa: E731
            # Contended figures: every backward launch of the TIMED region.  With P x D solves in flight a kernel's duration
            # includes the time its CUs spent on the other streams' kernels.
            contended = {"achieved": round(gbs(alg_bytes, t_all), 1),
                         "frac": round(gbs(real_all, t_all) / HBM_PEAK_GBS, 4) if real_all else None,
                         "frac_algorithmic": round(gbs(alg_bytes, t_all) / HBM_PEAK_GBS, 4),
                         "avg_launch_ms": prof_acc["bwd_ms"] / prof_acc["bwd_launches"], "launches": prof_acc["bwd_launches"],
                         "mean_problems_per_launch": n_act_sum / prof_acc["bwd_launches"], "batches_in_flight": P * D}
            # The kernel's own figures: the same launches of ONE solve with nothing else on the GPU -- the calibration solve of
            # this run (HIP events from the kernel's own start / end stamps on the solve's stream, one batch in flight).
            # These are the top-level keys; the timed region's are the *_contended keys.
            if single and single["bwd_ms"] > 0:
                t1 = single["bwd_ms"] * 1e-3
                n1 = single["bwd_launches"]
                alg1 = single["bwd_problem_steps"] / N * per_problem
                real1 = bps * single["bwd_problem_steps"] if bps else None
                own = {"achieved": round(gbs(alg1, t1), 1), "achieved_real": round(gbs(real1, t1), 1) if real1 else None,
                       "frac": round(gbs(real1, t1) / HBM_PEAK_GBS, 4) if real1 else None,
                       "frac_algorithmic": round(gbs(alg1, t1) / HBM_PEAK_GBS, 4), "avg_launch_ms": single["bwd_ms"] / n1,
                       "launches": n1, "mean_problems_per_launch": single["bwd_problem_steps"] / N / n1,
                       "traffic": (real1 / n1) if (traffic and real1) else None, "alg_per_launch": alg1 / n1,
                       "real_per_launch": (real1 / n1) if real1 else None,
                       "launch": "every backward launch of ONE solve of the batch with nothing else on the GPU (this run's calibration "
                                 f"solve: 65536 problems down to the tail threshold; launches of <= {thr_team} / <= {thr_wave} problems run the 8-lanes / "
                                 "wave-per-problem kernels and sit on the latency of N dependent steps; the last problems finish inside "
                                 "k_tail), time-weighted: sum of bytes / sum of durations"}
            else:
                own = dict(contended, achieved_real=round(gbs(real_all, t_all), 1) if real_all else None,
                           traffic=(real_all / prof_acc["bwd_launches"]) if (traffic and real_all) else None,
                           alg_per_launch=alg_bytes / prof_acc["bwd_launches"],
                           real_per_launch=(real_all / prof_acc["bwd_launches"]) if real_all else None,
                           launch="every backward launch of the timed region (no calibration solve in this run), time-weighted")
            full_alone_ms = single["bwd_full_ms"] if single else None
            real_full = rec["full_batch_launch"]["hbm_bytes_per_problem_step"] * B * N if rec else None
            roof = {
                "bound": "hbm", "kernel": f"cilqr::k_backward (+ k_backward_team / k_backward_wave for launches of <= {thr_team} / <= {thr_wave} problems)",
                "launch": own["launch"],
                # achieved / peak = frac, ON THE SAME BYTES: the HBM bytes really moved (PMC counters: FETCH_SIZE x 2 + WRITE_SIZE,
                # separate passes) -- the stricter figure: the kernel stores 34 of the 96 scalars of a step (the rest are structural
                # constants).  The SURVEY 8(d) figure on ALGORITHMIC bytes (dense: 880 B per problem-step + 352 B per problem) is
                # achieved_algorithmic / frac_algorithmic.  Without a traffic record the top-level pair falls back to the dense
                # bytes and says so in achieved_basis.
                "achieved": own["achieved_real"] if own["achieved_real"] is not None else own["achieved"],
                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": own["frac"] if own["frac"] is not None else own["frac_algorithmic"],
                "achieved_basis": ("HBM bytes really moved: PMC bytes per problem-step x problem-steps of these launches" if own["frac"] is not None
                                   else "ALGORITHMIC (dense) bytes: no traffic record for this workload"),
                "achieved_algorithmic": own["achieved"],
                "frac_algorithmic": own["frac_algorithmic"],
                "frac_full_batch": (round(gbs(real_full, full_alone_ms * 1e-3) / HBM_PEAK_GBS, 4) if (real_full and full_alone_ms) else None),
                "frac_full_batch_algorithmic": (round(gbs(B * per_problem, full_alone_ms * 1e-3) / HBM_PEAK_GBS, 4) if full_alone_ms else None),
                "frac_contended": contended["frac"], "frac_contended_algorithmic": contended["frac_algorithmic"],
                "bytes_per_problem_step": round(bps, 1) if bps else None,
                "bytes_per_problem_step_full_batch_launch": (round(rec["full_batch_launch"]["hbm_bytes_per_problem_step"], 1) if rec else None),
                "bytes_per_problem_step_minimum": api.REAL_BYTES_PER_STEP,
                "bytes_per_problem_step_algorithmic": api.DENSE_DOUBLES_PER_STEP * 8,
                # HBM bytes per launch from the PMC counters of THIS run (null when the counter passes could not run; frac then
                # rests on the bytes recorded under profiles/, see traffic_recorded)
                "traffic": own["traffic"],
                "algorithmic_bytes_per_launch": own["alg_per_launch"],
                "avg_launch_ms": own["avg_launch_ms"], "launches": own["launches"],
                "mean_problems_per_launch": own["mean_problems_per_launch"],
                "full_batch_avg_launch_ms": full_alone_ms,
                "avg_launch_ms_contended": contended["avg_launch_ms"], "launches_contended": contended["launches"],
                "batches_in_flight_contended": P * D,
                "traffic_measured": traffic,
                "traffic_recorded": ({"bytes_per_launch": own["real_per_launch"], "bytes_per_problem_step": bps,
                                      "source": os.path.relpath(args.traffic_file, ROOT)} if (rec and not traffic) else None),
                "contended": contended,
            }
            try:   # fp64-issue / stall record of the other kernels (rocprofv3 PMC, tools/kernel_rooflines.py): recorded, not measured here
                import glob as _glob
                kr_path = sorted(_glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_kernel_rooflines.json")))[-1]   # the latest round's record
                with open(kr_path) as f:
                    kr = json.load(f)
                if args.scene == "mix11" and N == 50 and B == 65536:
                    roof["other_kernels_recorded"] = {
                        "source": f"profiles/{os.path.basename(kr_path)} (separate rocprofv3 --pmc passes of this workload, one batch in flight)",
                        "kernels": {k: {f: v[f] for f in ("ms_per_solve", "bound", "valu_issue_frac", "hbm_frac", "wait_share", "valu_per_wave") if f in v}
                                    for k, v in kr["kernels"].items()
                                    if k.split("<")[0] in ("k_round_cost", "k_spec_cost", "k_spec_cost_packed", "k_quadratize", "k_multi_forward_packed", "k_multi_forward", "k_tail")}}
            except Exception:
                pass
            if prof_acc["full_launches"] > 0:
                t_full = prof_acc["full_ms"] / prof_acc["full_launches"] * 1e-3
                fb = B * per_problem / t_full / 1e9
                roof["full_batch"] = {
                    "kernel": "cilqr::k_backward", "launch": f"all {B} problems of the batch (one launch per solve)",
                    "achieved_alone": (round(gbs(B * per_problem, full_alone_ms * 1e-3), 1) if full_alone_ms else None),
                    "frac_alone": roof["frac_full_batch"], "frac_algorithmic_alone": roof["frac_full_batch_algorithmic"],
                    "avg_launch_ms_alone": full_alone_ms,
                    "achieved_contended": round(fb, 1),
                    "frac_contended": round(real_full / t_full / 1e9 / HBM_PEAK_GBS, 4) if real_full else None,
                    "frac_algorithmic_contended": round(fb / HBM_PEAK_GBS, 4),
                    "traffic_bytes_per_launch": real_full,
                    "algorithmic_bytes_per_launch": B * per_problem, "avg_launch_ms_contended": t_full * 1e3,
                    "launches_contended": prof_acc["full_launches"],
                    "note": "alone: the launch with nothing else in flight (calibration step); contended: HIP events in the timed "
                            "region, where other batches' kernels share the GPU",
                }
        cpu = None
        if args.full and args.cpu_sample > 0 and world == 1:   # rank 0 at N = 1 only
            from oracle import oracle as orc

            def ocfg_for(n_steps):
                c = api.default_config(n_steps)
                o = orc.OracleConfig()
                for name, _ in orc.OracleConfig._fields_:
                    setattr(o, name, getattr(c, name))
                return o

            ns = min(args.cpu_sample, B)
            sub = {k: (v[:ns] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in sc.items()}
            r = orc.solve_batch(sub, ocfg_for(N), want_margin=False)
            cpu = {"value": round(ns / r["seconds"], 2), "unit": "solves/s", "cores": 1, "kind": "port",
                   "sample": f"first {ns} scenes of rank 0's batch, single thread, g++ -O2 restatement "
                             f"(oracle/cilqr_oracle.cc), {r['seconds']:.1f} s",
                   "nproc": os.cpu_count()}
            # SURVEY 8(d), optional: the same restatement on all cores of the box -- the C library's own threaded loop
            # (oracle_solve_batch_threads: contiguous slices, one solver object per thread) over the whole batch --
            # labelled separately, never `value`
            try:
                # the cores this process may really use: the cgroup's CPU quota when there is one (the GPU boxes show 256
                # logical CPUs and allow 16 cores' worth of time; 256 threads under that quota are slower than 32)
                quota = None
                try:
                    q_, p_ = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
                    quota = None if q_ == "max" else max(1, int(round(int(q_) / int(p_))))
                except Exception:   # noqa: BLE001
                    quota = None
                ncpu = os.cpu_count() or 1
                nthr = max(1, min(ncpu, 2 * quota) if quota else ncpu)
                na = min(B, 16384)
                sub_a = {k: (v[:na] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in sc.items()}
                ra = orc.solve_batch_threads(sub_a, ocfg_for(N), threads=nthr)
                cpu["all_cores"] = {"value": round(na / ra["seconds"], 1), "unit": "solves/s", "threads": nthr,
                                    "cpu_quota_cores": quota, "logical_cpus": ncpu,
                                    "sample": f"first {na} scenes of rank 0's batch on {nthr} host threads inside the C library "
                                              f"(std::thread, contiguous slices), {ra['seconds']:.1f} s wall"}
            except Exception as e:   # noqa: BLE001
                cpu["all_cores"] = {"error": repr(e)}
            if args.cpu_configs > 0:
                # per scene family of the BASELINE configs, >= 256 scenes, per-solve times
                per = {}
                for fam in ("ped6", "mix11", "dyn20"):
                    scf = scenario.generate(fam, args.cpu_configs, seed=100 + args.seed, workers=workers)
                    rf = orc.solve_batch(scf, ocfg_for(scf["n_steps"]), want_margin=False, want_times=True, want_trace=True)
                    ms = rf["problem_seconds"] * 1e3
                    # trials of an iteration: index of the accepted step size + 1, or all eleven
                    trials = [int((a[a >= 0] + 1).sum() + 11 * (a == -1).sum()) for a in rf["alpha_trace"]]
                    per[fam] = {"scenes": int(args.cpu_configs), "n_steps": int(scf["n_steps"]),
                                "mean_ms": round(float(ms.mean()), 3), "median_ms": round(float(np.median(ms)), 3),
                                "p95_ms": round(float(np.quantile(ms, 0.95)), 3),
                                "solves_per_s": round(float(1e3 / ms.mean()), 2),
                                "mean_accepted_iterations": round(float((rf["n_cost"] - 1).mean()), 2),
                                "mean_line_search_trials": round(float(np.mean(trials)), 2)}
                cpu["per_config"] = per
            if latency:   # the CPU restatement on the scenes of the latency section, one solve at a time
                for fam, rec in latency.items():
                    if not isinstance(rec, dict) or "_scene" not in rec:
                        continue
                    scf = rec["_scene"]
                    rf = orc.solve_batch(scf, ocfg_for(scf["n_steps"]), want_margin=False, want_times=True)
                    ms = rf["problem_seconds"] * 1e3
                    rec["cpu_restatement"] = {"mean_ms": round(float(ms.mean()), 3), "median_ms": round(float(np.median(ms)), 3),
                                              "p95_ms": round(float(np.quantile(ms, 0.95)), 3), "threads": 1}
        out = {
            "metric": f"CILQR solves/sec ({N}-step horizon, batch={B} per GPU)",
            "value": round(value, 1), "unit": "solves/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BASELINE {WORKLOADS.get((args.scene, B), 'custom')}: batch={B}/GPU x {world} GPU, "
                                   f"{N}-step horizon, scene family {args.scene} ({spec.n_pedestrians} pedestrians + "
                                   f"{spec.n_dynamic} moving + {spec.n_static} static vehicles), reference road, "
                                   f"seed {args.seed}",
                       "batch_per_gpu": B, "n_steps": N, "cmax": cmax, "batches_in_flight": P * D, "handles": P, "in_flight_per_handle": D,
                       "exact_lane_ties": not args.fast_lane_ties,
                       "backward_thresholds": {"team": thr_team, "wave": thr_wave},     # cilqr_get_option: what the library holds
                       "coarse_trajectories": ("DP coarse planner (cilqr_dp_plan) + cilqr_build_corridors" if dp_info else "scene generator"),
                       "dp_scene_source": dp_info,
                       "results_gather": ("rccl" if use_rccl else "peer copies (one process, --multi)" if comm is not None else "none"),
                       "rccl_ranks": rccl_ranks, "processes": 1 if comm is not None else world},
            "roofline": roof,
            "cpu_baseline": cpu,
            "single_batch": ({"value": round(B / seq, 1), "unit": "solves/s", "ms_per_step": round(seq * 1e3, 3),
                              "note": "one batch in flight: the same solve called back to back, nothing overlapped"}
                             if seq else None),
            "one_handle": one_handle,
            "results_identical_across_solves_in_flight": same,
            "c_abi_gather": cabi,
            # every rank's own figures (the line's ms_per_step is their maximum) and the check that block r of the last gathered
            # step on rank 0 is rank r's result (a 64-bit position-dependent checksum computed where the result was produced)
            "per_rank": ({"ms_per_step": [round(1e3 * p_[0] / args.steps, 3) for p_ in per_rank],
                          "gather_thread_busy_ms_per_step": [round(1e3 * p_[2] / args.steps, 3) for p_ in per_rank]} if use_dist else None),
            "gather_verified_ranks": gather_verified,
            "results_gather_carrier": (args.gather if use_rccl else None),
            "results_gather_thread": ({"gathers": gather_timed["count"],
                                       "busy_ms_per_gather": round(1e3 * gather_timed["busy_s"] / max(1, gather_timed["count"]), 3),
                                       "note": "rank 0's gather thread (own stream): pack, agree on the ragged length, RCCL gather, unpack "
                                               "world x the payload; overlapped with the next steps' solves"} if use_dist else None),
            # the two figures a caller sees whose arrays are not already in HBM (never `value`)
            "pcie_inclusive": pcie,
            "end_to_end": end_to_end,
            # drop-in latency (never `value`): Plan through the C++ adapter with a batch of one, and small host batches
            "latency": ({fam: ({k: v for k, v in rec.items() if k != "_scene"} if isinstance(rec, dict) else rec)
                         for fam, rec in latency.items()} if latency else None),
            # per-phase HIP-event times of the calibration step (one batch alone, events around every phase)
            # quad / bwd / ls / other: the lockstep iterations; tail: the per-problem kernel that finishes the
            # last `tail_problems` problems in one launch (CILQR_OPT_TAIL_THRESHOLD)
            "breakdown_ms_per_step": ({**{k: round(single[k], 3) for k in ("quad_ms", "bwd_ms", "ls_ms", "other_ms", "tail_ms", "total_ms")},
                                       "tail_problems": single["tail_problems"], "lockstep_iterations": single["lockstep_launches"]}
                                      if single else None),
            "iterations_per_step": prof_acc["iters"] / args.steps if prof_acc["iters"] else (single or {}).get("iterations"),
            "mean_cost_rows": float(nc.mean()),
            "status_histogram": np.bincount(st, minlength=7).tolist(),
            "scene_generation_s": round(t_gen, 1),
            "device_bytes": dev_bytes_timed,
            "host": host,
        }
    if hung:   # a stuck collective cannot be torn down: print the line and leave
        if rank == 0:
            os.write(real_stdout, (json.dumps(out) + "\n").encode())
        os._exit(0)
    for c in ctx:
        c.opt.close()    # wrappers of the pool's handles: nothing destroyed here
    pool.close()
    if gatherer is not None:
        gatherer.close()
    if cabi_handle is not None:      # (after the last leg that gathers: the one-handle leg of a one-rank rehearsal still does)
        cabi_handle.comm_destroy()
        cabi_handle.close()
    if use_rccl:
        dist.barrier()
        dist.destroy_process_group()
    elif comm is not None:
        comm.barrier()
    if rank == 0:
        try:  # flush what native libraries left in the C stdio buffer (to stderr), then the JSON line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())


if __name__ == "__main__":
    main()
