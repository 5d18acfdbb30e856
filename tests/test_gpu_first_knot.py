"""The first-knot cache and the fused first evaluation change no bit of any result.

A solve never moves knot 0 (every rollout starts from goals[0]), so the cost kernels of the line search copy that knot's
state terms from a cache the first cost evaluation fills (DeviceState::knot0) and evaluate only the control's pair; the first
iterate is costed and quadratised in one pass (k_quadratize_first).  Both
are the same expressions on the same operands in the same order.  Two hooks read at cilqr_create -- CILQR_NO_KNOT0_CACHE,
CILQR_NO_FUSED_FIRST -- give a handle that evaluates everything the long way; every test here solves the same problems on
such a handle and on a default one and compares traj, the live rows of cost_hist, n_cost, status, n_iter and alpha_trace bit
for bit (row 0 of cost_hist and iteration 1's accepted step size come from the fused kernel).

Run as a script (`python tests/test_gpu_first_knot.py child scenes.npz`) it is the child process of
test_four_row_arena_and_multi_pass_remainder: the pass size of the re-strided candidate arena is read once per process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cilqr_amd import api, scenario  # noqa: E402

pytestmark = pytest.mark.gpu
HOOKS = ("CILQR_NO_KNOT0_CACHE", "CILQR_NO_FUSED_FIRST")
KEYS = ("traj", "n_cost", "status", "n_iter", "alpha_trace")


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _handle(sc, plain, opts=None, B=None, **cfg_over):
    """plain: both hooks set while the handle is created (they are read there and nowhere else)."""
    old = {k: os.environ.pop(k, None) for k in HOOKS}
    if plain:
        for k in HOOKS:
            os.environ[k] = "1"
    try:
        opt = api.BatchIlqrOptimizer(api.default_config(sc["n_steps"], **cfg_over), batch_capacity=B or sc["coarse"].shape[0],
                                     cmax=sc["cmax"])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    for k, v in (opts or {}).items():
        opt.set_option(k, v)
    return opt


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_same(got, ref, what):
    assert (ref["status"] != api.ST_RUNNING).all(), what
    for k in KEYS:
        assert got[k].shape == ref[k].shape and _bits(got[k]) == _bits(ref[k]), f"{what}: {k} differs"
        assert np.array_equal(got[k], ref[k], equal_nan=True), f"{what}: {k} differs"
    nc = ref["n_cost"]
    live = np.arange(ref["cost_hist"].shape[1])[None, :] < nc[:, None]
    assert _bits(got["cost_hist"][live]) == _bits(ref["cost_hist"][live]), f"{what}: live cost_hist rows differ"
    assert np.array_equal(got["cost_hist"][live], ref["cost_hist"][live], equal_nan=True), f"{what}: live cost_hist rows differ"


def _solve(opt, sc, road="plan", warm=None):
    if road == "submit":
        return opt.collect(opt.submit(sc, max_iter_trajs=3, alpha_trace=True, warm=warm))
    return opt.plan(sc, max_iter_trajs=3, alpha_trace=True, warm=warm)


def _compare(sc, what, opts=None, road="plan", warm=None, **cfg_over):
    """The same solve on a handle with both hooks off and on a default one; returns the default handle's result."""
    res = []
    for plain in (True, False):
        opt = _handle(sc, plain, opts, **cfg_over)
        res.append(_solve(opt, sc, road, warm))
        opt.close()
    _assert_same(res[1], res[0], what)
    return res[1]


# Lockstep schedules a batch of a few hundred does not reach with the default thresholds.  "default" sends all 192 problems
# straight to the tail kernel: no fused pass (job_begin keeps the separate kernels then) and a tail view without the cache, so
# that case holds only the cache's fill in k_cost_knots; the other three do the real checking of the short paths and the fusion.
SCHEDULES = {
    "default": {},                                                                        # straight to the tail kernel
    "speculative, then the tail": {api.OPT_TAIL_THRESHOLD: 24},                           # all eleven step sizes at once, re-packing
    "rounds + remainder, then the tail": {api.OPT_SPEC_THRESHOLD: 0, api.OPT_TAIL_THRESHOLD: 24},   # k_round_cost, k_spec_cost_packed
    "round-by-round rollouts": {api.OPT_SPEC_THRESHOLD: 0, api.OPT_SEQ_ROUNDS: 6, api.OPT_TAIL_THRESHOLD: 0},   # k_cost_knots on candidates
}


@pytest.fixture(scope="module")
def scenes192():
    return scenario.generate("mix11", 192, seed=711)


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_solve_batch(scenes192, schedule):
    g = _compare(scenes192, schedule, SCHEDULES[schedule])
    assert (g["n_iter"] > 1).sum() > 96 and (g["alpha_trace"][:, 0] >= 0).sum() > 96      # real solves, first steps accepted


def test_four_row_arena_and_multi_pass_remainder(scenes192, tmp_path):
    """CILQR_SPEC_ROWS=4 with passes of 8 entries: the four-row candidate arena and its multi-pass remainder (a child process:
    the pass size is read once per process)."""
    path = str(tmp_path / "scenes.npz")
    sc = scenes192
    np.savez(path, n_steps=sc["n_steps"], cmax=sc["cmax"], **{k: sc[k] for k in ("start", "coarse", "corridor", "ccount", "left", "right")})
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path],
                       env=dict(env, CILQR_SPEC_ROWS="4", CILQR_SPEC_PASS_ENTRIES="8"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["problems"] == 192
    print(rep)


@pytest.mark.parametrize("tail", [None, 16])
def test_submit_and_hand_over_to_the_finishing_arena(scenes192, tail):
    """cilqr_submit / cilqr_wait with the hand-over at 100 problems: the finishing arena receives the cache with the survivors
    (tail 16: and keeps iterating on it in lockstep; default: the tail kernel takes over there)."""
    opts = {api.OPT_FINISH_THRESHOLD: 100}
    if tail is not None:
        opts[api.OPT_TAIL_THRESHOLD] = tail
    g = _compare(scenes192, f"submit, tail {tail}", opts, road="submit")
    ref = _handle(scenes192, True, {api.OPT_TAIL_THRESHOLD: 0})
    _assert_same(g, _solve(ref, scenes192), "submitted against the synchronous lockstep solve")
    ref.close()


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("tail", [None, 0])
def test_batch_of_one_and_partial_wave(B, tail):
    sc = scenario.generate("mix11", B, seed=712 + B)
    _compare(sc, f"B = {B}, tail {tail}", {} if tail is None else {api.OPT_TAIL_THRESHOLD: tail})


@pytest.mark.parametrize("tail", [None, 0])
def test_hostile_problems_and_a_single_plane(tail):
    """One problem without a corridor (negative count: status 6), one knot without planes, one live plane with a NaN
    coefficient -- inside a batch; and the same batch cut down to cmax = 1."""
    opts = {} if tail is None else {api.OPT_TAIL_THRESHOLD: tail}
    sc = scenario.generate("mix11", 70, seed=713)
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    assert sc["ccount"][20, 0] >= 1 and sc["ccount"][21, 30] >= 1 and sc["ccount"][9, 0] >= 1
    sc["ccount"][3, 0] = -2            # knot 0 itself: the cache's fill sees it
    sc["ccount"][40, 17] = -1
    sc["ccount"][9, 0] = 0             # no planes at the cached knot
    sc["ccount"][9, 25] = 0
    sc["corridor"][20, 0, 0, 1] = np.nan   # live plane of knot 0
    sc["corridor"][21, 30, 0, 0] = np.nan
    g = _compare(sc, f"hostile, tail {tail}", opts)
    assert g["status"][3] == api.ST_NO_CORRIDOR and g["status"][40] == api.ST_NO_CORRIDOR
    assert not np.isfinite(g["cost_hist"][20, 0, 0]) and not np.isfinite(g["cost_hist"][21, 0, 0])
    one = dict(sc, corridor=np.ascontiguousarray(sc["corridor"][:, :, :1, :]), ccount=np.minimum(sc["ccount"], 1), cmax=1)
    _compare(one, f"cmax = 1, tail {tail}", opts)


@pytest.mark.parametrize("tail", [None, 0])
def test_warm_start_with_mixed_shifts(tail):
    opts = {} if tail is None else {api.OPT_TAIL_THRESHOLD: tail}
    sc = scenario.generate("mix11", 96, seed=714)
    cold = _handle(sc, True)
    rows = np.ascontiguousarray(cold.plan(sc)["traj"])
    cold.close()
    shift = np.resize(np.asarray([0, -1, 3, 0, sc["n_steps"] + 1, 1, 0, -1, 0, 12, 0], np.int32), 96)
    _compare(sc, f"warm, mixed shifts, tail {tail}", opts, warm=(rows, shift, api.ROWS_TRAJ))
    _compare(sc, f"warm, no shifts, tail {tail}", opts, warm=(rows, None, api.ROWS_TRAJ))


@pytest.mark.parametrize("schedule", ["default", "rounds + remainder, then the tail", "round-by-round rollouts"])
def test_three_discs_take_the_generic_kernels(schedule):
    sc = scenario.generate("mix11", 80, seed=715)
    _compare(sc, f"num_of_disc = 3, {schedule}", SCHEDULES[schedule], num_of_disc=3)


def _child_main(path):
    assert os.environ.get("CILQR_SPEC_ROWS") == "4" and os.environ.get("CILQR_SPEC_PASS_ENTRIES")
    z = np.load(path)
    sc = {k: z[k] for k in ("start", "coarse", "corridor", "ccount", "left", "right")}
    sc.update(n_steps=int(z["n_steps"]), cmax=int(z["cmax"]))
    out = {}
    for name, opts in (("rounds + remainder", {api.OPT_SPEC_THRESHOLD: 0, api.OPT_TAIL_THRESHOLD: 0}),
                       ("default thresholds, lockstep", {api.OPT_TAIL_THRESHOLD: 0}),
                       ("default", {}),
                       ("round-by-round rollouts", {api.OPT_SPEC_THRESHOLD: 0, api.OPT_SEQ_ROUNDS: 6, api.OPT_TAIL_THRESHOLD: 0})):
        g = _compare(sc, f"four rows: {name}", opts)
        out[name] = int((g["alpha_trace"] >= 4).sum())
    print(json.dumps({"ok": True, "problems": int(sc["start"].shape[0]), "accepted_beyond_four_rounds": out}))


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "child"
    _child_main(sys.argv[2])
