"""cilqr_policy_gains_batch / cilqr_policy_rollout_batch (include/cilqr.h, "policy") without a GPU: the declarations, the
exports, the NULL-handle refusals, and the rule of the rollout as cilqr_amd/policy.py states it -- against the long-double
Forward of tests/riccati_reference.py (from goals[0] and from a perturbed start) and on a hand-made three-step case with a
clamp on both sides, a NaN control and the three summaries.  The kernels themselves: tests/test_gpu_policy.py."""
import re

import numpy as np
import pytest

import riccati_reference as rr
from stage_reference import LD
from cilqr_amd import api, policy


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def test_header_declares_the_policy_calls():
    text = open(api.HEADER_PATH).read()
    assert re.search(r"^int cilqr_policy_gains_batch\(cilqr_handle h, const cilqr_problem_batch\* in, int32_t layout,", text, re.M)
    assert re.search(r"^int cilqr_policy_rollout_batch\(cilqr_handle h, int32_t batch, int32_t layout,", text, re.M)
    m = re.search(r"^#define CILQR_POLICY_MAX_SAMPLES (\d+)", text, re.M)
    assert m and int(m.group(1)) == 256 == api.POLICY_MAX_SAMPLES
    assert re.search(r"^#define CILQR_ABI_VERSION 7$", text, re.M)


def test_library_exports_the_policy_calls_at_abi_7():
    L = api.lib()
    assert L.cilqr_abi_version() == 7 == api.ABI_VERSION
    for name in ("cilqr_policy_gains_batch", "cilqr_policy_rollout_batch"):
        assert name in api.EXPORTS and hasattr(L, name)


def test_null_handle_is_refused():
    L = api.lib()
    a = np.zeros(64)
    p = api._ptr(a)
    prob = api.ProblemBatch()
    assert L.cilqr_policy_gains_batch(None, prob, api.ROWS_TRAJ, p, None, p, p, None, None) == api.ERR_NULL
    assert L.cilqr_policy_rollout_batch(None, 1, api.ROWS_TRAJ, p, 2, p, None, 0.0, 1, p, 0, 2, p, None, None, None,
                                        api.MEM_HOST) == api.ERR_NULL


# ---------------------------------------------------------------------------------------------
# the statement against the long-double Forward
class _Cfg:
    dt, wheel_base = 0.1, 2.8


def _crafted(B=5, N=7, seed=3):
    """a small problem: a gently curving nominal, gains of the size a solve produces, feed-forward terms"""
    r = np.random.default_rng(seed)
    X = np.zeros((B, N + 1, 6))
    X[:, :, 0] = np.linspace(0, 4, N + 1)[None] + r.normal(0, 0.1, (B, 1))
    X[:, :, 1] = r.normal(0, 0.3, (B, 1)) + 0.05 * np.arange(N + 1)[None]
    X[:, :, 2] = r.uniform(-0.4, 0.4, (B, 1)) + 0.01 * np.arange(N + 1)[None]
    X[:, :, 3] = r.uniform(2, 8, (B, 1))
    X[:, :, 4] = r.normal(0, 0.3, (B, N + 1))
    X[:, :, 5] = r.normal(0, 0.05, (B, N + 1))
    U = r.normal(0, 0.5, (B, N, 2)) * np.array([1.0, 0.1])
    K = r.normal(0, 1.0, (B, N, 2, 6)) * np.array([1.0, 0.2])[None, None, :, None]
    k = r.normal(0, 0.2, (B, N, 2))
    return X, U, K, k


def _rows_of(X, U, layout):
    xc, uc, F = policy.COLUMNS[layout]
    rows = np.full((X.shape[0], X.shape[1], F), np.nan)
    rows[:, :, xc] = X
    rows[:, :-1, uc] = U
    return rows


def _rr_step(cfg):
    """the step of rr.forward: x + dt f(x + dt / 2 f(x, u), u), theta and delta wrapped"""
    dt, Lw = LD(cfg.dt), LD(cfg.wheel_base)

    def step(i, x, u):
        shape = x.shape
        x, u = x.reshape(-1, 6), u.reshape(-1, 2)
        mid = x + dt / 2 * rr._f(x, u, Lw)
        nxt = x + dt * rr._f(mid, u, Lw)
        nxt[:, 2], nxt[:, 5] = rr.wrap(nxt[:, 2]), rr.wrap(nxt[:, 5])
        return nxt.reshape(shape)
    return step


@pytest.mark.parametrize("layout", [api.ROWS_TRAJ, api.ROWS_PLAN])
@pytest.mark.parametrize("alpha", [1.0, 0.2512, 0.0])
def test_statement_reproduces_the_long_double_forward(layout, alpha):
    """x0 = goals[0] (the nominal's first state) and a start perturbed in all six components: states and controls of the
    statement in long double against rr.forward.  The two differ by the order of a six-term sum only: 1e-15."""
    cfg = _Cfg()
    X, U, K, k = _crafted()
    B, N = U.shape[:2]
    off = np.array([0.3, -0.2, 0.05, 0.5, 0.2, 0.02])
    starts = np.stack([X[:, 0], X[:, 0] + off, X[:, 0] - off])
    got = policy.rollout(_rows_of(X, U, layout), layout, K, starts, _rr_step(cfg), cfg.dt, cfg.wheel_base, kff=k, alpha=alpha,
                         dtype=LD)
    for s in range(3):
        Xn, Un = rr.forward(alpha, starts[s], X, U, K, k, cfg)
        assert np.abs(got["rows"][s, :, :, 1:7] - Xn).max() < 1e-15
        assert np.abs(got["rows"][s, :, :N, 8:10] - Un).max() < 1e-15
    assert np.all(got["rows"][:, :, N, 8:10] == 0) and np.all(got["n_clamped"] == 0)
    assert np.all(got["rows"][:, :, :, 0] == (np.arange(N + 1).astype(LD) * LD(cfg.dt))[None, None])
    assert np.all(got["max_dev"][0] >= got["end_dev"][0])
    assert np.all(got["max_dev"][1] >= np.hypot(0.3, 0.2) * (1 - 1e-15))


def test_without_feed_forward_alpha_is_not_read():
    cfg = _Cfg()
    X, U, K, k = _crafted()
    rows = _rows_of(X, U, api.ROWS_TRAJ)
    a = policy.rollout(rows, api.ROWS_TRAJ, K, X[None, :, 0] + 0.1, _rr_step(cfg), cfg.dt, cfg.wheel_base, alpha=0.7)
    b = policy.rollout(rows, api.ROWS_TRAJ, K, X[None, :, 0] + 0.1, _rr_step(cfg), cfg.dt, cfg.wheel_base, kff=np.zeros_like(k),
                       alpha=1.0)
    assert np.array_equal(a["rows"], b["rows"])


def test_clamp_and_summaries_on_a_hand_made_case():
    """One problem, three steps, K = 0 except one entry, so every control is known by hand:
         u_i = u*_i + K_i[.][0] (x_i - x*_i),  the step moves x by +1 and leaves the rest (a stand-in for the dynamics).
       sample 0 starts 2 m ahead, sample 1 on the nominal.  Bounds: jerk in [-1, 1], rate in [-0.5, 0.5]."""
    N = 3
    X = np.zeros((1, N + 1, 6))
    X[0, :, 0] = [0.0, 1.0, 2.0, 3.0]
    U = np.array([[[0.5, 0.1], [0.9, -0.4], [np.nan, 0.0]]])
    K = np.zeros((1, N, 2, 6))
    K[0, 0, 0, 0] = 1.0      # step 0: jerk = 0.5 + 2 = 2.5 -> clamped to 1 (sample 0); 0.5 on the nominal
    K[0, 1, 1, 0] = -1.0     # step 1: rate = -0.4 - 2 = -2.4 -> clamped to -0.5 (sample 0); -0.4 on the nominal
    rows = _rows_of(X, U, api.ROWS_TRAJ)
    start = np.zeros((2, 1, 6))
    start[0, 0, 0] = 2.0
    start[0, 0, 1] = 1.5     # 1.5 m beside the nominal as well

    def step(i, x, u):
        xn = x.copy()
        xn[..., 0] += 1.0
        xn[..., 1] *= 0.5
        return xn
    got = policy.rollout(rows, api.ROWS_TRAJ, K, start, step, 0.1, 2.8, bounds=(-1.0, 1.0, -0.5, 0.5))
    u = got["rows"][:, 0, :, 8:10]
    wrapped = lambda v: float(policy.normalize_angle(np.float64(v)))      # noqa: E731  (v + pi) - pi: v to a few ulps of pi
    assert np.array_equal(u[0, 0], [1.0, wrapped(0.1)]) and np.array_equal(u[1, 0], [0.5, wrapped(0.1)])
    assert u[0, 1, 0] == 0.9 and u[0, 1, 1] == wrapped(-0.5) and u[1, 1, 1] == wrapped(-0.4)
    assert abs(wrapped(-0.5) + 0.5) < 1e-15
    assert np.isnan(u[0, 2, 0]) and np.isnan(u[1, 2, 0])          # a NaN passes the clamp ...
    assert list(got["n_clamped"][:, 0]) == [2, 0]                   # ... and is no clamped step
    assert np.all(u[:, 3] == 0.0)
    # deviations of sample 0: (2, 1.5) (2, .75) (2, .375) (2, .1875)
    assert got["max_dev"][0, 0] == np.sqrt(2.0 * 2.0 + 1.5 * 1.5) and got["end_dev"][0, 0] == np.sqrt(2.0 * 2.0 + 0.1875 * 0.1875)
    assert got["max_dev"][1, 0] == 0.0 and got["end_dev"][1, 0] == 0.0
    # without bounds nothing is clamped; n_out = 2 records two rows, the second with controls (0, 0), summaries over those two
    free = policy.rollout(rows, api.ROWS_TRAJ, K, start, step, 0.1, 2.8, n_out=2)
    assert free["rows"].shape == (2, 1, 2, 10) and np.array_equal(free["rows"][0, 0, 0, 8:10], [2.5, wrapped(0.1)])
    assert np.all(free["rows"][:, 0, 1, 8:10] == 0.0) and np.all(free["n_clamped"] == 0)
    assert free["end_dev"][0, 0] == np.sqrt(2.0 * 2.0 + 0.75 * 0.75)
    # a NaN deviation stays in max_dev
    start[1, 0, 1] = np.nan
    nan = policy.rollout(rows, api.ROWS_TRAJ, K, start, step, 0.1, 2.8)
    assert np.isnan(nan["max_dev"][1, 0]) and not np.isnan(nan["max_dev"][0, 0])
    alone = policy.rollout(rows, api.ROWS_TRAJ, K, start[:1], step, 0.1, 2.8)
    assert np.array_equal(nan["rows"][0].view(np.int64), alone["rows"][0].view(np.int64))
