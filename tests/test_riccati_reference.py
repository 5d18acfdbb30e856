"""The double-precision oracle's Backward, CalGradientNorm and Forward held against their long-double restatement
(tests/riccati_reference.py), and that statement against a third form in exact rational arithmetic.  No GPU.

Inputs (tests/riccati_cases.py): the crafted table under every configuration at lambda 0 .. 1e11, and generated scenes at the
horizons 1 .. 5, 50, 64, 65, 130 from the init guess.  Bounds: parity_util.rel_err with the floor 1e-6 (backward) and
test_gpu_stages' measure (forward) below STAGE_TOL / 4 -- for every problem up to N = 50 and every tame rollout; at N >= 64 the
double recursion itself drifts, so an eighth of the (problem, lambda) pairs may lie beyond, none beyond STEP_TOL = 1e-8.  The
measured worst figures (printed by the tests): DESIGN.md, section 5."""
from fractions import Fraction

import numpy as np
import pytest

import riccati_cases as rc
import riccati_reference as rr
import stage_cases as sc
from oracle import oracle as orc

HORIZONS = (1, 2, 3, 4, 5, 50, 64, 65, 130)
FAMILIES = ("mix11", "dyn20x")
PER_FAMILY = 12
TIGHT = rc.STAGE_TOL / 4


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    orc.lib()


# ---------------------------------------------------------------------------------------------
# inputs and the oracle's results on them, computed once and left unchanged
# ---------------------------------------------------------------------------------------------
_INPUTS, _BACKWARD, _FORWARD = {}, {}, {}


def _oracle_for(cfg, scene, b):
    o = orc.Oracle(cfg)
    assert o.set_problem(scene["start"][b], scene["coarse"][b], scene["corridor"][b], scene["ccount"][b], scene["left"], scene["right"]) == 0
    return o


def inputs(key):
    """key: ("table", configuration) or ("horizon", N) -> dict(cfg, scene, X, U, q, goals, lambdas, n_steps)"""
    if key in _INPUTS:
        return _INPUTS[key]
    if key[0] == "table":
        g = sc.evaluate(key[1])[sc.MAIN_CMAX]
        out = dict(cfg=g["cfg"], scene=g["scene"], X=g["X"], U=g["U"], goals=g["goals"], lambdas=rc.TABLE_LAMBDAS, n_steps=sc.N_STEPS,
                   q={k: g["oracle"][k] for k in ("A", "B", "lx", "lu", "lxx", "luu")})
    else:
        n = key[1]
        cfg = orc.default_config(n)
        parts = []
        for f, name in enumerate(FAMILIES):
            scene = rc.horizon_scene(name, n, PER_FAMILY, seed=rc.HORIZON_SEED + 10 * n + f)
            for b in range(PER_FAMILY):
                o = _oracle_for(cfg, scene, b)
                X, U = o.init_guess()
                parts.append(dict(scene=scene, b=b, X=X, U=U, q=o.quadratize(X, U), goals=o.constraints()[0]))
        out = dict(cfg=cfg, parts=parts, X=np.stack([p["X"] for p in parts]), U=np.stack([p["U"] for p in parts]),
                   goals=np.stack([p["goals"] for p in parts]), lambdas=rc.HORIZON_LAMBDAS, n_steps=n,
                   q={k: np.stack([p["q"][k] for p in parts]) for k in ("A", "B", "lx", "lu", "lxx", "luu")})
    _INPUTS[key] = out
    return out


def _oracles(inp):
    B = inp["X"].shape[0]
    if "parts" in inp:
        return [_oracle_for(inp["cfg"], p["scene"], p["b"]) for p in inp["parts"]]
    o = orc.Oracle(inp["cfg"])         # Backward, CalGradientNorm and Forward read goals[0] only: set per problem below
    return [(o, b) for b in range(B)]


def _with(inp, entry):
    if isinstance(entry, tuple):
        o, b = entry
        s = inp["scene"]
        assert o.set_problem(s["start"][b], s["coarse"][b], s["corridor"][b], s["ccount"][b], s["left"], s["right"]) == 0
        return o
    return entry


def backward_report(key):
    """Oracle and statement on every (problem, lambda): dist [B, L, 4] (K, k, dV, gradient norm), the oracle's gains, census."""
    if key in _BACKWARD:
        return _BACKWARD[key]
    inp = inputs(key)
    B, L = inp["X"].shape[0], len(inp["lambdas"])
    N = inp["n_steps"]
    oK, ok_, odV, ogn = np.zeros((B, L, N, 2, 6)), np.zeros((B, L, N, 2)), np.zeros((B, L, 2)), np.zeros((B, L))
    for b, entry in enumerate(_oracles(inp)):
        o = _with(inp, entry)
        qb = {k: v[b] for k, v in inp["q"].items()}
        for l, lam in enumerate(inp["lambdas"]):
            oK[b, l], ok_[b, l], odV[b, l] = o.backward(float(lam), qb)
            ogn[b, l] = o.grad_norm(ok_[b, l], inp["U"][b])
    # the statement: every lambda in one pass (problem axis = lambda-major)
    census = {}
    q = {k: np.concatenate([v] * L) for k, v in inp["q"].items()}
    lam = np.repeat(np.asarray(inp["lambdas"], np.float64), B)
    sK, sk, sdV = rr.backward(lam, q, census=census)
    sgn = rr.grad_norm(sk, np.concatenate([inp["U"]] * L))
    eK, ek, edV = rr.backward(lam, q, eager=True)
    assert np.array_equal(eK, sK) and np.array_equal(ek, sk)                    # the switch touches delta_V only
    dist = np.zeros((B, L, 4))
    for l in range(L):
        for b in range(B):
            j = l * B + b
            dist[b, l, :3] = rc.backward_distance((oK[b, l], ok_[b, l], odV[b, l]), (sK[j], sk[j], sdV[j]))
            dist[b, l, 3] = rc.rel_err(ogn[b, l], float(sgn[j]), 1e-6)
    out = dict(dist=dist, K=oK, k=ok_, census=census)
    _BACKWARD[key] = out
    return out


def forward_report(key):
    """Oracle and statement rollouts at every (problem, forward lambda, step size): tame [B, 2, 11], dist [B, 2, 11], wrap masks."""
    if key in _FORWARD:
        return _FORWARD[key]
    inp, bw = inputs(key), backward_report(key)
    B, A = inp["X"].shape[0], len(rr.ALPHAS)
    ls = [inp["lambdas"].index(lam) for lam in rc.FORWARD_LAMBDAS]
    tame, oX, oU = np.zeros((B, len(ls), A), bool), {}, {}
    for b, entry in enumerate(_oracles(inp)):
        o = _with(inp, entry)
        for j, l in enumerate(ls):
            for a, alpha in enumerate(rr.ALPHAS):
                oX[b, j, a], oU[b, j, a] = o.forward(alpha, inp["X"][b], inp["U"][b], bw["K"][b, l], bw["k"][b, l])
                tame[b, j, a] = rc.tame(oX[b, j, a])
    dist = np.zeros((B, len(ls), A))
    u1, th = np.zeros((B, len(ls), A), bool), np.zeros((B, len(ls), A), bool)
    for j, l in enumerate(ls):
        for a, alpha in enumerate(rr.ALPHAS):
            census = {}
            sX, sU = rr.forward(alpha, inp["goals"][:, 0], inp["X"], inp["U"], bw["K"][:, l], bw["k"][:, l], inp["cfg"], census)
            u1[:, j, a], th[:, j, a] = census["u1_wrapped"], census["theta_wrapped"]
            for b in range(B):
                dist[b, j, a] = rc.forward_distance((oX[b, j, a], oU[b, j, a]), (sX[b], sU[b]))
    out = dict(tame=tame, dist=dist, u1_wrapped=u1, theta_wrapped=th)
    _FORWARD[key] = out
    return out


# ---------------------------------------------------------------------------------------------
# oracle against statement
# ---------------------------------------------------------------------------------------------
def _check_backward(key):
    inp, rep = inputs(key), backward_report(key)
    d = rep["dist"]
    worst = d.max(axis=(0, 1))
    where = np.unravel_index(int(np.argmax(d.max(axis=2))), d.shape[:2])
    print(f"\n[{key}] oracle vs statement, worst rel_err: " + ", ".join(f"{n} {v:.2e}" for n, v in zip(rc.QUANTITIES + ("gnorm",), worst))
          + f"; per lambda: " + ", ".join(f"{lam:g}: {d[:, l].max():.2e}" for l, lam in enumerate(inp["lambdas"]))
          + f" (worst at problem {where[0]}, lambda {inp['lambdas'][where[1]]:g})")
    pair = d.max(axis=2)                                         # [problem, lambda]
    assert (pair < rc.STEP_TOL).all(), (key, float(pair.max()))
    if inp["n_steps"] < rc.LONG:
        assert (pair < TIGHT).all(), (key, float(pair.max()), where)
    else:
        loose = int((pair >= TIGHT).sum())
        print(f"[{key}] {loose} of {pair.size} (problem, lambda) pairs beyond STAGE_TOL / 4")
        assert loose <= rc.LOOSE_CAP * pair.size, (key, loose, pair.size)
    return worst


@pytest.mark.parametrize("name", list(sc.CONFIGS))
def test_oracle_backward_on_the_crafted_table(name):
    _check_backward(("table", name))


@pytest.mark.parametrize("n_steps", HORIZONS)
def test_oracle_backward_at_every_horizon(n_steps):
    _check_backward(("horizon", n_steps))


def _check_forward(key):
    """A rollout is WILD where oracle and statement part (STAGE_TOL / 4 or more): a first-iteration step flung it through a pole
    of tan, where a double and a long-double rollout differ by O(1) and nothing can be asserted.  No tame rollout may be wild,
    and the wild share is capped (riccati_cases.wild_cap)."""
    inp, rep = inputs(key), forward_report(key)
    N = inp["n_steps"]
    tame, d = rep["tame"], rep["dist"]
    wild = d >= TIGHT
    wild_at = sorted({rr.ALPHAS[a] for a in np.nonzero(wild)[2]})
    print(f"\n[{key}] forward, oracle vs statement: {int(tame.sum())} of {tame.size} rollouts tame, worst {d[tame].max() if tame.any() else 0.0:.2e}; "
          f"worst of the others that agree {d[~tame & ~wild].max() if (~tame & ~wild).any() else 0.0:.2e}; {int(wild.sum())} wild"
          + (f" (at step sizes {wild_at})" if wild_at else ""))
    assert not (tame & wild).any(), (key, float(d[tame].max()))
    counted = wild if N < rc.LONG else wild[:, :, [a for a, al in enumerate(rr.ALPHAS) if al <= rc.SMALL_ALPHA]]
    assert int(counted.sum()) <= rc.wild_cap(N, counted.size), (key, int(counted.sum()), counted.size)


@pytest.mark.parametrize("name", list(sc.CONFIGS))
def test_oracle_forward_on_the_crafted_table(name):
    _check_forward(("table", name))


@pytest.mark.parametrize("n_steps", HORIZONS)
def test_oracle_forward_at_every_horizon(n_steps):
    _check_forward(("horizon", n_steps))


def test_census():
    """Everything the statement distinguishes happens somewhere in the inputs."""
    keys = [("table", name) for name in sc.CONFIGS] + [("horizon", n) for n in HORIZONS]
    count = dict(symmetrisation_differs=0, lazy_differs_from_eager=0, u1_wrapped=0, theta_wrapped=0, tame=0, wild=0)
    lambdas, horizons = {}, {}
    for key in keys:
        inp, bw, fw = inputs(key), backward_report(key), forward_report(key)
        for k in ("symmetrisation_differs", "lazy_differs_from_eager"):
            count[k] += bw["census"][k]
        count["u1_wrapped"] += int(fw["u1_wrapped"].sum())
        count["theta_wrapped"] += int(fw["theta_wrapped"].sum())
        count["tame"] += int(fw["tame"].sum())
        count["wild"] += int((fw["dist"] >= TIGHT).sum())
        for lam in inp["lambdas"]:
            lambdas[lam] = lambdas.get(lam, 0) + inp["X"].shape[0]
        horizons[inp["n_steps"]] = horizons.get(inp["n_steps"], 0) + inp["X"].shape[0]
    print("\ncensus: " + ", ".join(f"{k} {v}" for k, v in count.items()) + "; problems per lambda: "
          + ", ".join(f"{k:g}: {v}" for k, v in sorted(lambdas.items())) + "; per N: " + ", ".join(f"{k}: {v}" for k, v in sorted(horizons.items())))
    assert all(v > 0 for v in count.values()), count
    assert set(lambdas) == set(rc.TABLE_LAMBDAS) | set(rc.HORIZON_LAMBDAS) and all(v > 0 for v in lambdas.values())
    assert set(horizons) == set(HORIZONS) | {sc.N_STEPS} and all(v > 0 for v in horizons.values())


def test_the_step_sizes_are_the_line_searchs():
    """ALPHAS equals the kAlpha of search_core.hpp (the only place the kernels keep it), read from the source text."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cilqr_amd", "csrc", "search_core.hpp")
    text = open(path).read()
    body = re.search(r"kAlpha\[kNumAlpha\]\s*=\s*\{([^}]*)\}", text).group(1)
    assert tuple(float(t) for t in body.replace("\n", " ").split(",")) == rr.ALPHAS


# ---------------------------------------------------------------------------------------------
# the third form: the same recursion in exact rational arithmetic
# ---------------------------------------------------------------------------------------------
def _fmat(rows):
    return [[Fraction(v) for v in r] for r in rows]


def _mm(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(len(b))) for j in range(len(b[0]))] for i in range(len(a))]


def _tr(a):
    return [list(r) for r in zip(*a)]


def _add(*ms):
    return [[sum(m[i][j] for m in ms) for j in range(len(ms[0][0]))] for i in range(len(ms[0]))]


def _exact_backward(lam, q, eager):
    """riccati_reference.backward's formulas on one problem, entries Fractions, vectors as one-column matrices."""
    N = len(q["A"])
    Vx, Vxx = q["lx"][N], q["lxx"][N]
    Ks, ks = [None] * N, [None] * N
    dV = [Fraction(0), Fraction(0)]
    for i in range(N - 1, -1, -1):
        A, B, Bt = q["A"][i], q["B"][i], _tr(q["B"][i])
        Qu, Quu, Qux = _add(q["lu"][i], _mm(Bt, Vx)), _add(q["luu"][i], _mm(_mm(Bt, Vxx), B)), _mm(_mm(Bt, Vxx), A)
        m = [[Quu[0][0] + lam, Quu[0][1]], [Quu[1][0], Quu[1][1] + lam]]
        det = m[0][0] * m[1][1] - m[0][1] * m[1][0]
        neg_inv = [[-m[1][1] / det, m[0][1] / det], [m[1][0] / det, -m[0][0] / det]]
        K, k = _mm(neg_inv, Qux), _mm(neg_inv, Qu)
        Ks[i], ks[i] = K, k
        Kt, At, Qxu = _tr(K), _tr(A), _tr(Qux)
        Vx = _add(q["lx"][i], _mm(At, Vx), _mm(_mm(Kt, Quu), k), _mm(Kt, Qu), _mm(Qxu, k))
        Vxx = _add(q["lxx"][i], _mm(_mm(At, Vxx), A), _mm(_mm(Kt, Quu), K), _mm(Kt, Qux), _mm(Qxu, K))
        for c in range(6):
            for r in range(6):
                Vxx[r][c] = (Vxx[r][c] + Vxx[c][r]) / 2
        if not eager:
            Qu, Quu = _add(q["lu"][i], _mm(Bt, Vx)), _add(q["luu"][i], _mm(_mm(Bt, Vxx), B))
        half_k = [[v[0] / 2] for v in k]
        dV[0] += _mm(_tr(k), Qu)[0][0]
        dV[1] += _mm(_mm(_tr(half_k), Quu), k)[0][0]
    return Ks, ks, dV


def _exact_problem():
    """N = 3, every entry a small integer or a dyadic fraction (exactly a double), A and B with the sparsity of the model's."""
    N = 3
    q = dict(A=[], B=[], lx=[], lu=[], lxx=[], luu=[])
    for i in range(N + 1):
        f = lambda a, b=0: Fraction(a + i, 8) + b                                       # noqa: E731
        H = [[Fraction(0)] * 6 for _ in range(6)]
        block = [[3 + i, f(1), -f(2)], [f(1), 2, f(3)], [-f(2), f(3), 4 + i]]
        for r in range(3):
            for c in range(3):
                H[r][c] = Fraction(block[r][c])
            H[3 + r][3 + r] = Fraction(2 + r + i, 2)
        q["lxx"].append(H)
        q["lx"].append(_fmat([[f(1)], [-f(3)], [f(2, 1)], [Fraction(-1, 4)], [f(5)], [Fraction(i - 1, 2)]]))
        if i == N:
            break
        A = [[Fraction(int(r == c)) for c in range(6)] for r in range(6)]
        A[0][2], A[0][3], A[0][4], A[0][5] = -f(3), Fraction(1, 8), Fraction(1, 128), -f(1)
        A[1][2], A[1][3], A[1][4], A[1][5] = f(7), Fraction(1, 16), Fraction(1, 256), f(2)
        A[2][3], A[2][4], A[2][5] = Fraction(1, 32), Fraction(1, 512), f(9)
        A[3][4] = Fraction(1, 8)
        q["A"].append(A)
        Bm = [[Fraction(0)] * 2 for _ in range(6)]
        Bm[2][1], Bm[3][0], Bm[4][0], Bm[5][1] = f(5), Fraction(1, 128), Fraction(1, 8), Fraction(1, 8)
        q["B"].append(Bm)
        q["lu"].append(_fmat([[f(2)], [-f(1, 1)]]))
        q["luu"].append(_fmat([[2 + i, 0], [0, Fraction(5, 2)]]))
    return q


def _to_float(q):
    out = {}
    for k, v in q.items():
        a = np.array([[[float(e) for e in row] for row in m] for m in v])
        assert all(Fraction(float(e)) == e for m in v for row in m for e in row)         # exactly representable
        out[k] = (a[..., 0] if k in ("lx", "lu") else a)[None]
    return out


@pytest.mark.parametrize("eager", [False, True], ids=["lazy", "eager"])
@pytest.mark.parametrize("lam", [Fraction(0), Fraction(1, 4)], ids=["lambda_0", "lambda_quarter"])
def test_statement_agrees_with_exact_rational_arithmetic(lam, eager):
    """2^-60 relative, every quantity measured against its own largest entry (an entry that is a difference of larger ones
    carries their rounding: long double rounds at 2^-64, the three steps leave a few dozen roundings in an entry)."""
    q = _exact_problem()
    Ks, ks, dV = _exact_backward(lam, q, eager)
    sK, sk, sdV = rr.backward(float(lam), _to_float(q), eager=eager)
    worst = 0.0
    for name, got, exact in (("K", sK[0], Ks), ("k", sk[0], [[v[0] for v in k] for k in ks]), ("dV", sdV[0], dV)):
        exact = np.array(exact, dtype=object)
        scale = max(abs(e) for e in exact.ravel())
        assert scale > 0
        for g, e in zip(np.asarray(got).ravel(), exact.ravel()):
            mant, exp = np.frexp(g)                                     # the long double as an exact Fraction
            hi = int(np.floor(np.ldexp(mant, 64)))
            err = abs(Fraction(hi, 2 ** 64) * Fraction(2) ** int(exp) - e) / scale
            worst = max(worst, float(err))
            assert err <= Fraction(1, 2 ** 60), (name, float(err))
    # the two readings of delta_V differ on this problem, and the in-place symmetrisation matters
    other = _exact_backward(lam, q, not eager)[2]
    assert other != dV
    print(f"\nlambda {lam}, {'eager' if eager else 'lazy'}: worst distance to the exact result {worst:.2e} (2^-60 = {2.0 ** -60:.2e})")
