"""The table of seeded search states that tests/test_search_reference.py (CPU, the oracle's stages) and tests/test_gpu_search.py
(the device's stage doors) run through the statement of tests/search_reference.py.

ENTRY = one iterate (a scene row with warm controls) at one regularisation lambda: its eleven candidate totals, delta_V_ and
gradient norm come from a PROVIDER of stage results -- the oracle, or the device's stage doors.  CASE = an entry with a seed
(cost_old, dlambda, and lambda = the entry's).  Seeds are laid around every threshold of the statement as pairs of ADJACENT
doubles of the seeded quantity with opposite verdicts (found by bisection on the statement's own expression), with solid cases
(far from every threshold) beside them for the comparison against the oracle's replay."""
import dataclasses
import math

import numpy as np

import search_reference as sr

PLAIN_LAMBDAS = (0.0, 1e-8, 1e-6, 1.0, 1e4)
BATCHES = (1, 9, 65, 257, 300)
BIG_CAPACITY = 320
ZERO_TOL_MAX_ITER = 200       # the harvesting solves (abs_cost_tol = rel_cost_tol = 0)
MARGIN_SOLID = 1e-9


def nxt(x):
    return float(np.nextafter(x, math.inf))


def prv(x):
    return float(np.nextafter(x, -math.inf))


def _ord(x):
    i = int(np.float64(x).view(np.int64))
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)


def _unord(i):
    return float(np.int64(i if i >= 0 else (-i) | -0x8000000000000000).view(np.float64))


def bisect_flip(a, b, key):
    """Adjacent doubles (x, y) between a and b with key(x) == key(a) != key(y); None when key(a) == key(b) or an end is
    not finite."""
    if not (math.isfinite(a) and math.isfinite(b)):
        return None
    ka = key(a)
    if ka == key(b):
        return None
    lo, hi = _ord(a), _ord(b)
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if key(_unord(mid)) == ka:
            lo = mid
        else:
            hi = mid
    return _unord(lo), _unord(hi)


def lambda_values():
    """(lambda, tag) beyond PLAIN_LAMBDAS: the neighbours of 1e-8 and of 1e-5, and the pair around lam * 1.6 = 1e11 with the
    double that lands exactly on 1e11 where one exists within 64 ulps."""
    out = [(prv(1e-8), "lam>1e-8"), (nxt(1e-8), "lam>1e-8"), (1e-5, "lam<1e-5"), (prv(1e-5), "lam<1e-5")]
    pair = bisect_flip(1e10, 1e11, lambda l: l * sr.RATIO > sr.REG_MAX)
    out += [(pair[0], "lam*ndl>1e11"), (pair[1], "lam*ndl>1e11")]
    x = pair[0]
    for _ in range(64):
        if x * sr.RATIO == sr.REG_MAX:
            out.append((x, "lam*ndl==1e11"))
            break
        x = prv(x)
    return out


DL_ACCEPT = bisect_flip(0.5, 2.0, lambda d: sr.div(d, sr.RATIO) < 1.0 / sr.RATIO)     # (first side, second side) of cc:273's fmin
DL_REJECT = bisect_flip(0.5, 2.0, lambda d: d * sr.RATIO > sr.RATIO)                  # (second side, first side) of cc:298's fmax


def take_rows(scene, idx):
    """the scene with problem rows idx (repeats allowed)"""
    n = scene["coarse"].shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    return {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.shape[:1] == (n,) and k not in ("left", "right") else v)
            for k, v in scene.items()}


def pick_iterates(iter_trajs, n_iter_trajs, traj, n_steps):
    """controls [4, N, 2] of the first, the middle and the last recorded iterate and of the final trajectory of one solve"""
    n = int(n_iter_trajs)
    rows = [iter_trajs[0], iter_trajs[n // 2], iter_trajs[n - 1], traj]
    return np.stack([np.ascontiguousarray(r[:n_steps, 8:10]) for r in rows])


CRAFTED_N = 7
CRAFTED_ROWS = 60


def crafted_rows():
    """(scene, U) of the N = 7 table of stage_cases.py (default configuration, main group: every row strings eight of the
    crafted cases along its knots), the first CRAFTED_ROWS rows -- the crafted controls are the warm controls, the scene
    (corridors, lane table) is the table's own"""
    import stage_cases as sc
    g = sc.evaluate("default", True, 1)[sc.MAIN_CMAX]
    idx = np.arange(min(CRAFTED_ROWS, g["U"].shape[0]))
    return take_rows(g["scene"], idx), np.ascontiguousarray(g["U"][idx])


def zero_tolerance_scene(n_steps, batch, seed):
    import riccati_cases as rc
    return rc.horizon_scene("mix11", n_steps, batch, seed=seed)


# ---------------------------------------------------------------------------------------------
# providers of stage results
# ---------------------------------------------------------------------------------------------
def oracle_stage(ocfg, scene, X, U, lam):
    """The oracle's stages on iterates (X, U) [B, ...] (X None: the open-loop rollout of U from goals_[0]) at lam [B]."""
    from oracle import oracle as orc
    B = U.shape[0]
    N, K = ocfg.n_steps, ocfg.n_steps + 1
    out = dict(X=np.zeros((B, K, 6)), U=np.array(U, dtype=np.float64), cost0=np.zeros((B, 5)), totals=np.zeros((B, 11, 5)),
               dV=np.zeros((B, 2)), gnorm=np.zeros(B), Xc=np.zeros((B, 11, K, 6)), Uc=np.zeros((B, 11, N, 2)))
    for b in range(B):
        o = orc.Oracle(ocfg)
        assert o.set_problem(scene["start"][b], scene["coarse"][b], scene["corridor"][b], scene["ccount"][b],
                             scene["left"], scene["right"]) == 0
        Xb = o.open_loop_rollout(o.constraints()[0][0], U[b]) if X is None else X[b]
        out["X"][b] = Xb
        out["cost0"][b] = o.total_cost(Xb, U[b])
        Kfb, kff, dV = o.backward(float(lam[b]), o.quadratize(Xb, U[b]))
        out["dV"][b], out["gnorm"][b] = dV, o.grad_norm(kff, U[b])
        for r, alpha in enumerate(sr.ALPHAS):
            out["Xc"][b, r], out["Uc"][b, r] = o.forward(alpha, Xb, U[b], Kfb, kff)
            out["totals"][b, r] = o.total_cost(out["Xc"][b, r], out["Uc"][b, r])
    return out


def device_stage(opt, opt_cost, scene, X, U, lam):
    """The same from the device's stage doors.  opt: the handle whose iterate and gains stay in place over the eleven rollouts;
    opt_cost: a second handle of the same configuration, which costs each candidate (cilqr_stage_set_trajectory resets the stages
    of the handle it is called on).  X None: the warm first iterate of the controls U, as a solve forms it."""
    from cilqr_amd import api
    B = U.shape[0]
    if X is None:
        opt.stage_load(scene, warm=(np.ascontiguousarray(U), None, api.ROWS_CONTROLS))
        opt.stage_init_guess()
        X, U = opt.read(api.T_X), opt.read(api.T_U)
    else:
        opt.stage_load(scene)
        opt.stage_set_trajectory(X, U)
    opt_cost.stage_load(scene)
    opt_cost.stage_set_trajectory(X, U)
    out = dict(X=X, U=U, cost0=opt_cost.stage_total_cost(), totals=np.zeros((B, 11, 5)),
               Xc=np.zeros((B, 11) + X.shape[1:]), Uc=np.zeros((B, 11) + U.shape[1:]))
    opt.stage_quadratize()
    opt.stage_backward(np.asarray(lam, dtype=np.float64))
    out["dV"], out["gnorm"] = opt.read(api.T_DV), opt.read(api.T_GNORM)
    for r, alpha in enumerate(sr.ALPHAS):
        opt.stage_forward(alpha)
        Xc, Uc = opt.read(api.T_XCAND), opt.read(api.T_UCAND)
        opt_cost.stage_set_trajectory(Xc, Uc)
        out["totals"][:, r] = opt_cost.stage_total_cost()
        out["Xc"][:, r], out["Uc"][:, r] = Xc, Uc
    return out


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    entry: int            # index into the entries (iterate x lambda) the table was laid on
    cost_old: float
    lam: float
    dlam: float
    kind: str
    pair: object = None   # cases that share a pair id are the two sides of one threshold
    threshold: str = ""
    lambda_side: bool = False   # the branch shows only in lambda' / dlambda': visible from the second iteration on
    two_step: bool = False      # rejects every step size at lambda = 2^-20, then -- at lambda' = 1 exactly -- accepts a late one


def _step(T, dV, gnorm, c, lam, dl, tol, it=None):
    it = tol["max_iter"] - 1 if it is None else it
    return sr.step(T, dV, gnorm, c, lam, dl, it, tol["abs"], tol["rel"], tol["max_iter"])


def lay_entry(e, row, T, dV, gnorm, lam, tag, tol, per_entry_tolerance=2):
    """The cases of entry e (an iterate, `row`, at one lambda).  T [11][5], dV [2]; tag: "" for a plain lambda, else the lambda
    threshold the entry serves (its pairs span the entries of a row)."""
    T = [[float(x) for x in row] for row in T]
    dV = (float(dV[0]), float(dV[1]))
    gnorm, lam = float(gnorm), float(lam)
    cases = []

    def add(kind, c, dl=1.0, pair=None, threshold="", lambda_side=False):
        cases.append(Case(e, float(c), lam, float(dl), kind, pair, threshold, lambda_side))

    tot = [row[0] for row in T]
    finite = all(math.isfinite(t) for t in tot) and all(math.isfinite(v) for v in dV)
    if tag == "lam<1e-5" or (gnorm < sr.GNORM_MIN and lam < sr.GNORM_LAMBDA) or not finite:
        # decided (or spoiled) before the search: one seed; the two lambdas around 1e-5 pair up across their entries
        add("before the search" if finite else "non-finite stage", tot[0] + 1.0 if finite else 1.0,
            pair=("lam<1e-5", row) if tag == "lam<1e-5" else None, threshold="lam<1e-5" if tag == "lam<1e-5" else "")
        return cases
    below = min(tot) - 1.0                     # below every total: every step size is rejected
    solid = {}
    Es = [-alpha * (dV[0] + alpha * dV[1]) for alpha in sr.ALPHAS]

    def first_index(c):
        for q, alpha in enumerate(sr.ALPHAS):
            if sr.verdict(alpha, c, tot[q], dV)[0]:
                return q
        return sr.NONE

    # where a verdict can change: the two ends of every step size's acceptance interval in cost_old, (tot + 1e-4 E, tot + 10 E)
    ends = sorted(tot[q] + z * Es[q] for q in range(11) if Es[q] > 0.0 and math.isfinite(Es[q]) for z in (sr.BETA_MIN, sr.BETA_MAX))
    for r in range(11):
        E = Es[r]
        if not (E > 0.0 and math.isfinite(E)):
            continue
        lo_r, hi_r = tot[r] + sr.BETA_MIN * E, tot[r] + sr.BETA_MAX * E
        pts = [p for p in ends if lo_r <= p <= hi_r]
        best = None
        for p, q in zip(pts, pts[1:]):                 # between two ends the verdicts are constant: the widest stretch where
            m = 0.5 * (p + q)                          # alpha_r is the FIRST accepted, alpha_0 .. alpha_{r-1} rejected
            if (best is None or q - p > best[2] - best[1]) and first_index(m) == r:
                best = (m, p, q)
        if best is None:
            continue
        inside, p, q = best
        if _step(T, dV, gnorm, inside, lam, 1.0, tol)["margin"] < MARGIN_SOLID:
            continue
        solid[r] = inside
        if tag:
            continue
        add("solid accept", inside)
        for end, beyond in ((p, p - 1e-3 * (q - p)), (q, q + 1e-3 * (q - p))):
            pair = bisect_flip(inside, beyond, first_index)
            if pair is None:
                continue
            # which step size changed its mind, and at which end of (1e-4, 10)
            flipped = next(k for k, alpha in enumerate(sr.ALPHAS)
                           if sr.verdict(alpha, pair[0], tot[k], dV)[0] != sr.verdict(alpha, pair[1], tot[k], dV)[0])
            name = "z=1e-4" if sr.verdict(sr.ALPHAS[flipped], pair[0], tot[flipped], dV)[3] < 1.0 else "z=10"
            for c in pair:
                add("threshold", c, pair=(name, e, r, flipped), threshold=name)
    if tag in ("", "lam>1e-8") and solid:
        r = min(solid)
        if tag == "lam>1e-8" or lam == sr.REG_MIN:
            add("lambda at 1e-8, accept", solid[r], pair=("lam>1e-8", row), threshold="lam>1e-8", lambda_side=True)
        if tag == "":
            for side, dl in enumerate(DL_ACCEPT):
                add("dlambda at fmin, accept", solid[r], dl=dl, pair=("fmin(dl/1.6)", e), threshold="fmin(dl/1.6, 1/1.6)", lambda_side=True)
            add("dlambda 1, accept", solid[r], dl=1.0, lambda_side=True)
    if tag == "":
        for r in sorted(solid)[:per_entry_tolerance]:
            # dcost on either side of abs_cost_tol, exactly on it where tot + abs_tol is exact; dcost / cost_old around rel_cost_tol
            pair = bisect_flip(tot[r] + tol["abs"] / 2, tot[r] + 2 * tol["abs"], lambda c, r=r: c - tot[r] < tol["abs"])
            if pair and all(_step(T, dV, gnorm, c, lam, 1.0, tol)["index"] == r for c in pair):
                for c in pair:
                    add("threshold", c, pair=("abs", e, r), threshold="abs_cost_tol")
            c = tot[r] + tol["abs"]
            if c - tot[r] == tol["abs"] and _step(T, dV, gnorm, c, lam, 1.0, tol)["index"] == r:
                add("dcost == abs_cost_tol", c)
            if tot[r] > 0.0 and tol["rel"] > 0.0:
                pair = bisect_flip(tot[r] / (1 - tol["rel"] / 2), tot[r] / (1 - 2 * tol["rel"]),
                                   lambda c, r=r: sr.div(c - tot[r], c) < tol["rel"])
                if pair and all(_step(T, dV, gnorm, c, lam, 1.0, tol)["index"] == r for c in pair):
                    for c in pair:
                        add("threshold", c, pair=("rel", e, r), threshold="rel_cost_tol")
    # every step size rejected: the other half of the schedule
    if tag in ("", "lam*ndl>1e11", "lam*ndl==1e11", "lam>1e-8"):
        add("reject all", below, pair=("lam*ndl>1e11", row) if tag == "lam*ndl>1e11" else None,
            threshold="lam*ndl>1e11" if tag == "lam*ndl>1e11" else "", lambda_side=True)
        if tag == "":
            for dl in DL_REJECT:
                add("dlambda at fmax, reject", below, dl=dl, pair=("fmax(dl*1.6)", e), threshold="fmax(dl*1.6, 1.6)", lambda_side=True)
            for c in (math.nan, math.inf, -math.inf):
                add("hostile", c)
    return cases


# a reject at lambda = 2^-20 with dlambda = 0.625 * 2^20 gives ndl = 2^20 (0.625 * 1.6 is exactly 1) and lambda' = 1.0 exactly:
# a plain lambda, at which the row is staged already -- and far enough from 2^-20 for the eleven totals to differ
TWO_STEP_LAMBDA, TWO_STEP_DLAMBDA = 2.0 ** -20, (1.0 / sr.RATIO) * 2.0 ** 20


def lay_table(stage, entries, tol):
    """stage: a provider's result over the entries (one problem per entry); entries: (row, lambda, tag) as entries_for gives"""
    cases = []
    for e, (row, lam, tag) in enumerate(entries):
        if tag != "two-step":
            cases += lay_entry(e, row, stage["totals"][e], stage["dV"][e], stage["gnorm"][e], lam, tag, tol)
    # Two-iteration cases: in a solve's FIRST iteration the active list is the identity, so a pending list that mixes list
    # positions and slots shows only later, once problems have left.  A seed that every step size rejects at lambda = 2^-20
    # (the iterate stays, lambda' = 1.0) and whose first accept at lambda = 1 is a later step size, looked for among the seeds
    # of the row's entry at lambda = 1.
    assert TWO_STEP_DLAMBDA * sr.RATIO == 2.0 ** 20 and TWO_STEP_LAMBDA * 2.0 ** 20 == 1.0
    at_one = {row: e for e, (row, lam, tag) in enumerate(entries) if tag == "" and lam == 1.0}
    for e0, (row, lam, tag) in enumerate(entries):
        if tag != "two-step" or row not in at_one:
            continue
        e1 = at_one[row]
        for c in [k for k in cases if k.entry == e1 and math.isfinite(k.cost_old) and k.dlam == 1.0 and not k.lambda_side]:
            first = _step(stage["totals"][e0], stage["dV"][e0], stage["gnorm"][e0], c.cost_old, lam, TWO_STEP_DLAMBDA, tol, it=0)
            second = _step(stage["totals"][e1], stage["dV"][e1], stage["gnorm"][e1], c.cost_old, 1.0, first["dlam"], tol, it=1)
            if first["index"] == sr.NONE and first["lam"] == 1.0 and second["index"] >= 1:
                cases.append(Case(e0, c.cost_old, lam, TWO_STEP_DLAMBDA, "late accept after a reject", two_step=True))
    return cases


def entries_for(n_rows, tagged_rows):
    """(row, lambda, tag) of every entry: each row at the plain lambdas and at the two lambdas around 1e-5 (the gradient-norm exit
    needs an iterate whose norm is small: which rows have one is the provider's to say), the first `tagged_rows` rows also at the
    other threshold lambdas"""
    special = lambda_values()
    out = [(row, lam, "") for row in range(n_rows) for lam in PLAIN_LAMBDAS]
    out += [(row, lam, tag) for row in range(n_rows) for lam, tag in special if tag == "lam<1e-5"]
    out += [(row, lam, tag) for row in range(min(tagged_rows, n_rows)) for lam, tag in special if tag != "lam<1e-5"]
    out += [(row, TWO_STEP_LAMBDA, "two-step") for row in range(n_rows)]
    return out


def run_statement(cases, stage, tol, it=None):
    """The statement's one-iteration result of every case, and the census of the table."""
    census = sr.Census()
    results = []
    for c in cases:
        s = _step(stage["totals"][c.entry], stage["dV"][c.entry], stage["gnorm"][c.entry], c.cost_old, c.lam, c.dlam, tol, it)
        census.add(s)
        results.append(s)
    count_flips(cases, results, census)
    return results, census


def outcome(s, threshold=""):
    """what the two sides of a pair are compared by: everything the iteration leaves -- except across a pair that seeds two
    lambdas, whose lambda' differ whatever the branch: the branch itself (accepted index, status, lambda' == 0)"""
    if threshold.startswith("lam"):
        return (s["index"], s["status"], s["lam"] == 0.0)
    return (s["index"], s["status"], s["lam"], s["dlam"], None if s["row"] is None else tuple(s["row"]))


def count_flips(cases, results, census, key=outcome):
    pairs = {}
    for c, s in zip(cases, results):
        if c.pair is not None:
            pairs.setdefault((c.threshold, c.pair), []).append(key(s, c.threshold))
    for (threshold, _), seen in pairs.items():
        if len(seen) >= 2 and len({repr(k) for k in seen}) > 1:
            census.add_flip(threshold)
    return census


def run_chains(cases, stage0, stage_fn, tol, n_back=3):
    """The statement over n_back iterations of every case (iter = max_iter - n_back): a numpy loop over a provider's stages
    and the statement's decisions.  stage0: the provider's result over the ENTRIES (first iterate); stage_fn(X, U, lam) -> the
    same over the cases' current iterates.  Returns (expected arrays, census)."""
    n, M = len(cases), tol["max_iter"]
    e = np.array([c.entry for c in cases])
    X, U = stage0["X"][e].copy(), stage0["U"][e].copy()
    cost_old = np.array([c.cost_old for c in cases])
    lam, dlam = np.array([c.lam for c in cases]), np.array([c.dlam for c in cases])
    alive = np.ones(n, bool)
    x = dict(trace=np.full((n, n_back), -3), status=np.zeros(n, int), n_cost=np.ones(n, int), n_iter=np.full(n, M - n_back),
             n_iter_trajs=np.ones(n, int), rows=np.zeros((n, n_back, 5)), its=np.zeros((n, n_back + 1) + X.shape[1:]))
    x["its"][:, 0] = X
    census = sr.Census()
    for k in range(n_back):
        if not alive.any():
            break
        st = stage0 if k == 0 else stage_fn(X, U, np.where(alive, lam, 1.0))
        for i in np.flatnonzero(alive):
            j = e[i] if k == 0 else i
            s = sr.step(st["totals"][j], st["dV"][j], st["gnorm"][j], cost_old[i], lam[i], dlam[i], M - n_back + k, tol["abs"], tol["rel"], M)
            census.add(s)
            x["trace"][i, k] = s["index"]
            if s["index"] >= 0:
                x["rows"][i, x["n_cost"][i] - 1] = s["row"]
                x["n_cost"][i] += 1
                X[i], U[i] = st["Xc"][j, s["index"]], st["Uc"][j, s["index"]]
            if s["emits"]:
                x["its"][i, x["n_iter_trajs"][i]] = X[i]
                x["n_iter_trajs"][i] += 1
            cost_old[i], lam[i], dlam[i] = s["cost_old"], s["lam"], s["dlam"]
            x["status"][i], x["n_iter"][i], alive[i] = s["status"], s["it"], not s["done"]
    x.update(X=X, U=U, lam=lam, dlam=dlam)
    return x, census


def final_bits(x, i):
    """what a chain leaves of case i, for the comparison of the two sides of a pair"""
    return (tuple(int(v) for v in x["trace"][i]), int(x["status"][i]), int(x["n_cost"][i]),
            np.ascontiguousarray(x["rows"][i]).tobytes(), np.ascontiguousarray(x["X"][i]).tobytes())


def chain_flips(cases, x):
    """per threshold: the pairs whose two sides end in different bits"""
    pairs, flips = {}, {}
    for i, c in enumerate(cases):
        if c.pair is not None:
            pairs.setdefault((c.threshold, c.pair), []).append(i)
    for (th, _), members in pairs.items():
        if len({final_bits(x, i) for i in members}) > 1:
            flips[th] = flips.get(th, 0) + 1
    return flips


THRESHOLDS = ("z=1e-4", "z=10", "abs_cost_tol", "rel_cost_tol", "lam>1e-8", "lam<1e-5", "fmin(dl/1.6, 1/1.6)", "fmax(dl*1.6, 1.6)",
              "lam*ndl>1e11")
