"""The statement of what follows the five stages of an iteration of Optimize() (algorithm/ilqr/ilqr_optimizer.cc): the
gradient-norm exit (cc:235-241), the acceptance test over the eleven step sizes (cc:246-261) and the bookkeeping after it
(cc:272-319) -- written from those formulas, one problem and one iteration at a time, in IEEE doubles and in the reference's
expression order.  The product is built without contraction and with an IEEE divide, so this predicts BITS: the accepted
index, the recorded cost row, lambda', dlambda', the status and the three counts.

Inputs of step(): the eleven candidate totals (five columns each: total, J, dynamics bounds, corridor, lane), delta_V_ (two
numbers), the gradient norm, and the search state cost_old, lambda, dlambda, iter with the configuration's abs_cost_tol,
rel_cost_tol and max_iter.  chain() runs several iterations, asking a callback for the stage results of each iterate.

Census: the branch counters every table of cases is measured by (tests/search_cases.py, the CPU and the GPU tests)."""
import math

import numpy as np

ALPHAS = (1.0000, 0.5012, 0.2512, 0.1259, 0.0631, 0.0316, 0.0158, 0.0079, 0.0040, 0.0020, 0.0010)   # cc:197
BETA_MIN, BETA_MAX = 1e-4, 10.0        # cc:258
RATIO, REG_MIN, REG_MAX = 1.6, 1e-8, 1e11
GNORM_MIN, GNORM_LAMBDA = 1e-6, 1e-5   # cc:236
ST_RUNNING, ST_ABS, ST_REL, ST_GNORM, ST_UNSOLVED, ST_MAX_ITER = 0, 1, 2, 3, 4, 5
NONE, BEFORE = -1, -2                  # accepted index: every step size rejected / left before the search
CLAUSES = ("z<=1e-4", "z>=10", "dcost<=0", "z nan")


def fmin(a, b):
    """C's fmin: a NaN loses against a number"""
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    return a if a < b else b


def fmax(a, b):
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    return a if a > b else b


def div(a, b):
    """IEEE a / b (Python raises where C gives an infinity or a NaN)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def verdict(alpha, cost_old, total, dV):
    """(accepted, rejecting clause or None, dcost, z) of one step size: cc:254-258"""
    dcost = cost_old - total
    expected = -alpha * (dV[0] + alpha * dV[1])
    z = div(dcost, expected)
    if (z > BETA_MIN and z < BETA_MAX) and dcost > 0.0:
        return True, None, dcost, z
    if math.isnan(z):
        clause = "z nan"
    elif not z > BETA_MIN:
        clause = "z<=1e-4"
    elif not z < BETA_MAX:
        clause = "z>=10"
    else:
        clause = "dcost<=0"
    return False, clause, dcost, z


def step(totals, dV, gnorm, cost_old, lam, dlam, it, abs_tol, rel_tol, max_iter):
    """One iteration.  totals [11][5].  Returns a dict: index (0..10, NONE, BEFORE), clauses (the clause that rejected each
    earlier step size), row (the five columns recorded, or None), cost_old / lam / dlam afterwards, status (ST_RUNNING: the solve
    goes on), done, emits (the new iterate joins iter_trajs), it (the next iteration index), and `branches`: the census names
    this iteration took.  `margin`: the smallest relative distance to its threshold of a decision on a COMPUTED quantity (the
    gradient norm, z, dcost, dcost / cost_old); the schedule's decisions are on the seeded lambda and dlambda, which are exact."""
    lam, dlam, cost_old = float(lam), float(dlam), float(cost_old)
    out = dict(index=BEFORE, clauses=[], row=None, cost_old=cost_old, lam=lam, dlam=dlam, status=ST_RUNNING, done=False,
               emits=False, it=it + 1, branches=[], margin=math.inf)
    br = out["branches"]

    def near(a, b):
        s = max(abs(a), abs(b))
        if s > 0.0 and not math.isnan(s) and not math.isinf(s):
            out["margin"] = min(out["margin"], abs(a - b) / s)

    if lam < GNORM_LAMBDA:
        near(gnorm, GNORM_MIN)
    if gnorm < GNORM_MIN and lam < GNORM_LAMBDA:                                   # cc:236-241
        out.update(status=ST_GNORM, done=True)
        br.append("exit gnorm")
        return out
    index, dcost = NONE, 0.0
    for r, alpha in enumerate(ALPHAS):                                             # cc:246-265
        ok, clause, dcost, z = verdict(alpha, cost_old, float(totals[r][0]), (float(dV[0]), float(dV[1])))
        near(z, BETA_MIN)
        near(z, BETA_MAX)
        if cost_old != 0.0 and not math.isnan(dcost) and not math.isinf(dcost) and not math.isinf(cost_old):
            out["margin"] = min(out["margin"], abs(dcost) / abs(cost_old))
        if ok:
            index = r
            break
        out["clauses"].append(clause)
        br.append("reject " + clause)
    out["index"] = index
    br.append(f"accept {index}" if index >= 0 else "accept none")
    if index >= 0:
        a, b = div(dlam, RATIO), 1.0 / RATIO
        br.append("fmin(dl/1.6, 1/1.6): first" if a < b else "fmin(dl/1.6, 1/1.6): second")
        ndl = fmin(a, b)                                                           # cc:273
        br.append("lam > 1e-8: 1" if lam > REG_MIN else "lam > 1e-8: 0")
        out["dlam"] = ndl
        out["lam"] = lam * ndl * (1.0 if lam > REG_MIN else 0.0)                   # cc:275
        out["row"] = [float(c) for c in totals[index]]
        rel = div(dcost, cost_old)
        near(dcost, abs_tol)
        near(rel, rel_tol)
        if dcost < abs_tol or rel < rel_tol:                                       # cc:281-293
            out.update(status=ST_ABS if dcost < abs_tol else ST_REL, done=True)
            br.append("exit abs" if dcost < abs_tol else "exit rel")
            if dcost < abs_tol and rel < rel_tol:
                br.append("exit abs and rel")
            if it + 1 >= max_iter:
                br.append("exit converged at max_iter")
        else:
            out["emits"] = True                                                    # cc:294
            out["cost_old"] = float(totals[index][0])                              # cc:295
    else:
        a = dlam * RATIO
        br.append("fmax(dl*1.6, 1.6): first" if a > RATIO else "fmax(dl*1.6, 1.6): second")
        ndl = fmax(a, RATIO)                                                       # cc:298
        b = lam * ndl
        br.append("fmax(lam*ndl, 1e-8): first" if b > REG_MIN else "fmax(lam*ndl, 1e-8): second")
        nl = fmax(b, REG_MIN)                                                      # cc:299
        out["dlam"], out["lam"] = ndl, nl
        if nl > REG_MAX:                                                           # cc:302
            out.update(status=ST_UNSOLVED, done=True)
            br.append("exit unsolved")
    if not out["done"] and it + 1 >= max_iter:                                     # cc:312
        out.update(status=ST_MAX_ITER, done=True)
        br.append("exit max_iter")
    return out


def chain(stage, cost_old, lam, dlam, it, abs_tol, rel_tol, max_iter):
    """The iterations of a solve from a seeded search state.  stage(k, lam, accepted) -> (totals [11][5], dV, gnorm) of the
    iterate in force at iteration k: `accepted` lists the indices accepted so far (the iterate is the candidate of the last
    one; an empty list: the first iterate).  Returns dict(steps, rows (cost rows after row 0), status, n_iter, n_cost,
    n_iter_trajs, accepted, lam, dlam, cost_old)."""
    steps, rows, accepted = [], [], []
    n_it = 1
    status = ST_RUNNING
    k = 0
    while True:
        totals, dV, gnorm = stage(k, lam, tuple(accepted))
        s = step(totals, dV, gnorm, cost_old, lam, dlam, it, abs_tol, rel_tol, max_iter)
        steps.append(s)
        if s["index"] >= 0:
            accepted.append(s["index"])
            rows.append(s["row"])
        n_it += int(s["emits"])
        cost_old, lam, dlam, it, status = s["cost_old"], s["lam"], s["dlam"], s["it"], s["status"]
        k += 1
        if s["done"]:
            break
    return dict(steps=steps, rows=rows, status=status, n_iter=it, n_cost=1 + len(rows), n_iter_trajs=n_it,
                accepted=accepted, lam=lam, dlam=dlam, cost_old=cost_old)


# ---------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------
BRANCHES = tuple(
    [f"accept {r}" for r in range(11)] + ["accept none"] + ["reject " + c for c in CLAUSES]
    + ["exit gnorm", "exit abs", "exit rel", "exit unsolved", "exit max_iter", "exit abs and rel", "exit converged at max_iter"]
    + ["fmin(dl/1.6, 1/1.6): first", "fmin(dl/1.6, 1/1.6): second", "fmax(dl*1.6, 1.6): first", "fmax(dl*1.6, 1.6): second",
       "fmax(lam*ndl, 1e-8): first", "fmax(lam*ndl, 1e-8): second", "lam > 1e-8: 0", "lam > 1e-8: 1"])


class Census:
    """How often each branch of the statement was taken (cases), and how many adjacent pairs flipped per threshold."""

    def __init__(self):
        self.branches = {b: 0 for b in BRANCHES}
        self.flips = {}

    def add(self, step_result):
        for b in set(step_result["branches"]):      # once per iteration, however many step sizes a clause rejected
            self.branches[b] += 1

    def add_flip(self, threshold):
        self.flips[threshold] = self.flips.get(threshold, 0) + 1

    def missing(self, at_least=1):
        return [b for b, n in self.branches.items() if n < at_least]

    def report(self):
        return "; ".join(f"{b} {n}" for b, n in self.branches.items()) + " | flips: " + \
            "; ".join(f"{t} {n}" for t, n in sorted(self.flips.items()))
