"""The double-precision oracle's cost and quadratisation stages held against their long-double restatement
(tests/stage_reference.py) on the crafted table of knot cases (tests/stage_cases.py): states exactly on a barrier's edge, half-
filled plane chunks, 64+ planes, far planes, unwrapped headings, discs beyond the lane tables and on the lane lines.  No GPU.

Bound: parity_util.entry_err (relative per entry, floor 1e-3 of the knot's -- for cost rows the problem's -- largest entry) at
the project's STAGE_TOL = 1e-9.  Worst error over every configuration, both rotations, with and without the intended lane
ties (measured, printed by test_oracle_agrees_with_the_long_double_statement): see DESIGN.md, section 5."""
import numpy as np
import pytest

import stage_cases as sc
import stage_reference as sr
from parity_util import entry_err
from oracle import oracle as orc

STAGE_TOL = 1e-9
TENSORS = ("A", "B", "lx", "lu", "lxx", "luu")


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    orc.lib()


def errors(got, ref):
    """{tensor: (worst entry_err, where)} of one group's stage outputs against a reference's (cost rows: one 'knot' per problem)"""
    out = {"cost": entry_err(got["cost"], np.asarray(ref["cost"], np.float64))}
    for k in TENSORS:
        g, r = np.asarray(got[k]), np.asarray(ref[k], np.float64)
        out[k] = entry_err(g.reshape((-1,) + g.shape[2:]), r.reshape((-1,) + r.shape[2:]))
    return out


def test_the_load_stage_is_mirrored_bit_for_bit():
    """The exact-edge cases are found with stage_cases' own plain-double copy of the load stage's shrink-and-normalise: it must
    be the oracle's, or those cases sit beside their edge."""
    for name in sc.CONFIGS:
        for cmax, g in sc.evaluate(name).items():
            cnt = g["scene"]["ccount"]
            live = np.arange(cmax)[None, None, :] < cnt[:, :, None]
            mine = sc.processed_planes(g["scene"]["corridor"], g["cfg"])
            assert np.array_equal(mine[live], g["cor"][live]), (name, cmax)
            assert np.array_equal(sc.processed_lanes(g["scene"]["left"], g["cfg"]), g["left"][0])
            assert np.array_equal(sc.processed_lanes(g["scene"]["right"], g["cfg"]), g["right"][0])


@pytest.mark.parametrize("name", list(sc.CONFIGS))
def test_oracle_agrees_with_the_long_double_statement(name):
    worst = {}
    for ties in (False, True):
        for rotation in (0, 1):
            for cmax, g in sc.evaluate(name, ties, rotation).items():
                for k, (e, where) in errors(g["oracle"], g["ld"]).items():
                    b = where[0] if k == "cost" else where[0] // (sc.K if k in ("lx", "lxx") else sc.N_STEPS)
                    i = None if k == "cost" else where[0] % (sc.K if k in ("lx", "lxx") else sc.N_STEPS)
                    what = g["cases"][g["which"][b, i]]["name"] if i is not None else f"problem {b}"
                    assert e < STAGE_TOL, (name, ties, rotation, cmax, k, e, where, what)
                    worst[k] = max(worst.get(k, 0.0), e)
    print(f"\n[{name}] oracle vs long double, worst entry_err: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_every_branch_is_taken_and_every_case_sits_at_both_kinds_of_knot():
    total = {k: 0 for k in sr.census_keys()}
    per_config = {}
    for name in sc.CONFIGS:
        for ties in (False, True):
            for cmax, g in sc.evaluate(name, ties, 0).items():
                for k, v in g["census"].items():
                    total[k] += v
                    per_config.setdefault(name, {}).setdefault(k, 0)
                    per_config[name][k] += v
    print("\ncensus over the table: " + ", ".join(f"{k} {v}" for k, v in total.items()))
    missing = [k for k, v in total.items() if v == 0]
    assert not missing, missing
    # under eps = 2^-6 every one of the ten bounds has a double exactly on its edge, and so have the corridor and both lanes
    cfg = sc.oracle_config("dyadic_eps")
    names = [c["name"] for g in sc.table(cfg).values() for c in g]
    assert sum(n.endswith(":edge_exact") for n in names) == 10 + 3, [n for n in names if "edge" in n]
    for fam in sr.FAMILIES:
        assert per_config["dyadic_eps"][f"{fam}:exactly_minus_eps"] > 0, fam
    # the default configuration has the one its eps allows (0 - v = -eps), all others one ulp beside
    assert per_config["default"]["state_bounds:exactly_minus_eps"] > 0
    # packer: every case at a terminal knot and at an interior one, in both rotations, at different places; neighbouring slots
    # mostly with different plane counts; the intended ties only on request
    for rotation in (0, 1):
        for cmax, g in sc.evaluate("default", True, rotation).items():
            n, which = len(g["cases"]), g["which"]
            assert set(which[:, -1]) == set(range(n)) and set(which[:, :-1].ravel()) == set(range(n)), (cmax, rotation)
            cnt = g["scene"]["ccount"]
            if cmax > 1:      # (cmax = 2 has the counts 0, 1, 2 only: half of all pairs differ at best)
                assert (cnt[1:] != cnt[:-1]).mean() > (0.5 if cmax >= 5 else 0.3), (cmax, rotation)
    a, b = sc.evaluate("default", True, 0), sc.evaluate("default", True, 1)
    assert all(not np.array_equal(a[c]["which"], b[c]["which"]) for c in a if len(a[c]["cases"]) > 1)
    assert any(c["tie"] for c in a[sc.MAIN_CMAX]["cases"])
    assert not any(c["tie"] for g in sc.evaluate("default", False, 0).values() for c in g["cases"])
    # cmax = 70: counts 63 .. 70 and the far family are there
    counts70 = {c["planes"].shape[0] for c in a[70]["cases"]}
    assert set(range(63, 71)) <= counts70 and {0, 1, 2, 3} <= counts70
    assert sum(c["cls"] == "far" for c in a[70]["cases"]) == 8


def test_far_family_needs_the_renormalised_product():
    """The far family's factors: 64 of them fit a double, all of a 70-plane knot's do not."""
    g = sc.evaluate("default")[70]
    far = [k for k, c in enumerate(g["cases"]) if c["cls"] == "far" and c["planes"].shape[0] == 70]
    b, i = np.argwhere(g["which"] == far[0])[0]
    off = sc.disc_offsets(g["cfg"])
    x = g["X"][b, i]
    px, py = x[0] + off[0] * np.cos(x[2]), x[1] + off[0] * np.sin(x[2])
    f = -(g["cor"][b, i, :, 0] * px + g["cor"][b, i, :, 1] * py - g["cor"][b, i, :, 2])
    assert (f > 2.6e4).all() and (f < 6.4e4).all()
    with np.errstate(over="ignore"):
        assert np.isfinite(np.prod(f[:64])) and not np.isfinite(np.prod(f))


def test_barrier_hooks_on_exact_edge_arguments():
    """oracle_barrier_value / _jacobian / _hessian at g = -eps exactly, at both neighbours, at 0 and beyond, against the
    long-double barrier with the branch the double g selects."""
    for name in ("default", "barrier", "dyadic_eps"):
        cfg = sc.oracle_config(name)
        o = orc.Oracle(cfg)
        bar = sr.Barrier(cfg)
        eps = float(cfg.barrier_eps)
        dg = np.array([0.6, -0.8, 0.35, 0.0, 0.0, 0.0])          # (the hook takes 6- and 2-vectors)
        ddg = np.zeros((6, 6))
        ddg[2, 2] = -0.45
        for g in (-eps, np.nextafter(-eps, -1.0), np.nextafter(-eps, 0.0), -0.5 * eps, -0.0, 0.0, 1e-6, 5.0, -3.0, -4.0e4):
            log = bar.branch(g)
            assert bool(log) == (g < -eps)
            G = sr.LD(g)
            assert entry_err(np.array([[o.barrier_value(g)]]), np.array([[float(bar.value(G, log))]]))[0] < STAGE_TOL, (name, g)
            j = np.asarray(bar.slope(G, log) * dg.astype(sr.LD), np.float64)
            assert entry_err(o.barrier_jacobian(g, dg)[None], j[None])[0] < STAGE_TOL, (name, g)
            c1, c2 = bar.curvature(G, log)
            H = np.asarray(c1 * np.outer(dg, dg).astype(sr.LD) - c2 * ddg.astype(sr.LD), np.float64)
            assert entry_err(o.barrier_hessian(g, dg, ddg)[None], H[None])[0] < STAGE_TOL, (name, g)
        # the two sides of the edge differ by the factor the tests of the kernels rely on
        c_log, _ = bar.curvature(sr.LD(np.nextafter(-eps, -1.0)), True)
        c_rel, _ = bar.curvature(sr.LD(-eps), False)
        assert abs(float(c_log / c_rel) - 1.0 / eps) < 1e-6 / eps
