#!/usr/bin/env python
"""(Under tests/: it runs the CPU oracle.)  Child process of tests/test_gpu_parity.py::test_delta_v_evaluation_switch.

Runs with CILQR_LIB = cilqr_amd/lib/libcilqr_hip_dveager.so, the TEST-ONLY build of the product sources with
-DCILQR_DV_EVAL_EAGER (cilqr_amd/csrc/backward_core.hpp): delta_V_ of Backward (ilqr_optimizer.cc:383-384) from the Qu / Quu
the gains were computed from, instead of the lazy re-evaluation on the updated Vx / Vxx.  Checks, and prints one JSON line:
  * the backward stage in all three mappings (wavefront / eight lanes / one lane per problem): delta_V_ equals the oracle's
    EAGER variant (oracle_set_semantics(1, .)) to 1e-9, the three mappings agree bit for bit, gains are those of the
    default reading -- and delta_V_ is NOT the lazy oracle's (the switch does something);
  * the same three mappings on the crafted table at lambda 0 .. 1e11 against the long-double statement's eager reading
    (tests/riccati_reference.py), reported as "eager_statement_on_the_table";
  * whole solves: every step of every problem replays in the eager oracle within 1e-8."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def eager_against_the_statement(api, orc):
    """The crafted table (tests/stage_cases.py, default configuration, main group) at the lambda sweep of
    tests/test_gpu_riccati.py: delta_V of this library, in all three mappings, against the long-double statement's eager reading
    (tests/riccati_reference.py, eager=True) on the device's own quadratisation -- with that test's tolerance rule: STAGE_TOL
    where the eager oracle is within STAGE_TOL / 4 of the statement, 4 x the oracle's distance elsewhere (no problem may be
    there at N = 7); the gains against the statement's too."""
    import riccati_cases as rc
    import riccati_reference as rr
    import stage_cases as sc
    from resample_cases import same_rows
    g = sc.evaluate("default", True, 1)[sc.MAIN_CMAX]
    B = g["X"].shape[0]
    opt = api.BatchIlqrOptimizer(api.default_config(sc.N_STEPS), batch_capacity=B, cmax=sc.MAIN_CMAX)
    opt.set_option(api.OPT_EXACT_LANE_TIES, 1)
    opt.stage_load(g["scene"])
    opt.stage_set_trajectory(g["X"], g["U"])
    opt.stage_quadratize()
    q = {k: opt.read(t) for k, t in dict(A=api.T_A, B=api.T_B, lx=api.T_LX, lu=api.T_LU, lxx=api.T_LXX, luu=api.T_LUU).items()}
    lam = np.array([rc.TABLE_LAMBDAS[b % len(rc.TABLE_LAMBDAS)] for b in range(B)])
    outs = []
    for team, wave in ((0, 0), (4096, 0), (0, 4096)):
        opt.set_option(api.OPT_TEAM_THRESHOLD, team)
        opt.set_option(api.OPT_WAVE_THRESHOLD, wave)
        opt.stage_backward(lam)
        outs.append((opt.read(api.T_KFB), opt.read(api.T_KFF), opt.read(api.T_DV)))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert same_rows(a, b), "the mappings differ on the table"
    opt.close()
    sK, sk, s_eager = rr.backward(lam, q, eager=True)
    s_lazy = rr.backward(lam, q)[2]
    o = orc.Oracle(g["cfg"])
    orc.set_semantics(1, -1)
    worst, worst_oracle, n_lazy = np.zeros(3), np.zeros(3), 0
    for b in range(B):
        s = g["scene"]
        assert o.set_problem(s["start"][b], s["coarse"][b], s["corridor"][b], s["ccount"][b], s["left"], s["right"]) == 0
        ref = o.backward(float(lam[b]), {k: q[k][b] for k in q})
        d_o = rc.backward_distance(ref, (sK[b], sk[b], s_eager[b]))
        tol, loose = rc.statement_tolerance(d_o)
        assert not loose, (b, d_o)
        d = rc.backward_distance([t[b] for t in outs[0]], (sK[b], sk[b], s_eager[b]))
        assert (d < tol).all(), (b, float(lam[b]), d, tol)
        worst, worst_oracle = np.maximum(worst, d), np.maximum(worst_oracle, d_o)
        n_lazy += int(rc.backward_distance([outs[0][2][b]], [s_lazy[b]])[0] > 1e-6)
    orc.set_semantics(0, -1)
    assert n_lazy > 0                      # this library's delta_V is not the lazy statement's
    return {"worst_vs_eager_statement": dict(zip(rc.QUANTITIES, worst.tolist())),
            "eager_oracle_vs_eager_statement": dict(zip(rc.QUANTITIES, worst_oracle.tolist())), "problems_differing_from_the_lazy_statement": n_lazy}


def main():
    from cilqr_amd import api, scenario
    from oracle import oracle as orc
    from parity_util import assert_steps, oracle_cfg_from, rel_err
    assert "dveager" in api.LIB_PATH, api.LIB_PATH
    B = 96
    sc = scenario.generate("mix11", B, seed=52)
    cfg = api.default_config(sc["n_steps"])
    opt = api.BatchIlqrOptimizer(cfg, batch_capacity=B, cmax=sc["cmax"])
    ocfg = oracle_cfg_from(opt.cfg)
    opt.stage_load(sc)
    opt.stage_init_guess()
    X, U = opt.read(api.T_X), opt.read(api.T_U)
    opt.stage_quadratize()
    q = {k: opt.read(t) for k, t in dict(A=api.T_A, B=api.T_B, lx=api.T_LX, lu=api.T_LU, lxx=api.T_LXX, luu=api.T_LUU).items()}
    lam = np.linspace(0.5, 3.0, B)
    forms = {}
    for name, team, wave in (("wave", 4096, 1024), ("team", 4096, 0), ("lane", 0, 0)):
        opt.set_option(api.OPT_TEAM_THRESHOLD, team)
        opt.set_option(api.OPT_WAVE_THRESHOLD, wave)
        opt.stage_backward(lam)
        forms[name] = (opt.read(api.T_KFB), opt.read(api.T_KFF), opt.read(api.T_DV))
    for name in ("team", "lane"):
        for a, b in zip(forms[name], forms["wave"]):
            assert np.array_equal(a, b), f"{name} and wave mappings differ"
    Kfb, kff, dV = forms["wave"]
    worst_eager, n_differs_from_lazy = 0.0, 0
    for b in range(B):
        o = orc.Oracle(ocfg)
        assert o.set_problem(sc["start"][b], sc["coarse"][b], sc["corridor"][b], sc["ccount"][b], sc["left"], sc["right"]) == 0
        qb = {k: q[k][b] for k in q}
        orc.set_semantics(0, -1)
        oK, ok_, dV_lazy = o.backward(float(lam[b]), qb)
        orc.set_semantics(1, -1)
        oK1, ok1, dV_eager = o.backward(float(lam[b]), qb)
        assert np.array_equal(oK, oK1) and np.array_equal(ok_, ok1)        # the switch touches delta_V_ only
        assert rel_err(Kfb[b], oK, 1e-6) < 1e-9 and rel_err(kff[b], ok_, 1e-6) < 1e-9
        worst_eager = max(worst_eager, rel_err(dV[b], dV_eager, 1e-6))
        n_differs_from_lazy += int(rel_err(dV[b], dV_lazy, 1e-6) > 1e-6)
    assert worst_eager < 1e-9, worst_eager
    assert n_differs_from_lazy >= B // 2, n_differs_from_lazy
    opt.close()
    eager_statement = eager_against_the_statement(api, orc)
    # whole solves, replayed step by step in the eager oracle
    n = 160
    sc = scenario.generate("mix11", n, seed=77)
    opt = api.BatchIlqrOptimizer(cfg, batch_capacity=n, cmax=sc["cmax"])
    g = opt.plan(sc, max_iter_trajs=48, alpha_trace=True)
    orc.set_semantics(1, -1)
    rep = assert_steps(g, sc, ocfg, what="eager delta_V build against the eager oracle")
    orc.set_semantics(0, -1)
    opt.close()
    print(json.dumps({"ok": True, "worst_dV_error_vs_eager_oracle": worst_eager, "stage_problems_differing_from_lazy": n_differs_from_lazy,
                      "eager_statement_on_the_table": eager_statement,
                      "steps": {k: v for k, v in rep.items() if k != "failed"}}))


if __name__ == "__main__":
    main()
