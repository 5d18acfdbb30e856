"""The obstacle points per knot on the GPU (cilqr_scene_points_batch) and the batched TrajectoryPlanner::Plan
(cilqr_plan_scenes_batch), what can be held without a GPU: the C-ABI surface and the Python layers' argument checks.
The kernels themselves: tests/test_gpu_scene_points.py."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

from cilqr_amd import api, scenario, scene_io


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _packed(n=2, seed=1):
    spec = dataclasses.replace(scenario.SPECS["mix11"], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True)
    sf = scene_io.from_generator(sc)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_HOST, **{k: keep[k].ctypes.data for k in keep})
    return sc, packed, keep, sb


def test_both_calls_are_declared_exported_and_mirrored():
    hdr = open(api.HEADER_PATH).read()
    L = api.lib()
    for name in ("cilqr_scene_points_batch", "cilqr_plan_scenes_batch"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.cilqr_abi_version() == 7 == api.ABI_VERSION
    assert int(re.search(r"CILQR_ABI_VERSION (\d+)", hdr).group(1)) == 7
    for name, value in (("CILQR_PLAN_FIELDS", api.PLAN_FIELDS), ("CILQR_PLAN_DP_FAILED", api.PLAN_DP_FAILED),
                        ("CILQR_PLAN_CORRIDOR_FAILED", api.PLAN_CORRIDOR_FAILED), ("CILQR_OPT_SCENE_CHUNK", api.OPT_SCENE_CHUNK)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    # the new corridor_count code stands beside -2 ... -4 in the header
    assert re.search(r"-5 at knot 0", hdr)


def test_a_null_handle_is_refused_and_nothing_is_written():
    sc, packed, keep, sb = _packed()
    K = 51
    P = (packed["max_static"] + packed["max_dynamic"]) * packed["max_vertices"]
    times = np.arange(K) * 0.1
    pts = np.full((2, K, P, 2), -7.0)
    cnt, ok = np.full((2, K), -7, dtype=np.int32), np.full(2, -7, dtype=np.int32)
    L = api.lib()
    rc = L.cilqr_scene_points_batch(None, C.byref(sb), K, times.ctypes.data, 0, P, pts.ctypes.data, cnt.ctypes.data, ok.ctypes.data)
    assert rc == api.ERR_NULL and (pts == -7.0).all() and (cnt == -7).all() and (ok == -7).all()
    assert b"null" in L.cilqr_error_string(rc)

    M = api.default_config(50).max_iter
    traj, hist = np.full((2, K, 10), -7.0), np.full((2, M + 1, 5), -7.0)
    nc, st = np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int32)
    sol = api.SolutionBatch(api.MEM_HOST, 0, traj.ctypes.data, hist.ctypes.data, nc.ctypes.data, st.ctypes.data, None, None, None, None)
    plan, outcome = np.full((2, K, api.PLAN_FIELDS), -7.0), np.full(2, -7, dtype=np.int32)
    n_dp, n_cor = C.c_int32(-7), C.c_int32(-7)
    dp_cfg, cor_cfg = api.default_dp_config(tf=5.0), api.default_corridor_config()
    start = np.ascontiguousarray(sc["start"])
    rc = L.cilqr_plan_scenes_batch(None, C.byref(dp_cfg), C.byref(cor_cfg), C.byref(sb), start.ctypes.data, K, C.byref(sol),
                                   plan.ctypes.data, None, outcome.ctypes.data, C.byref(n_dp), C.byref(n_cor))
    assert rc == api.ERR_NULL and n_dp.value == -7 and n_cor.value == -7
    assert (traj == -7.0).all() and (hist == -7.0).all() and (nc == -7).all() and (st == -7).all()
    assert (plan == -7.0).all() and (outcome == -7).all()


def test_generate_dp_refuses_an_unknown_points_producer():
    with pytest.raises(ValueError, match="points must be 'host' or 'device'"):
        scenario.generate_dp("mix11", 2, seed=1, points="fpga")
