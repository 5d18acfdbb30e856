"""The batched DP coarse planner (cilqr_dp_plan_batch, ABI 7), what can be held without a GPU: the padded scene
arrays of scene_io.pack_scene_batch and the C-ABI surface.  The planner itself: tests/test_gpu_dp_batch.py."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

from cilqr_amd import api, scenario, scene_io


@pytest.fixture(scope="module", autouse=True)
def _build(built):
    return built


def _scenes(family, n, seed):
    spec = dataclasses.replace(scenario.SPECS[family], min_clearance=-1.0)
    sc = scenario.generate(spec, n, seed=seed, scenarios=True)
    return sc, scene_io.from_generator(sc)


@pytest.mark.parametrize("family,seed", [("mix11", 3), ("demo80", 4), ("dyn20", 5)])
def test_pack_scene_batch_round_trips(family, seed):
    sc, sf = _scenes(family, 12, seed)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    B = 12
    S, D, V, T = (packed[k] for k in ("max_static", "max_dynamic", "max_vertices", "max_samples"))
    assert packed["batch"] == B
    assert packed["static_points"].shape == (B, S, V, 2) and packed["static_counts"].shape == (B, S)
    assert packed["dynamic_polygon_points"].shape == (B, D, V, 2) and packed["dynamic_trajectories"].shape == (B, D, T, 4)
    assert packed["static_counts"].dtype == packed["dynamic_polygon_counts"].dtype == packed["dynamic_trajectory_counts"].dtype == np.int32
    # every SPECS family fits the kernel's fixed-size storage
    assert V <= api.DP_MAX_VERTICES and S <= api.DP_MAX_STATIC and D <= api.DP_MAX_DYNAMIC and T <= api.DP_MAX_SAMPLES
    n_dyn = 0
    for b in range(B):
        flat = scene_io.flatten_scene(sf.center, sf.scenes[b])
        back = scene_io.unpack_scene(packed, b)
        assert flat.keys() == back.keys()
        for k in flat:
            assert flat[k].dtype == back[k].dtype and np.array_equal(flat[k], back[k]), (b, k)
        ns, nd = len(sf.scenes[b].static), len(sf.scenes[b].dynamic)
        n_dyn += nd
        # the slots behind the used ones are unused: count 0, zeros
        assert not packed["static_counts"][b, ns:].any() and not packed["static_points"][b, ns:].any()
        assert not packed["dynamic_polygon_counts"][b, nd:].any() and not packed["dynamic_trajectory_counts"][b, nd:].any()
        assert not packed["dynamic_trajectories"][b, nd:].any()
    assert n_dyn > 0
    # explicit, larger sizes pad further and change nothing that is used
    wide = scene_io.pack_scene_batch(sf.center, sf.scenes, max_static=S + 2, max_dynamic=D + 1, max_vertices=V + 3, max_samples=T + 7)
    assert wide["static_points"].shape == (B, S + 2, V + 3, 2) and wide["dynamic_trajectories"].shape == (B, D + 1, T + 7, 4)
    for b in range(B):
        back, back_w = scene_io.unpack_scene(packed, b), scene_io.unpack_scene(wide, b)
        assert all(np.array_equal(back[k], back_w[k]) for k in back)


def test_pack_scene_batch_refuses_a_scene_that_exceeds_a_maximum():
    sc, sf = _scenes("mix11", 6, 9)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    for k in ("max_static", "max_dynamic", "max_vertices", "max_samples"):
        if packed[k] < 2:
            continue
        with pytest.raises(ValueError, match=rf"scene \d+ needs {k} = {packed[k]}.*{k} = {packed[k] - 1}"):
            scene_io.pack_scene_batch(sf.center, sf.scenes, **{k: packed[k] - 1})
    sf.scenes[2].static.append(np.zeros((0, 2)))
    with pytest.raises(ValueError, match="scene 2 holds a polygon without vertices"):
        scene_io.pack_scene_batch(sf.center, sf.scenes)


def test_an_empty_batch_of_obstacles_packs_to_unused_slots():
    sc, sf = _scenes("mix11", 2, 1)
    for s in sf.scenes:
        s.static, s.dynamic = [], []
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    assert packed["max_static"] == packed["max_dynamic"] == packed["max_vertices"] == packed["max_samples"] == 1
    assert not packed["static_counts"].any() and not packed["dynamic_polygon_counts"].any()
    assert scene_io.unpack_scene(packed, 1)["static_points"].shape == (0, 2)


def test_the_batched_planner_is_declared_exported_and_mirrored():
    hdr = open(api.HEADER_PATH).read()
    assert re.search(r"\bint cilqr_dp_plan_batch\s*\(", hdr) and "typedef struct cilqr_scene_batch" in hdr
    assert "cilqr_dp_plan_batch" in api.EXPORTS
    L = api.lib()
    assert hasattr(L, "cilqr_dp_plan_batch")
    assert L.cilqr_abi_version() == 7 == api.ABI_VERSION
    assert int(re.search(r"CILQR_ABI_VERSION (\d+)", hdr).group(1)) == 7
    # the limits the header states are the ones the binding carries
    for name, value in (("VERTICES", api.DP_MAX_VERTICES), ("STATIC", api.DP_MAX_STATIC), ("DYNAMIC", api.DP_MAX_DYNAMIC),
                        ("SAMPLES", api.DP_MAX_SAMPLES), ("KNOTS", api.DP_MAX_KNOTS)):
        assert int(re.search(rf"#define CILQR_DP_MAX_{name} (\d+)", hdr).group(1)) == value
    # the struct's layout is the header's: 2 x int32, pointer, 6 x int32, 6 pointers
    assert C.sizeof(api.SceneBatchStruct) == 8 + 8 + 24 + 6 * 8
    assert api.SceneBatchStruct.static_points.offset == 40 and api.SceneBatchStruct.center.offset == 8


def test_a_null_handle_is_refused():
    sc, sf = _scenes("mix11", 2, 1)
    packed = scene_io.pack_scene_batch(sf.center, sf.scenes)
    keep = {k: np.ascontiguousarray(packed[k]) for k in api._SCENE_BATCH_ARRAYS}
    sb = api.scene_batch_struct(packed, api.MEM_HOST, **{k: keep[k].ctypes.data for k in keep})
    cfg = api.default_dp_config(tf=5.0)
    start = np.ascontiguousarray(sc["start"][:, :3])
    found = np.zeros(2, dtype=np.int32)
    nnf = C.c_int32(-7)
    rc = api.lib().cilqr_dp_plan_batch(None, C.byref(cfg), C.byref(sb), start.ctypes.data, 51, None, None, None, None,
                                       found.ctypes.data, C.byref(nnf))
    assert rc == api.ERR_NULL and nnf.value == -7 and not found.any()
    assert b"null" in api.lib().cilqr_error_string(rc)


def test_generate_dp_refuses_an_unknown_planner():
    with pytest.raises(ValueError, match="planner must be 'host' or 'device'"):
        scenario.generate_dp("mix11", 2, seed=1, planner="fpga")
