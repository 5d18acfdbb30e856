"""Warm start (cilqr_warm_start, include/cilqr.h) without a GPU: the five entry points exist at every layer, reject a NULL
handle, and cilqr_amd.warm.warm_controls -- the NumPy statement of the gather rule the GPU tests compare against -- does what
the header says on hand-written cases."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from cilqr_amd import api, warm

NAMES = ("cilqr_solve_batch_warm", "cilqr_submit_warm", "cilqr_stage_load_warm", "cilqr_pool_submit_warm",
         "cilqr_multi_solve_warm")
N = 50
I32_MAX = 2 ** 31 - 1


def test_entry_points_are_declared_bound_and_exported(built):
    hdr = open(api.HEADER_PATH).read()
    assert int(re.search(r"#define CILQR_ABI_VERSION (\d+)", hdr).group(1)) == 7 == api.ABI_VERSION
    assert int(re.search(r"#define CILQR_ROWS_CONTROLS (\d+)", hdr).group(1)) == api.ROWS_CONTROLS == warm.ROWS_CONTROLS == 3
    assert (api.ROWS_TRAJ, api.ROWS_PLAN, api.ROWS_COARSE) == (warm.ROWS_TRAJ, warm.ROWS_PLAN, warm.ROWS_COARSE)
    assert "typedef struct cilqr_warm_start" in hdr
    L = api.lib()
    assert L.cilqr_abi_version() == 7
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (cilqr_[a-z_0-9]+)", out))
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/cilqr.h"
        assert name in api.EXPORTS and name in exported
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in api.lib()"
    # the struct of the binding is the header's: two int32, two pointers
    assert C.sizeof(api.WarmStart) == 8 + 2 * C.sizeof(C.c_void_p)
    assert [f[0] for f in api.WarmStart._fields_] == ["memory", "layout", "rows", "shift"]


def test_entry_points_reject_a_null_handle(built):
    L = api.lib()
    prob, sol = api.ProblemBatch(), api.SolutionBatch()
    rows = np.zeros((1, N, 2))
    w = api.WarmStart(api.MEM_HOST, api.ROWS_CONTROLS, rows.ctypes.data, None)
    for name in ("cilqr_solve_batch_warm", "cilqr_submit_warm", "cilqr_pool_submit_warm", "cilqr_multi_solve_warm"):
        assert getattr(L, name)(None, C.byref(prob), C.byref(w), C.byref(sol)) == api.ERR_NULL, name
        assert getattr(L, name)(None, None, None, None) == api.ERR_NULL, name
    assert L.cilqr_stage_load_warm(None, C.byref(prob), C.byref(w)) == api.ERR_NULL
    assert L.cilqr_stage_load_warm(None, None, None) == api.ERR_NULL


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rows(layout, B, rng):
    """random rows of a layout with every column filled, and the [B][N][2] controls that were put into them"""
    stride, col = warm.CONTROL_COLUMNS[layout]
    R = warm.rows_per_problem(layout, N)
    rows = rng.normal(size=(B, R, stride))
    ctl = rng.normal(size=(B, N, 2))
    rows[:, :N, col:col + 2] = ctl
    return rows, ctl


@pytest.mark.parametrize("layout", [warm.ROWS_TRAJ, warm.ROWS_PLAN, warm.ROWS_CONTROLS])
def test_warm_controls_on_hand_written_cases(layout):
    rng = np.random.default_rng(11)
    shifts = [0, 1, N - 1, N, N + 5, I32_MAX, -1]
    rows, ctl = _rows(layout, len(shifts), rng)
    U = warm.warm_controls(rows, np.asarray(shifts, np.int32), layout, N)
    assert U.shape == (len(shifts), N, 2) and U.dtype == np.float64
    assert np.array_equal(_bits(U[0]), _bits(ctl[0]))                                  # shift 0: the controls themselves
    assert np.array_equal(_bits(U[1, :N - 1]), _bits(ctl[1, 1:])) and not U[1, N - 1].any()   # 1: moved up, a zero pair at the end
    assert np.array_equal(_bits(U[2, 0]), _bits(ctl[2, N - 1])) and not U[2, 1:].any()        # N - 1: only the last pair is left
    for b in (3, 4, 5):                                                                # N, N + 5, 2^31 - 1: all zeros
        assert np.array_equal(_bits(U[b]), np.zeros((N, 2), np.uint64))                # (+0.0, not -0.0)
    assert not U[6].any()                                                              # -1: not warm-started, nothing gathered
    # no shift array: 0 for every problem
    assert np.array_equal(_bits(warm.warm_controls(rows, None, layout, N)), _bits(ctl))
    # the knot row K - 1 of the knot layouts is never read
    if layout != warm.ROWS_CONTROLS:
        poisoned = rows.copy()
        poisoned[:, N] = np.nan
        assert np.array_equal(_bits(warm.warm_controls(poisoned, np.asarray(shifts, np.int32), layout, N)), _bits(U))


@pytest.mark.parametrize("layout", [warm.ROWS_TRAJ, warm.ROWS_PLAN, warm.ROWS_CONTROLS])
def test_warm_controls_copies_bits(layout):
    """Neither clamped nor wrapped nor canonicalised: values far outside the control bounds, an angle beyond pi, -0.0, an
    infinity and a NaN with a payload all arrive as the bits they were."""
    stride, col = warm.CONTROL_COLUMNS[layout]
    rows = np.zeros((2, warm.rows_per_problem(layout, N), stride))
    special = np.array([1e9, -7.5, 4.0 * np.pi, -0.0, np.inf], np.float64)
    rows[0, :5, col] = special
    rows[0, :5, col + 1] = special[::-1]
    nan_payload = np.array([0x7ff8dead0000beef, 0xfff0000000000001], np.uint64).view(np.float64)   # a quiet and a signalling NaN
    rows[1, 3, col:col + 2] = nan_payload
    U = warm.warm_controls(rows, np.asarray([0, 2], np.int32), layout, N)
    assert np.array_equal(_bits(U[0, :5, 0]), _bits(special)) and np.array_equal(_bits(U[0, :5, 1]), _bits(special[::-1]))
    assert np.array_equal(_bits(U[1, 1]), _bits(nan_payload))       # row 3 with shift 2 is step 1
    assert not U[1, :1].any() and not U[1, 2:].any()


def test_warm_controls_rejects_what_carries_no_controls():
    with pytest.raises(ValueError):
        warm.warm_controls(np.zeros((1, N + 1, 9)), None, warm.ROWS_COARSE, N)
    with pytest.raises(ValueError):
        warm.warm_controls(np.zeros((1, N + 1, 10)), None, 17, N)
    with pytest.raises(ValueError):
        warm.warm_controls(np.zeros((1, N + 1, 10)), None, warm.ROWS_PLAN, N)     # 10 columns are not a plan row
    with pytest.raises(ValueError):
        warm.warm_controls(np.zeros((1, N - 1, 2)), None, warm.ROWS_CONTROLS, N)   # too few rows


def test_make_warm_builds_the_struct_from_host_arrays():
    rows = np.zeros((3, N + 1, 10))
    w, keep = api.make_warm((rows, [0, -1, 4]))
    assert (w.memory, w.layout) == (api.MEM_HOST, api.ROWS_TRAJ) and w.rows == keep[0].ctypes.data
    assert keep[1].dtype == np.int32 and w.shift == keep[1].ctypes.data
    w, keep = api.make_warm((np.zeros((3, N, 2)), None, api.ROWS_CONTROLS))
    assert w.layout == api.ROWS_CONTROLS and w.shift is None
    assert api.make_warm(None) == (None, None)
