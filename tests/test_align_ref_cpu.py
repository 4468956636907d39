"""The host side of include/coxgraph_hip_align.h without a GPU (cox_align_grid, cox_align_select through the library, against
tests/align_ref.py), and the reference search itself on the analytic room: it recovers seeded true poses to within one final grid
step per axis.  DESIGN.md section 7o."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import align_ref as A
import track_ref
from coxgraph_amd import capi
from coxgraph_amd.capi import CoxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cox_align_config_default", "cox_align_create", "cox_align_destroy", "cox_align_grid", "cox_align_kernel_time", "cox_align_search",
           "cox_align_select", "cox_align_set_samples", "cox_align_sweep"]


def test_align_header_symbols_are_exported(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coxgraph_hip_align.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text))) == SYMBOLS
    assert not [s for s in SYMBOLS if not hasattr(hip.lib, s)]
    assert "#define COX_ALIGN_Q 1024u" in text and A.Q == capi.ALIGN_Q == 1024


def test_structures_have_the_headers_layout(hip):
    assert C.sizeof(capi.AlignScore) == 24 == A.SCORE_DTYPE.itemsize == capi.ALIGN_SCORE_DTYPE.itemsize
    assert A.SCORE_DTYPE == capi.ALIGN_SCORE_DTYPE
    assert C.sizeof(capi.AlignConfig) == 16 and C.sizeof(capi.AlignSearchConfig) == 120
    assert C.sizeof(capi.AlignLevel) == 8 + 32 + 8 + 4 * 64 + 32 * 64 + 24 * 64
    c = capi.align_config(hip)
    assert c.inlier_distance == np.float32(0.4) and c.no_correspondence_cost == 0.0


# ---- cox_align_grid ---------------------------------------------------------------------------------------------------------------
GRIDS = {
    "room_level0": ((0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP),
    "frozen_z_and_yaw": ((0.3, -0.1, 1.5, 0.2), (1.0, 0.5, 0.7, 3.0), (0.25, 0.1, 0.0, 0.0)),
    "all_frozen": ((1.0, 2.0, 3.0, 4.0), (1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0)),
    "half_below_step": ((0.1, 0.2, 0.3, 0.4), (0.19, 0.2, 0.3, 0.05), (0.4, 0.4, 0.4, 0.2)),   # 0.475 -> 0, 0.5 -> 1 (away from zero), 0.75 -> 1, 0.25 -> 0
    "refinement": ((0.4, -0.8, 0.0, math.radians(30.0)), (0.2, 0.2, 0.2, math.radians(5.0)), (0.2, 0.2, 0.2, math.radians(5.0))),
    "refinement_frozen_z": ((0.4, -0.8, 0.7, -3.0), (0.05, 0.05, 0.0, 0.01), (0.05, 0.05, 0.0, 0.01)),
    "inexact_ratio": ((0.0, 0.0, 0.0, 0.0), (0.7, 0.35, 0.1 * 3, 1.0), (0.1, 0.1, 0.1, 0.3)),
    "yaw_not_wrapped": ((0.0, 0.0, 0.0, 3.0), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.5)),
}


@pytest.mark.parametrize("name", list(GRIDS))
def test_grid_matches_the_reference_bit_for_bit(hip, name):
    center, half, step = GRIDS[name]
    want = A.grid(center, half, step)
    got = capi.align_grid(hip, center, half, step)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    counts = [2 * A._llround(h / s) + 1 if s > 0 else 1 for h, s in zip(half, step)]
    assert len(got) == int(np.prod(counts))
    if name == "room_level0":
        assert counts == [7, 7, 3, 35]
    if name == "half_below_step":
        assert counts == [1, 3, 3, 1]
    if name == "refinement":
        assert counts == [3, 3, 3, 3] and got[40].tobytes() == np.array(center, np.float64).tobytes()   # the kept pose is its own centre candidate
    if name == "yaw_not_wrapped":
        assert got[:, 3].max() == 4.0 > math.pi
    # C order: x slowest, yaw fastest
    assert np.all(np.diff(got[:counts[3], 3]) > 0) or counts[3] == 1
    assert np.all(got[::max(1, len(got) // counts[0]), 0][:counts[0]] == np.unique(got[:, 0]))


def test_grid_refuses_bad_arguments(hip):
    ok = ((0.0,) * 4, (1.0,) * 4, (0.5,) * 4)
    n = C.c_uint64()
    f = hip.fn("align_grid")
    arr = [np.array(v, np.float64) for v in ok]
    p = [capi._fp(a) for a in arr]
    assert f(p[0], p[1], p[2], None, C.c_uint64(0), C.byref(n)) == 0 and n.value == 5 ** 4
    small = np.zeros((10, 4))
    assert f(p[0], p[1], p[2], capi._fp(small), C.c_uint64(10), C.byref(n)) == -7 and not small.any()   # COX_ERR_BUFFER_TOO_SMALL
    for k in range(3):
        q = list(p)
        q[k] = None
        assert f(q[0], q[1], q[2], None, C.c_uint64(0), C.byref(n)) == -1
    assert f(p[0], p[1], p[2], None, C.c_uint64(0), None) == -1
    for which, bad in ((0, math.nan), (0, math.inf), (1, -0.1), (1, math.inf), (2, -0.5), (2, math.nan)):
        v = [list(x) for x in ok]
        v[which][2] = bad
        with pytest.raises(CoxError) as e:
            capi.align_grid(hip, *v)
        assert e.value.status == -1, (which, bad)
    with pytest.raises(CoxError):       # 4097^2 poses: beyond COX_ALIGN_MAX_GRID
        capi.align_grid(hip, (0.0,) * 4, (2048.0, 2048.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0))
    with pytest.raises(CoxError):
        capi.align_grid(hip, (0.0,) * 4, (1e300, 0.0, 0.0, 0.0), (1e-300, 0.0, 0.0, 0.0))


# ---- cox_align_select -------------------------------------------------------------------------------------------------------------
def _records(seed, n, ties):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, A.SCORE_DTYPE)
    rec["score"] = rng.integers(0, 1 << 40, n)
    rec["n_corr"] = rng.integers(0, 300, n)
    rec["n_inlier"] = np.minimum(rec["n_corr"], rng.integers(0, 300, n))
    rec["cost"] = rng.uniform(0, 1, n)
    if ties:   # duplicated records: the index decides
        src = rng.integers(0, n, n // 2)
        rec[rng.integers(0, n, n // 2)] = rec[src]
    return rec


@pytest.mark.parametrize("keep", (1, 2, 8, 63, 64))
@pytest.mark.parametrize("n,ties", ((1, False), (5, True), (64, True), (65, False), (1000, True), (5145, True)))
def test_select_matches_the_reference(hip, keep, n, ties):
    rec = _records(17 * n + keep, n, ties)
    for min_corr in (0, 1, 150, 299, 300):
        want = A.select(rec, min_corr, keep)
        got = capi.align_select(hip, rec, min_corr, keep)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (min_corr, got, want)
        assert len(got) == min(keep, int((rec["n_corr"] >= min_corr).sum()))
    assert len(capi.align_select(hip, rec, 300, keep)) == 0     # min_corr excludes everything: n_corr < 300


def test_select_breaks_ties_by_index(hip):
    rec = np.zeros(200, A.SCORE_DTYPE)
    rec["n_corr"] = 10
    rec["score"][[150, 20, 77]] = 5
    rec["score"][[199, 3]] = 9
    assert capi.align_select(hip, rec, 10, 64).tolist()[:6] == [3, 199, 20, 77, 150, 0]
    assert capi.align_select(hip, rec, 10, 1).tolist() == [3]
    assert capi.align_select(hip, rec, 11, 64).tolist() == []
    assert capi.align_select(hip, rec[:0], 0, 8).tolist() == []
    big = np.zeros(3, A.SCORE_DTYPE)
    big["score"] = [(1 << 63) + 1, (1 << 63) + 2, 1 << 63]       # compared as unsigned 64-bit
    assert capi.align_select(hip, big, 0, 3).tolist() == [1, 0, 2]


def test_select_refuses_bad_arguments(hip):
    rec = _records(1, 10, False)
    idx, n = np.zeros(64, np.uint32), C.c_uint32()
    f = hip.fn("align_select")
    args = lambda scores=capi._fp(rec), keep=8, out=capi._fp(idx), cnt=C.byref(n): (scores, C.c_uint64(10), C.c_uint32(0), C.c_uint32(keep), out, cnt)  # noqa: E731
    assert f(*args()) == 0 and n.value == 8
    assert f(*args(keep=0)) == -1 and f(*args(keep=65)) == -1
    assert f(*args(scores=None)) == -1 and f(*args(out=None)) == -1 and f(*args(cnt=None)) == -1
    assert f(None, C.c_uint64(0), C.c_uint32(0), C.c_uint32(1), capi._fp(idx), C.byref(n)) == 0 and n.value == 0


# ---- the reference search on the analytic room ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def room_layer():
    return A.RefLayer(A.ROOM_VOXEL, *track_ref.analytic_layer_arrays(A.ROOM_VOXEL, truncation=A.ROOM_TRUNCATION))


@functools.lru_cache(maxsize=None)
def room_search(k):
    """the reference search for the k-th seeded true pose (shared with tests/test_gpu_align.py)"""
    true_pose = A.room_true_poses(6)[k]
    pts = A.room_problem(true_pose)
    return true_pose, pts, A.search(room_layer(), pts, (0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP, min_corr=len(pts) // 4, **A.ROOM_SEARCH)


def test_room_layer_is_the_one_the_rule_was_tried_on():
    assert len(room_layer().keys) == 48


@pytest.mark.parametrize("k", range(3))
def test_reference_search_recovers_the_true_pose_within_one_final_step(k):
    true_pose, pts, out = room_search(k)
    assert len(pts) == 300 and np.all(pts[:, 3] == 0) and np.all(pts[:, 4] == 1)
    assert all(abs(t) <= h for t, h in zip(true_pose, A.ROOM_HALF))
    levels = out["levels"]
    assert [lv["n_candidates"] for lv in levels] == [5145, 648, 648, 648, 648]
    assert [lv["inlier_distance"] for lv in levels] == [float(np.float32(v)) for v in (0.4, 0.2, 0.1, 0.1, 0.1)]
    assert np.array_equal(levels[-1]["step"], np.array(A.FINAL_STEP))
    err = A.pose_error_steps(out["poses"][0], true_pose)
    print(f"[reference search {k}] true {np.round(true_pose, 4)} found {np.round(out['poses'][0], 4)} error in final steps {np.round(err, 3)} "
          f"record {out['scores'][0]}")
    assert np.all(err <= 1.0), err
    assert out["scores"][0]["n_corr"] >= len(pts) // 4
    # scores fall along the kept list, and rise from level to level at the same tau
    for lv in levels:
        assert np.all(np.diff(lv["kept_score"]["score"].astype(np.int64)) <= 0)
    assert levels[4]["kept_score"]["score"][0] >= levels[3]["kept_score"]["score"][0] >= levels[2]["kept_score"]["score"][0]
