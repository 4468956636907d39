"""The observation-history rule by hand (tests/history_ref.py restates it in numpy, DESIGN.md section 7f defines it) and the C ABI of
include/coxgraph_hip_history.h -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import history_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)


def _words(*bits):
    m = np.zeros(8, np.uint32)
    for b in bits:
        m[b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    return m


def test_a_point_marks_a_named_block_cell_and_bit():
    """10 cm voxels, identity pose: (0.57, -0.33, 2.05) m scales to (5.7, -3.3, 20.5) -> voxel (5, -4, 20): block (0, -1, 1);
    local (5, 12, 4) -> cell (1, 3, 1) = 1 + 4 * 3 + 16 * 1 = 29.  Frame 37 is bit 5 of word 1."""
    rec = hr.Record(0.10)
    rec.mark(IDENTITY, [[0.57, -0.33, 2.05]], 37, 0.2, 10.0)
    idx, masks = rec.arrays()
    assert idx.tolist() == [[0, -1, 1]]
    want = np.zeros((64, 8), np.uint32)
    want[29, 1] = 1 << 5
    assert np.array_equal(masks[0], want)
    # the pose moves it: a quarter turn about z (x -> y, y -> -x) and 1.6 m along x put it at (1.6 + 0.33, 0.57, 2.05):
    # voxel (19, 5, 20) -> block (1, 0, 1), local (3, 5, 4) -> cell (0, 1, 1) = 20
    s = np.float32(np.sqrt(0.5))
    rec = hr.Record(0.10)
    rec.mark(np.array([s, 0, 0, s, 1.6, 0, 0], np.float32), [[0.57, -0.33, 2.05]], 0, 0.2, 10.0)
    idx, masks = rec.arrays()
    assert idx.tolist() == [[1, 0, 1]] and np.flatnonzero(masks[0].any(axis=1)).tolist() == [20] and masks[0][20, 0] == 1


def test_two_frames_share_a_cell_and_blocks_sort_by_z_y_x():
    rec = hr.Record(0.10)
    rec.mark(IDENTITY, [[0.05, 0.05, 1.0], [0.35, 0.05, 1.0]], 3, 0.2, 10.0)   # same cell (voxels 0 and 3 along x)
    rec.mark(IDENTITY, [[0.05, 0.05, 1.0], [1.65, 0.05, 0.5]], 4, 0.2, 10.0)   # + block (1, 0, 0)
    idx, masks = rec.arrays()
    assert idx.tolist() == [[0, 0, 0], [1, 0, 0]]
    cell = 0 + 4 * 0 + 16 * 2  # local z = 10 -> 2
    assert masks[0][cell, 0] == (1 << 3) | (1 << 4) and np.count_nonzero(masks[0]) == 1
    assert masks[1][0 + 16 * 1, 0] == 1 << 4


def test_points_outside_the_range_or_not_finite_leave_nothing():
    for p in ([0.0, 0.0, 0.19], [0.0, 0.0, 10.01], [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, -np.inf]):
        rec = hr.Record(0.10)
        rec.mark(IDENTITY, [p], 0, 0.2, 10.0)
        assert rec.arrays()[0].shape == (0, 3), p
    rec = hr.Record(0.10)
    rec.mark(IDENTITY, [[0.0, 0.0, 0.2], [0.0, 0.0, 10.0]], 0, 0.2, 10.0)  # both limits are inside
    assert len(rec.arrays()[0]) == 2
    rec = hr.Record(0.10)
    rec.mark(IDENTITY, [[0.0, 0.0, 1.0]], 0, 0.2, 10.0, freespace=True)   # every point of a freespace cloud is a clearing ray
    assert rec.arrays()[0].shape == (0, 3)


def test_run_length_encoding_by_hand():
    assert hr.runs_of_mask(_words()) == []
    assert hr.runs_of_mask(np.array([0b01110110, 0, 0, 0, 0, 0, 0, 0], np.uint32)) == [[1, 2], [4, 6]]
    assert hr.runs_of_mask(_words(30, 31, 32, 33)) == [[30, 33]]      # across bits 31 / 32: one run
    assert hr.runs_of_mask(_words(31)) == [[31, 31]] and hr.runs_of_mask(_words(32)) == [[32, 32]]
    assert hr.runs_of_mask(_words(255)) == [[255, 255]]
    assert hr.runs_of_mask(np.full(8, 0xFFFFFFFF, np.uint32)) == [[0, 255]]
    assert hr.runs_of_mask(_words(0, 2, 63, 64, 254, 255)) == [[0, 0], [2, 2], [63, 64], [254, 255]]


def test_triangle_history_is_the_union_of_its_vertices_cells():
    rec = hr.Record(0.10)
    rec.mark(IDENTITY, [[0.05, 0.05, 1.0]], 1, 0.2, 10.0)
    rec.mark(IDENTITY, [[0.45, 0.05, 1.0]], 2, 0.2, 10.0)   # the next cell along x
    rec.mark(IDENTITY, [[0.45, 0.05, 1.0]], 7, 0.2, 10.0)
    idx, masks = rec.arrays()
    tri = np.array([[0.05, 0.05, 1.0], [0.06, 0.05, 1.0], [0.05, 0.06, 1.0],     # inside the first cell
                    [0.35, 0.05, 1.0], [0.45, 0.05, 1.0], [0.35, 0.06, 1.0],     # across both
                    [5.0, 5.0, 5.0], [5.1, 5.0, 5.0], [5.0, 5.1, 5.0]], np.float32)  # in a block nobody saw
    tm = hr.triangle_masks(tri, 0.10, idx, masks)
    hb, hist, has = hr.encode(tm, [0, 6, 9])
    assert hb.tolist() == [0, 2, 6, 6] and hist.tolist() == [1, 1, 1, 2, 7, 7] and has.tolist() == [1, 0]


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_history.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def test_history_header_symbols_are_exported(hip):
    syms = _declared_symbols()
    assert len(syms) >= 14 and "cox_obs_create" in syms and "cox_integrator_attach_history" in syms and "cox_meshlayer_history" in syms
    missing = [s for s in syms if not hasattr(hip.lib, s)]
    assert not missing, missing


def test_history_entry_points_fail_cleanly(hip):
    """Without a GPU the constructor says COX_ERR_NO_DEVICE whatever it is handed; NULL handles -> COX_ERR_INVALID_ARG."""
    f = hip.fn
    h, u = C.c_void_p(), C.c_uint64()
    T = (C.c_float * 7)(1, 0, 0, 0, 0, 0, 0)
    st = f("obs_create")(None, C.c_uint64(0), C.byref(h))
    assert st == (-2 if hip.device_count() == 0 else -1)
    assert f("obs_clear")(None) == -1 and f("obs_sync")(None) == -1 and f("obs_set_frame")(None, C.c_uint32(0)) == -1
    assert f("obs_set_auto_grow")(None, C.c_int(0)) == -1
    assert f("obs_stats")(None, C.byref(u), None, None) == -1 and f("obs_counts")(None, None, None) == -1
    assert f("obs_download")(None, None, None, C.c_uint64(0), C.byref(u)) == -1
    assert f("obs_record")(None, T, None, C.c_uint64(0), C.c_int(0), C.c_float(0.1), C.c_float(5.0), C.c_int(1)) == -1
    assert f("obs_record_dev")(None, T, None, C.c_uint64(0), C.c_int(0), C.c_float(0.1), C.c_float(5.0), C.c_int(1), None) == -1
    assert f("integrator_attach_history")(None, None) == -1
    assert f("meshlayer_history_size")(None, None, C.byref(u), C.byref(u), None) == -1
    assert f("meshlayer_history")(None, None, None, None, None, C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)) == -1
    f("obs_destroy", None)(None)


def test_history_smoke_compiles_and_reports_no_gpu(hip, tmp_path):
    exe = str(tmp_path / "history_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "history_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    rc = subprocess.call([exe])
    assert rc == (0 if hip.device_count() > 0 else 77)
