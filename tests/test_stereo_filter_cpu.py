"""The filters on the disparity of dense stereo as far as they go without a GPU: the C ABI of
include/coxgraph_hip_stereo_filter.h, the numpy reference (tests/stereo_filter_ref.py) against closed forms worked out by hand, the
reference on the shared scene, and the C++ wrapper."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stereo_filter_ref as fr
import stereo_ref as sr
from coxgraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cox_stereo_filter_config_default", "cox_stereo_filter_download", "cox_stereo_filter_last_stats", "cox_stereo_get_filters",
           "cox_stereo_set_filters"]
OLD_SYMBOLS = ["cox_stereo_compute", "cox_stereo_compute_dev", "cox_stereo_config_default", "cox_stereo_create", "cox_stereo_destroy",
               "cox_stereo_download", "cox_stereo_last_stats", "cox_stereo_rectify_maps", "cox_stereo_stream", "cox_stereo_sync"]
X = fr.INVALID


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def img(rows):
    return np.array(rows, np.uint16)


# ---- 1. the ABI --------------------------------------------------------------------------------------------------------------------
def test_filter_header_symbols_are_exported(hip):
    assert _declared("coxgraph_hip_stereo_filter.h") == SYMBOLS
    assert not [s for s in SYMBOLS if not hasattr(hip.lib, s)]
    assert "cox_selftest_stereo_filters" in _declared("coxgraph_hip_selftest.h") and hasattr(hip.lib, "cox_selftest_stereo_filters")
    import __graft_entry__ as entry
    assert "coxgraph_hip_stereo_filter.h" in entry.PUBLIC_HEADERS


def test_the_stereo_header_still_declares_what_it_did():
    assert _declared("coxgraph_hip_stereo.h") == OLD_SYMBOLS


@pytest.mark.parametrize("mine,ref,size", [(capi.StereoFilterConfig, fr.Config, 16), (capi.StereoFilterStats, fr.Stats, 48)], ids=["config", "stats"])
def test_filter_structures_have_the_stated_layout(mine, ref, size):
    assert C.sizeof(mine) == C.sizeof(ref) == size
    assert [n for n, _ in mine._fields_] == [n for n, _ in ref._fields_]
    for n, _ in ref._fields_:
        assert getattr(mine, n).offset == getattr(ref, n).offset and getattr(mine, n).size == getattr(ref, n).size, n
    assert [n for n, _ in capi.StereoFilterConfig._fields_] == ["median_size", "speckle_window", "speckle_range16", "reserved"]
    assert [n for n, _ in capi.StereoFilterStats._fields_] == ["n_median_changed", "n_components", "n_speckle_components", "n_speckle_pixels",
                                                              "median_ms", "speckle_ms"]
    text = _header("coxgraph_hip_stereo_filter.h")
    name = "cox_stereo_filter_config" if mine is capi.StereoFilterConfig else "cox_stereo_filter_stats"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in ref._fields_]


def test_filter_defaults_are_both_off(hip):
    c = capi.StereoFilterConfig(9, 9, 9, 9)
    hip.fn("stereo_filter_config_default", None)(C.byref(c))
    assert (c.median_size, c.speckle_window, c.speckle_range16, c.reserved) == (0, 0, 16, 0)
    assert {k: getattr(c, k) for k in fr.DEFAULTS} == fr.DEFAULTS
    hip.fn("stereo_filter_config_default", None)(None)
    for name, value in (("DISPARITY_RAW", fr.DISPARITY_RAW), ("DISPARITY_MEDIAN", fr.DISPARITY_MEDIAN), ("LABELS", fr.LABELS)):
        assert re.search(r"\bCOX_STEREO_FILTER_%s = %d\b" % (name, value), _header("coxgraph_hip_stereo_filter.h")), name
        assert capi.STEREO_FILTER_BUFFERS[name.lower()] == value


def test_filter_entries_fail_cleanly_without_a_gpu(hip):
    want = -1 if hip.device_count() > 0 else -2   # with a device the argument check is reached
    c, st = capi.StereoFilterConfig(), capi.StereoFilterStats()
    assert hip.fn("stereo_set_filters")(None, C.byref(c)) == want
    assert hip.fn("stereo_set_filters")(None, None) == want
    assert hip.fn("stereo_get_filters")(None, C.byref(c)) == want
    assert hip.fn("stereo_filter_last_stats")(None, C.byref(st)) == want
    assert hip.fn("stereo_filter_download")(None, 0, None, C.c_uint64(0)) == want
    d = np.zeros((2, 2), np.uint16)
    med, out, lab, counts, guards = d.copy(), d.copy(), np.zeros((2, 2), np.uint32), np.zeros(4, np.uint64), np.zeros(3, np.uint32)
    args = (C.c_int(2), C.c_int(2), C.byref(c), capi._fp(med), capi._fp(lab), capi._fp(out), capi._fp(counts), capi._fp(guards))
    if hip.device_count() > 0:
        assert hip.lib.cox_selftest_stereo_filters(0, None, *args) == -1
    else:
        assert hip.lib.cox_selftest_stereo_filters(0, capi._fp(d), *args) == -2


# ---- 2. the reference against closed forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,want", [
    ([[X, X, X], [X, 50, X], [X, X, X]], 50),              # n = 1: rank 0, the pixel itself
    ([[X, 70, X], [X, 30, X], [X, X, X]], 30),             # n = 2: rank 0, the lower of the two
    ([[10, X, 40], [X, 30, X], [20, X, X]], 20),           # n = 4: 10 20 30 40, rank 1: the lower median
    ([[10, X, 40], [X, 30, X], [20, X, 50]], 30),          # n = 5: 10 20 30 40 50, rank 2
    ([[90, 10, 80], [20, 70, 30], [60, 40, 50]], 50),      # n = 9: rank 4
    ([[0, X, X], [X, 0xFFFE, X], [X, X, 0xFFFE]], 0xFFFE),  # n = 3 with the extreme values: 0 FFFE FFFE, rank 1
], ids=["n1", "n2", "n4", "n5", "n9", "extremes"])
def test_median_rank_rule(window, want):
    d = img(window)
    out = fr.median3(d)
    assert out[1, 1] == want
    keep = np.ones((3, 3), bool)
    keep[1, 1] = False
    assert np.array_equal(out[keep], d[keep])   # the eight others are border pixels


def test_median_leaves_borders_and_invalid_pixels_alone():
    d = img([[5, 900, 5, 5, 5], [900, 5, 5, X, 5], [5, 5, 900, 5, 5], [5, 5, 5, 5, 900]])
    out = fr.median3(d)
    border = np.ones(d.shape, bool)
    border[1:-1, 1:-1] = False
    assert np.array_equal(out[border], d[border])                        # 900 on the border stays
    assert out[1, 3] == X                                                # invalid stays invalid: nothing is filled
    assert out[2, 2] == 5 and out[1, 1] == 5 and out[1, 2] == 5 and out[2, 1] == 5 and out[2, 3] == 5
    for small in (img([[7]]), img([[7, 900]]), img([[7, 900], [900, 7]]), img([[7], [900], [7]])):
        assert np.array_equal(fr.median3(small), small)                  # no pixel off the border
    assert fr.run(d, median_size=3)["counts"]["n_median_changed"] == 1   # only the 900 in the middle


def test_staircase_links_along_the_chain():
    r = 16
    stairs = img([[100 + r * k for k in range(8)]])
    assert np.array_equal(fr.labels(stairs, r), np.zeros((1, 8), np.uint32))              # steps of exactly the range: one component
    steep = img([[100 + (r + 1) * k for k in range(8)]])
    assert np.array_equal(fr.labels(steep, r), np.arange(8, dtype=np.uint32)[None, :])    # one more: one component per step
    assert np.array_equal(fr.labels(stairs.T.copy(), r), np.zeros((8, 1), np.uint32))
    assert np.array_equal(fr.labels(steep, 0), np.arange(8, dtype=np.uint32)[None, :])
    assert np.array_equal(fr.labels(img([[4, 4, 4, 5]]), 0), img([[0, 0, 0, 3]]))         # range 0 links equal values only


def test_diagonal_contact_does_not_link():
    d = img([[8, 8, X, X], [8, 8, X, X], [X, X, 8, 8], [X, X, 8, 8]])
    lab = fr.labels(d, 16)
    N = fr.NO_LABEL
    assert np.array_equal(lab, np.array([[0, 0, N, N], [0, 0, N, N], [N, N, 10, 10], [N, N, 10, 10]], np.uint32))
    assert fr.run(d, speckle_window=3)["counts"] == dict(n_median_changed=0, n_components=2, n_speckle_components=0, n_speckle_pixels=0)
    assert np.all(fr.speckle(d, 4, 16) == X)


def test_window_is_the_largest_size_removed():
    d = img([[8, 8, 8, X, 300, 300, 300, 300]])   # components of 3 and of 4 pixels
    assert np.array_equal(fr.speckle(d, 3, 16), img([[X, X, X, X, 300, 300, 300, 300]]))   # exactly `window`: removed; window + 1: kept
    assert np.array_equal(fr.speckle(d, 2, 16), d)
    assert np.all(fr.speckle(d, 4, 16) == X)
    r = fr.run(d, speckle_window=3)
    assert r["counts"] == dict(n_median_changed=0, n_components=2, n_speckle_components=1, n_speckle_pixels=3)
    assert np.array_equal(fr.run(d, speckle_window=0)["filtered"], d) and fr.run(d)["labels"] is None


def test_labels_are_the_least_index_of_the_component():
    # a hook whose least index (1) is reached last from its other end: 7 - 11 - 10 - 9 - 5 - 1
    d = img([[X, 8, X, X], [X, 8, X, 8], [X, 8, 8, 8]])
    lab = fr.labels(d, 16)
    assert np.array_equal(lab[d != X], np.full(6, 1, np.uint32)) and np.all(lab[d == X] == fr.NO_LABEL)
    assert np.array_equal(fr.sizes(lab)[d != X], np.full(6, 6))


# ---- 3. the reference on the scene -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
def test_the_filtered_reference_finds_the_scene_with_fewer_outliers(noisy):
    seed = 0
    left, right, truth = sr.scene(160, 96, seed=seed)
    if noisy:
        noise = np.random.default_rng(1000 + seed).integers(-12, 13, right.shape)
        right = np.clip(right.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    out = fr.match_filtered(left, right, sr.SCENE_K, sr.SCENE_BASELINE, median_size=3, speckle_window=20, speckle_range16=16, n_disparities=64, n_paths=8)
    raw, d = out["disparity_raw"], out["disparity"]
    valid = d != fr.INVALID
    share, close = float(valid.mean()), float((np.abs(d[valid].astype(np.int64) - 16 * truth[valid]) <= 16).mean())
    before, after = fr.outliers(raw, truth), fr.outliers(d, truth)
    print("valid: %.1f %%, of them within 1 px: %.1f %%, outliers %d -> %d, filter counts %s" % (100 * share, 100 * close, before, after, out["filter_stats"]))
    assert share >= 0.70 and close >= 0.95
    assert after < before
    assert np.array_equal(np.isnan(out["depth"]), ~valid) and out["stats"]["n_valid_pixels"] == int(valid.sum())
    assert np.all(d[~(raw != fr.INVALID)] == fr.INVALID)   # nothing is filled
    plain = sr.match(left, right, sr.SCENE_K, sr.SCENE_BASELINE, n_disparities=64, n_paths=8)
    assert np.array_equal(raw, plain["disparity"])
    for k in ("n_rejected_uniqueness", "n_rejected_lr"):
        assert out["stats"][k] == plain["stats"][k]
    off = fr.match_filtered(left, right, sr.SCENE_K, sr.SCENE_BASELINE, n_disparities=64, n_paths=8)   # both off: the frame of sr.match
    assert np.array_equal(off["disparity"], plain["disparity"]) and off["stats"] == plain["stats"]
    assert np.array_equal(off["depth"].view(np.uint32), plain["depth"].view(np.uint32))


# ---- 4. the C++ wrapper ------------------------------------------------------------------------------------------------------------
def test_cpp_filter_wrapper_compiles_and_runs_its_host_part(hip, tmp_path):
    exe = str(tmp_path / "stereo_filter_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "stereo_filter_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    # 0: all of it, on a GPU; 77: the host part passed and there is no GPU
    assert out.returncode == (0 if hip.device_count() > 0 else 77), out.stdout + out.stderr
