"""The median and the speckle filter on the disparity of dense stereo, on the GPU, against tests/stereo_filter_ref.py (DESIGN.md section
7n, steps 7a and 7b): through cox_selftest_stereo_filters on images that try the labelling, and as whole frames through
StereoMatcher.  Every comparison is exact, word for word."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_filter_cases as fc
import stereo_filter_ref as fr
import stereo_ref as sr
from coxgraph_amd import capi
from coxgraph_amd.capi import CoxError, Layer, StereoMatcher

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("n_valid_pixels", "n_rejected_uniqueness", "n_rejected_lr", "n_rejected_depth")
FILTERS = dict(median_size=3, speckle_window=20, speckle_range16=16)
ZERO_FILTER_STATS = dict.fromkeys(fr.COUNTS, 0) | dict(median_ms=0.0, speckle_ms=0.0)
MODES = {"median": dict(median_size=3), "speckle": dict(speckle_window=5), "both": dict(median_size=3, speckle_window=5)}
X = fr.INVALID
_REF = {}


# ---- through the self-test entry ---------------------------------------------------------------------------------------------------
def check_filters(hip, d, **cfg):
    """7a and 7b of d on the GPU against the reference: the three images, the four counts, the guards"""
    want = fr.run(d, **cfg)
    status, got = fc.selftest(hip, d, **cfg)
    assert status == 0
    assert got["guards"] == [0, 0, 0]
    assert np.array_equal(got["median"], want["median"]), "median: %d pixels differ" % int(np.sum(got["median"] != want["median"]))
    if want["labels"] is None:
        assert np.all(got["labels"] == fc.FILL32)   # nothing was labelled
    else:
        assert np.array_equal(got["labels"], want["labels"]), "labels: %d pixels differ" % int(np.sum(got["labels"] != want["labels"]))
    assert np.array_equal(got["filtered"], want["filtered"]), "filtered: %d pixels differ" % int(np.sum(got["filtered"] != want["filtered"]))
    assert got["counts"] == want["counts"]
    return want


SHAPE_IDS = ["%dx%d" % s for s in fc.SHAPES]


@pytest.mark.parametrize("w,h", fc.SHAPES, ids=SHAPE_IDS)
def test_plain_images(hip, w, h):
    n = w * h
    check_filters(hip, fc.all_invalid(w, h), median_size=3, speckle_window=n)
    for window in (n - 1, n):
        if window > 0:
            want = check_filters(hip, fc.constant(w, h), median_size=3, speckle_window=window)
            assert want["counts"]["n_components"] == 1 and want["counts"]["n_speckle_pixels"] == (n if window == n else 0)
    want = check_filters(hip, fc.checkerboard(w, h, 100, 117), speckle_window=1, speckle_range16=16)   # 17 apart: every pixel alone
    assert want["counts"]["n_components"] == n and np.all(want["filtered"] == X)
    check_filters(hip, fc.checkerboard(w, h, 100, 116), median_size=3, speckle_window=max(n - 1, 1), speckle_range16=16)
    # the extreme values: 0 and 0xFFFE link at the largest range and at no smaller one
    want = check_filters(hip, fc.checkerboard(w, h, 0, 0xFFFE), speckle_window=1, speckle_range16=0xFFFE)
    assert want["counts"]["n_components"] == 1
    want = check_filters(hip, fc.checkerboard(w, h, 0, 0xFFFE), speckle_window=1, speckle_range16=0xFFFD)
    assert want["counts"]["n_components"] == n
    check_filters(hip, fc.checkerboard(w, h, 0, 0xFFFE), median_size=3, speckle_window=1, speckle_range16=0xFFFD)


@pytest.mark.parametrize("w,h", fc.SHAPES, ids=SHAPE_IDS)
def test_staircases_across_tile_borders(hip, w, h):
    for down in (False, True):
        steps = h if down else w
        want = check_filters(hip, fc.staircase(w, h, 16, down), speckle_window=1, speckle_range16=16)
        assert want["counts"]["n_components"] == 1
        want = check_filters(hip, fc.staircase(w, h, 17, down), speckle_window=w * h // steps, speckle_range16=16)
        assert want["counts"]["n_components"] == steps and np.all(want["filtered"] == X)
        check_filters(hip, fc.staircase(w, h, 17, down), median_size=3, speckle_window=max(w * h // steps - 1, 1), speckle_range16=16)
        want = check_filters(hip, fc.staircase(w, h, 1, down), speckle_window=1, speckle_range16=0)   # range 0 links equal values only
        assert want["counts"]["n_components"] == steps


@pytest.mark.parametrize("w,h", fc.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("image", ["serpentine", "serpentine_down", "spiral", "combs"])
def test_labels_travel_the_whole_chain(hip, image, w, h):
    d = fc.serpentine(w, h, down=True) if image == "serpentine_down" else getattr(fc, image)(w, h)
    n = int(np.sum(d != X))
    want = check_filters(hip, d, speckle_window=n, speckle_range16=16)
    assert want["counts"] == dict(n_median_changed=0, n_components=1, n_speckle_components=1, n_speckle_pixels=n)
    assert np.all(want["labels"][d != X] == 0)
    if n > 1:
        want = check_filters(hip, d, speckle_window=n - 1, speckle_range16=16)
        assert want["counts"]["n_speckle_pixels"] == 0 and np.array_equal(want["filtered"], d)
    check_filters(hip, d, median_size=3, speckle_window=3, speckle_range16=16)


@pytest.mark.parametrize("w,h", fc.SHAPES, ids=SHAPE_IDS)
def test_windows_and_ranges(hip, w, h):
    d = fc.blobs(w, h, seed=w + h)
    n = w * h
    for window in (0, 1, n - 1, n):
        check_filters(hip, d, speckle_window=window, speckle_range16=16)
    for r in (0, 9, 10, 20, 0xFFFE):
        check_filters(hip, d, median_size=3, speckle_window=4, speckle_range16=r)
    check_filters(hip, d, speckle_window=2 ** 31 - 1, speckle_range16=16)
    check_filters(hip, d)   # both off: the image comes back


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("w,h", fc.ODD_SHAPES, ids=["%dx%d" % s for s in fc.ODD_SHAPES])
def test_seeded_images(hip, w, h, mode):
    sizes = set()
    for seed in range(40):
        d = fc.seeded(w, h, seed) if seed % 2 == 0 else fc.blobs(w, h, seed)
        want = check_filters(hip, d, **MODES[mode])
        if want["labels"] is not None:
            ok = want["labels"] != fr.NO_LABEL
            sizes.update(np.unique(fr.sizes(want["labels"])[ok]).tolist())
    if mode != "median" and w * h > 300:
        assert len(sizes) >= 10 and max(sizes) > 20   # many sizes of components, not only single pixels


def test_selftest_refusals(hip):
    d = fc.seeded(33, 9, 0)
    for bad in (dict(median_size=1), dict(median_size=5), dict(median_size=-3), dict(speckle_window=-1), dict(speckle_range16=-1),
                dict(speckle_range16=0xFFFF), dict(reserved=1)):
        assert fc.selftest(hip, d, **bad)[0] == -1, bad
    check_filters(hip, d, median_size=3, speckle_window=7)


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
def reference(left, right, K=sr.SCENE_K, B=sr.SCENE_BASELINE, maps=None, filters=FILTERS, **cfg):
    """fr.match_filtered, computed once per input and configuration and never changed"""
    key = (left.tobytes(), right.tobytes(), left.shape, None if maps is None else (maps[0].tobytes(), maps[1].tobytes()),
           tuple(sorted(filters.items())), tuple(sorted(cfg.items())))
    if key not in _REF:
        out = fr.match_filtered(left, right, K, B, *(maps or (None, None)), **filters, **cfg)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def matcher(hip, w, h, filters=FILTERS, **cfg):
    m = StereoMatcher(hip, w, h, K_rect=sr.SCENE_K, baseline_m=sr.SCENE_BASELINE, **cfg)
    if filters is not None:
        m.set_filters(**filters)
    return m


def same_depth(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def check_frame(m, want, depth, rgba, disparity):
    """stage by stage, so that a mismatch names the first kernel that is wrong"""
    assert np.array_equal(m.download("cost_sum"), want["cost_sum"])
    assert np.array_equal(m.filter_download("disparity_raw"), want["disparity_raw"])
    assert np.array_equal(m.filter_download("disparity_median"), want["disparity_median"])
    if want["labels"] is not None:
        assert np.array_equal(m.filter_download("labels"), want["labels"])
    assert np.array_equal(m.download("disparity"), want["disparity"])
    assert np.array_equal(disparity, want["disparity"]), "disparity: %d pixels differ" % int(np.sum(disparity != want["disparity"]))
    assert same_depth(depth, want["depth"])
    assert np.array_equal(rgba, want["rgba"])
    st, fs = m.last_stats(), m.filter_stats()
    assert {k: st[k] for k in COUNTS} == want["stats"]
    assert {k: fs[k] for k in fr.COUNTS} == want["filter_stats"]
    assert st["frame_ms"] > 0 and st["depth_ms"] >= 0 and fs["median_ms"] >= 0 and fs["speckle_ms"] >= 0
    assert st["frame_ms"] >= fs["median_ms"] + fs["speckle_ms"]


FRAME_SHAPES = [(48, 20, 64), (101, 37, 64), (188, 120, 128)]


@pytest.mark.parametrize("mode", ["median", "speckle", "both"])
@pytest.mark.parametrize("w,h,D", FRAME_SHAPES, ids=["%dx%dx%d" % s for s in FRAME_SHAPES])
def test_filtered_frames_bit_for_bit(hip, w, h, D, mode):
    filters = dict(FILTERS, **{"median": dict(speckle_window=0), "speckle": dict(median_size=0), "both": {}}[mode])
    left, right, _ = sr.scene(w, h)
    want = reference(left, right, filters=filters, n_disparities=D)
    m = matcher(hip, w, h, filters, n_disparities=D)
    f = m.filters
    assert (f.median_size, f.speckle_window, f.speckle_range16, f.reserved) == (filters["median_size"], filters["speckle_window"], 16, 0)
    check_frame(m, want, *m.compute(left, right))
    if mode == "median":
        with pytest.raises(CoxError) as e:
            m.filter_download("labels")      # the frame ran without 7b
        assert e.value.status == -1
    if (w, h) == (188, 120) and mode == "both":
        assert want["filter_stats"]["n_speckle_pixels"] > 0 and want["filter_stats"]["n_median_changed"] > 0
    m.close()


def test_euroc_mapped_full_size_pair(hip):
    chain = sr.euroc_camchain()
    map0, map1, K, B, _ = capi.rectify_maps(hip, chain, 752, 480)
    left, right, _ = sr.scene(752, 480, seed=9)
    cfg = dict(n_disparities=64, n_paths=4)
    want = reference(left, right, K, B, (map0, map1), **cfg)
    assert want["filter_stats"]["n_components"] > 10000 and want["stats"]["n_valid_pixels"] > 10000
    m = StereoMatcher(hip, 752, 480, maps=(map0, map1), K_rect=K, baseline_m=B, **cfg)
    m.set_filters(**FILTERS)
    check_frame(m, want, *m.compute(left, right))
    print("752 x 480:", m.last_stats(), m.filter_stats())
    m.close()


def test_depth_limits_with_filters(hip):
    left, right, _ = sr.scene(160, 96)
    cfg = dict(n_disparities=64, min_depth_m=0.6, max_depth_m=1.6)
    want = reference(left, right, **cfg)
    assert want["stats"]["n_rejected_depth"] > 0 and want["stats"]["n_valid_pixels"] > 0
    m = matcher(hip, 160, 96, **cfg)
    check_frame(m, want, *m.compute(left, right))
    m.close()


def test_switching_on_off_on(hip):
    left, right, _ = sr.scene(160, 96)
    want = reference(left, right, n_disparities=64)
    never = matcher(hip, 160, 96, None, n_disparities=64)
    plain = [a.copy() for a in never.compute(left, right)]
    plain_stats = never.last_stats()
    assert never.filter_stats() == ZERO_FILTER_STATS
    m = matcher(hip, 160, 96, None, n_disparities=64)
    assert m.filter_stats() == ZERO_FILTER_STATS                  # before the first frame
    m.set_filters(**FILTERS)
    check_frame(m, want, *m.compute(left, right))
    m.set_filters()                                               # off
    f = m.filters
    assert (f.median_size, f.speckle_window, f.speckle_range16) == (0, 0, 16)
    off = m.compute(left, right)
    for a, b in zip(off, plain):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))  # word for word the frame of a handle that never had filters
    for which in ("rect_left", "rect_right", "cost_sum", "disparity"):
        assert np.array_equal(m.download(which), never.download(which))
    assert {k: m.last_stats()[k] for k in COUNTS} == {k: plain_stats[k] for k in COUNTS}
    assert m.filter_stats() == ZERO_FILTER_STATS
    buf = np.zeros(160 * 96, np.uint32)
    for which in (0, 1, 2):
        assert hip.fn("stereo_filter_download")(m.h_, which, capi._fp(buf), C.c_uint64(buf.nbytes)) == -1
    assert hip.fn("stereo_set_filters")(m.h_, None) == 0          # NULL: off as well
    m.set_filters(**FILTERS)
    check_frame(m, want, *m.compute(left, right))
    m.close()
    never.close()


def test_the_same_filtered_frame_twice(hip):
    left, right, _ = sr.scene(160, 96)
    other = sr.scene(160, 96, seed=3)
    m = matcher(hip, 160, 96, n_disparities=64)
    first = [a.copy() for a in m.compute(left, right)]
    check_frame(m, reference(other[0], other[1], n_disparities=64), *m.compute(other[0], other[1]))   # leaves nothing behind
    second = m.compute(left, right)
    check_frame(m, reference(left, right, n_disparities=64), *second)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    m.close()


def test_two_filtered_handles_in_flight(hip):
    a, b = sr.scene(160, 96, seed=1), sr.scene(188, 120, seed=2)
    fb = dict(median_size=0, speckle_window=50, speckle_range16=8)
    ma, mb = matcher(hip, 160, 96, n_disparities=64), matcher(hip, 188, 120, fb, n_disparities=128, n_paths=4)
    outs = []
    for _ in range(3):   # three frames each, none waited for until the end
        outs = [ma.compute_async(a[0], a[1]), mb.compute_async(b[0], b[1])]
    ma.sync()
    mb.sync()
    check_frame(ma, reference(a[0], a[1], n_disparities=64), *outs[0])
    check_frame(mb, reference(b[0], b[1], filters=fb, n_disparities=128, n_paths=4), *outs[1])
    ma.close()
    mb.close()


def test_filtered_compute_dev_behind_a_producer_stream_that_is_still_writing(hip):
    import torch
    w, h = 188, 120
    left, right, _ = sr.scene(w, h, seed=6)
    want = reference(left, right, n_disparities=128)
    m = matcher(hip, w, h, n_disparities=128)
    dev = torch.device("cuda")
    pinned = [torch.from_numpy(a).pin_memory() for a in (left, right)]
    left_d, right_d = (torch.full((h, w), 77, dtype=torch.uint8, device=dev) for _ in range(2))
    depth_d = torch.zeros((h, w), dtype=torch.float32, device=dev)
    rgba_d = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)
    disp_d = torch.zeros((h, w), dtype=torch.int16, device=dev)
    busy_src, busy_dst = torch.zeros(64 << 20, dtype=torch.uint8, device=dev), torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy_dst.copy_(busy_src)                    # the producer has work queued in front of the images ...
        left_d.copy_(pinned[0], non_blocking=True)      # ... and writes them last
        right_d.copy_(pinned[1], non_blocking=True)
        m.compute_dev(left_d, right_d, depth_d, rgba_d, disp_d, stream=s)
        left_d.zero_()                                  # the producer reuses the inputs: it waits until the frame has read them
        right_d.zero_()
    m.sync()
    check_frame(m, want, depth_d.cpu().numpy(), rgba_d.cpu().numpy(), disp_d.cpu().numpy().view(np.uint16))
    s.synchronize()
    assert int(left_d.max()) == 0 and int(right_d.max()) == 0
    # the median alone writes the caller's disparity itself; without rgba, on the null stream
    m.set_filters(median_size=3)
    want = reference(left, right, filters=dict(median_size=3), n_disparities=128)
    depth_d.zero_()
    disp_d.zero_()
    left_d.copy_(pinned[0])
    right_d.copy_(pinned[1])
    m.compute_dev(left_d, right_d, depth_d, None, disp_d)
    m.sync()
    assert same_depth(depth_d.cpu().numpy(), want["depth"]) and np.array_equal(disp_d.cpu().numpy().view(np.uint16), want["disparity"])
    m.close()


def test_filtered_depth_and_rgba_go_straight_into_the_depth_fusion(hip):
    import torch
    w, h, voxel = 160, 96, 0.05
    left, right, _ = sr.scene(w, h)
    want = reference(left, right, n_disparities=64)
    m = matcher(hip, w, h, n_disparities=64)
    dev = torch.device("cuda")
    left_d, right_d = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    depth_d = torch.zeros((h, w), dtype=torch.float32, device=dev)
    rgba_d = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    fuse = dict(truncation_distance=0.15, min_depth_m=0.2, max_depth_m=4.0)
    T = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
    on_device, through_host = Layer(hip, voxel), Layer(hip, voxel)
    d1, d2 = on_device.depth_integrator(**fuse), through_host.depth_integrator(**fuse)
    m.compute_dev(left_d, right_d, depth_d, rgba_d)
    d1.integrate_dev(T, depth_d, rgba_d, w, h, sr.SCENE_K, stream=m.stream())   # behind the filtered frame, without the host
    d1.sync()
    depth, rgba = depth_d.cpu().numpy(), rgba_d.cpu().numpy()
    assert same_depth(depth, want["depth"]) and np.array_equal(rgba, want["rgba"])
    d2.integrate(T, depth, rgba, sr.SCENE_K)
    d2.sync()
    (ia, va), (ib, vb) = on_device.download(), through_host.download()
    assert len(ia) > 0 and np.array_equal(ia, ib) and np.array_equal(va, vb)
    for x in (d1, d2, on_device, through_host, m):
        x.close()


def test_filter_refusals_leave_the_handle_usable(hip):
    left, right, _ = sr.scene(160, 96)
    want = reference(left, right, n_disparities=64)
    m = matcher(hip, 160, 96, n_disparities=64)

    def status(**fields):
        c = capi.StereoFilterConfig(**dict(dict(median_size=0, speckle_window=0, speckle_range16=16, reserved=0), **fields))
        return hip.fn("stereo_set_filters")(m.h_, C.byref(c))
    for bad in (dict(median_size=1), dict(median_size=2), dict(median_size=5), dict(median_size=-1), dict(speckle_window=-1), dict(speckle_window=-2 ** 31),
                dict(speckle_range16=-1), dict(speckle_range16=0xFFFF), dict(speckle_range16=2 ** 31 - 1), dict(reserved=1), dict(reserved=2 ** 32 - 1)):
        assert status(**bad) == -1, bad
        f = m.filters
        assert (f.median_size, f.speckle_window, f.speckle_range16, f.reserved) == (3, 20, 16, 0)   # the previous setting
    assert hip.fn("stereo_get_filters")(m.h_, None) == -1 and hip.fn("stereo_filter_last_stats")(m.h_, None) == -1
    assert hip.fn("stereo_set_filters")(None, None) == -1
    buf = np.zeros(160 * 96, np.uint32)
    assert hip.fn("stereo_filter_download")(m.h_, 0, capi._fp(buf), C.c_uint64(buf.nbytes)) == -1   # before the first frame
    check_frame(m, want, *m.compute(left, right))
    for which, need in ((0, 160 * 96 * 2), (1, 160 * 96 * 2), (2, 160 * 96 * 4)):
        assert hip.fn("stereo_filter_download")(m.h_, which, capi._fp(buf), C.c_uint64(need - 1)) == -7
        assert hip.fn("stereo_filter_download")(m.h_, which, capi._fp(buf), C.c_uint64(need)) == 0
    for which in (3, -1, 99):
        assert hip.fn("stereo_filter_download")(m.h_, which, capi._fp(buf), C.c_uint64(buf.nbytes)) == -1
    assert hip.fn("stereo_filter_download")(m.h_, 0, None, C.c_uint64(buf.nbytes)) == -1
    assert status(speckle_window=2 ** 31 - 1, speckle_range16=0xFFFE, median_size=3) == 0              # the ends of the ranges
    depth, _, disparity = m.compute(left, right)
    assert np.all(disparity == X) and np.all(np.isnan(depth)) and m.last_stats()["n_valid_pixels"] == 0
    m.set_filters(**FILTERS)
    check_frame(m, want, *m.compute(left, right))
    m.close()


# ---- C++ ---------------------------------------------------------------------------------------------------------------------------
def test_cpp_set_filters_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "stereo_filter_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "stereo_filter_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
