"""Dense stereo on the GPU against tests/stereo_ref.py: every comparison is exact, on the rectified images, the
cost sums S, the disparity, the depth (as uint32 words; NaN by isnan), rgba and the counts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_ref as sr
from coxgraph_amd import capi
from coxgraph_amd.capi import CoxError, Layer, StereoMatcher

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("n_valid_pixels", "n_rejected_uniqueness", "n_rejected_lr", "n_rejected_depth")
_REF = {}


def reference(left, right, maps=None, **cfg):
    """sr.match, computed once per input and configuration and never changed"""
    key = (left.tobytes(), right.tobytes(), left.shape, None if maps is None else (maps[0].tobytes(), maps[1].tobytes()), tuple(sorted(cfg.items())))
    if key not in _REF:
        out = sr.match(left, right, sr.SCENE_K, sr.SCENE_BASELINE, *(maps or (None, None)), **cfg)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def matcher(hip, w, h, maps=None, **cfg):
    return StereoMatcher(hip, w, h, maps=maps, K_rect=sr.SCENE_K, baseline_m=sr.SCENE_BASELINE, **cfg)


def same_depth(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def check_outputs(want, depth, rgba, disparity):
    assert np.array_equal(disparity, want["disparity"]), "disparity: %d pixels differ" % int(np.sum(disparity != want["disparity"]))
    assert same_depth(depth, want["depth"])
    assert np.array_equal(rgba, want["rgba"])


def check_frame(m, want, depth, rgba, disparity):
    """stage by stage, so that a mismatch names the first kernel that is wrong"""
    assert np.array_equal(m.download("rect_left"), want["rect_left"])
    assert np.array_equal(m.download("rect_right"), want["rect_right"])
    S = m.download("cost_sum")
    assert np.array_equal(S, want["cost_sum"]), "S: %d cells differ" % int(np.sum(S != want["cost_sum"]))
    assert np.array_equal(m.download("disparity"), want["disparity"])
    check_outputs(want, depth, rgba, disparity)
    st = m.last_stats()
    assert {k: st[k] for k in COUNTS} == want["stats"]
    assert st["frame_ms"] > 0 and all(st[k] >= 0 for k in ("remap_ms", "census_ms", "paths_ms", "winner_ms", "depth_ms"))


def run_case(hip, left, right, maps=None, **cfg):
    h, w = left.shape
    want = reference(left, right, maps, **cfg)
    m = matcher(hip, w, h, maps, **cfg)
    check_frame(m, want, *m.compute(left, right))
    m.close()
    return want


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(160, 96, 64), (101, 37, 64), (48, 20, 64), (300, 40, 256), (200, 9, 128), (64, 7, 64), (9, 7, 64), (8, 6, 64), (188, 120, 128)]


@pytest.mark.parametrize("w,h,D", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_shapes_bit_for_bit(hip, w, h, D):
    left, right, _ = sr.scene(w, h)
    want = run_case(hip, left, right, n_disparities=D)
    n_valid = int(np.sum(want["disparity"] != sr.INVALID))
    print("valid pixels:", n_valid)
    if (w, h) in ((9, 7), (8, 6)):
        assert n_valid == 0 and np.all(np.isnan(want["depth"]))
    if (w, h) in ((160, 96), (188, 120), (64, 7)):
        assert n_valid > 0


# ---- 2. parameters -----------------------------------------------------------------------------------------------------------------
PARAMS = [dict(n_paths=4), dict(n_paths=8), dict(p1=0, p2=0), dict(p1=7, p2=86), dict(p1=255, p2=255), dict(uniqueness_percent=0),
          dict(uniqueness_percent=10), dict(uniqueness_percent=50), dict(lr_max_diff=-1), dict(lr_max_diff=0), dict(lr_max_diff=1),
          dict(min_depth_m=0.6, max_depth_m=1.6), dict(min_depth_m=1.0), dict(max_depth_m=1.0), dict(n_paths=4, p1=3, p2=200, uniqueness_percent=99, lr_max_diff=5)]


@pytest.mark.parametrize("cfg", PARAMS, ids=["-".join("%s=%s" % kv for kv in c.items()) for c in PARAMS])
def test_parameters_bit_for_bit(hip, cfg):
    left, right, _ = sr.scene(160, 96)
    want = run_case(hip, left, right, n_disparities=64, **cfg)
    if "min_depth_m" in cfg or "max_depth_m" in cfg:
        assert want["stats"]["n_rejected_depth"] > 0 and want["stats"]["n_valid_pixels"] > 0   # the limits reject some pixels, not all
    if cfg.get("lr_max_diff", 1) < 0:
        assert want["stats"]["n_rejected_lr"] == 0


@pytest.mark.parametrize("pair", [sr.constant_pair, sr.stripes_pair], ids=["constant", "stripes"])
def test_ambiguous_pairs_bit_for_bit(hip, pair):
    left, right = pair(160, 96)
    want = run_case(hip, left, right, n_disparities=64)
    assert want["stats"]["n_valid_pixels"] == 0


# ---- 3. remap ----------------------------------------------------------------------------------------------------------------------
def identity_maps(w, h):
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return np.stack([u, v], -1).copy()


def test_identity_maps_give_the_input_back(hip):
    left, right, _ = sr.scene(101, 37)
    ident = identity_maps(101, 37)
    want = run_case(hip, left, right, (ident, ident), n_disparities=64)
    assert np.array_equal(want["rect_left"], left) and np.array_equal(want["rect_right"], right)
    plain = reference(left, right, n_disparities=64)   # NULL maps: the same frame, nothing masked either way
    for k in ("cost_sum", "disparity", "rgba"):
        assert np.array_equal(want[k], plain[k])
    run_case(hip, left, right, n_disparities=64)


def edge_maps(w, h, seed):
    """fractions on and next to the 1/64 rounding boundaries, the last column and row, and entries that are no pixel at all"""
    rng = np.random.default_rng(seed)
    m = identity_maps(w, h)
    j = rng.integers(0, 64, (h, w, 2)).astype(np.float32) / np.float32(64.0)     # multiples of 1/64: odd ones are ties of the rounding
    m = m * np.float32(0.75) + j
    side = rng.integers(0, 3, (h, w, 2))
    m = np.where(side == 0, np.nextafter(m, np.float32(-np.inf)), np.where(side == 1, np.nextafter(m, np.float32(np.inf)), m)).astype(np.float32)
    last = np.array([w - 1, h - 1], np.float32)
    special = [np.array([np.nan, 3.0]), np.array([3.0, np.nan]), np.array([np.inf, 2.0]), np.array([2.0, -np.inf]), np.array([-1 / 128, 5.0]),
               np.array([-1 / 64, 5.0]), np.array([-1 / 32, 5.0]), np.array([5.0, -1 / 32]), np.array([-3.0, -3.0]), np.array([1e30, 1.0]),
               np.array([3.0e38, 1.0]), np.array([1.0, -1e30]), last, last + np.array([1 / 128, 0]), last + np.array([1 / 64, 0]),
               last + np.array([0, 1 / 64]), last + np.array([0, 1 / 128]), last - np.array([1 / 64, 1 / 64]), np.array([w - 1, 0.5]),
               np.array([w, 1.0]), np.array([1.0, h]), np.array([0.0, 0.0]), np.array([w - 1.5, h - 1.5])]
    for k, s in enumerate(special * 3):
        m[(5 * k + 2) % h, (7 * k + 3) % w] = s.astype(np.float32)
    return m


def test_remap_at_rounding_boundaries_and_outside_the_source(hip):
    w, h = 90, 41
    left, right, _ = sr.scene(w, h, seed=4)
    maps = (edge_maps(w, h, 1), edge_maps(w, h, 2))
    want = run_case(hip, left, right, maps, n_disparities=64)
    _, masked = sr.remap(left, maps[0])
    assert 20 <= int(masked.sum()) < w * h // 2   # some entries are outside, most are not
    assert np.any(want["rect_left"] != left)


def test_euroc_maps_on_a_full_size_pair(hip):
    chain = sr.euroc_camchain()
    map0, map1, K, B, T = capi.rectify_maps(hip, chain, 752, 480)
    rng = np.random.default_rng(9)
    left, right = rng.integers(0, 256, (480, 752), dtype=np.uint8), rng.integers(0, 256, (480, 752), dtype=np.uint8)
    m = StereoMatcher(hip, 752, 480, calibration=chain, n_disparities=64, n_paths=4)
    assert np.array_equal(m.K_rect, K) and m.baseline_m == B and np.array_equal(m.T_c0_rect, T)
    m.compute(left, right)
    for which, img, mp in (("rect_left", left, map0), ("rect_right", right, map1)):
        want, masked = sr.remap(img, mp)
        assert not masked.any()
        assert np.array_equal(m.download(which), want), which
    m.close()


# ---- 4. orders ---------------------------------------------------------------------------------------------------------------------
def test_the_same_frame_twice_gives_the_same_bits(hip):
    left, right, _ = sr.scene(160, 96)
    want = reference(left, right, n_disparities=64)
    m = matcher(hip, 160, 96, n_disparities=64)
    first = [a.copy() for a in m.compute(left, right)]
    other = sr.scene(160, 96, seed=3)
    between = m.compute(other[0], other[1])             # another frame in between leaves nothing behind
    check_frame(m, reference(other[0], other[1], n_disparities=64), *between)
    second = m.compute(left, right)
    check_frame(m, want, *second)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    m.close()


def test_two_handles_with_frames_in_flight_at_once(hip):
    a, b = sr.scene(160, 96, seed=1), sr.scene(188, 120, seed=2)
    ma, mb = matcher(hip, 160, 96, n_disparities=64), matcher(hip, 188, 120, n_disparities=128, n_paths=4)
    outs = []
    for _ in range(3):   # three frames each, none waited for until the end
        outs = [ma.compute_async(a[0], a[1]), mb.compute_async(b[0], b[1])]
    ma.sync()
    mb.sync()
    check_frame(ma, reference(a[0], a[1], n_disparities=64), *outs[0])
    check_frame(mb, reference(b[0], b[1], n_disparities=128, n_paths=4), *outs[1])
    ma.close()
    mb.close()


def test_compute_dev_behind_a_producer_stream_that_is_still_writing(hip):
    import torch
    w, h = 188, 120
    left, right, _ = sr.scene(w, h, seed=6)
    want = reference(left, right, n_disparities=128)
    m = matcher(hip, w, h, n_disparities=128)
    host = m.compute(left, right)
    check_outputs(want, *host)
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
    # without rgba and disparity, on the null stream
    depth_d.zero_()
    left_d.copy_(pinned[0])
    right_d.copy_(pinned[1])
    m.compute_dev(left_d, right_d, depth_d)
    m.sync()
    assert same_depth(depth_d.cpu().numpy(), want["depth"]) and same_depth(depth_d.cpu().numpy(), host[0])
    m.close()


# ---- 5. downstream -----------------------------------------------------------------------------------------------------------------
def test_depth_and_rgba_go_straight_into_the_depth_fusion(hip):
    import torch
    w, h, voxel = 160, 96, 0.05
    left, right, truth = sr.scene(w, h)
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
    d1.integrate_dev(T, depth_d, rgba_d, w, h, sr.SCENE_K, stream=m.stream())   # behind the frame, without the host
    d1.sync()
    depth, rgba = depth_d.cpu().numpy(), rgba_d.cpu().numpy()
    assert same_depth(depth, want["depth"]) and np.array_equal(rgba, want["rgba"])
    d2.integrate(T, depth, rgba, sr.SCENE_K)
    d2.sync()
    (ia, va), (ib, vb) = on_device.download(), through_host.download()
    assert len(ia) > 0 and np.array_equal(ia, ib) and np.array_equal(va, vb)
    # the plane at disparity 8: the zero crossing along the ray of a background pixel, in front of the camera
    u, v = 30, 10
    assert truth[v, u] == sr.BACKGROUND and np.isfinite(depth[v, u])
    z_plane = float(sr.SCENE_K[0]) * float(sr.SCENE_BASELINE) / sr.BACKGROUND
    z = np.arange(z_plane - 0.14, z_plane + 0.14, 0.005)
    pts = np.stack([(u - sr.SCENE_K[2]) / sr.SCENE_K[0] * z, (v - sr.SCENE_K[3]) / sr.SCENE_K[1] * z, z], 1).astype(np.float32)
    q = on_device.query(pts, mode="interpolate")
    ok = (q["status"] & capi.Q_VALUE) != 0
    zs, ds = z[ok], q["distance"][ok]
    k = np.nonzero((ds[:-1] > 0) & (ds[1:] <= 0))[0]
    assert len(k) >= 1
    k = k[0]
    z_cross = zs[k] + (zs[k + 1] - zs[k]) * ds[k] / (ds[k] - ds[k + 1])
    print("zero crossing at %.4f m, plane at %.4f m" % (z_cross, z_plane))
    assert abs(z_cross - z_plane) <= voxel
    for x in (d1, d2, on_device, through_host, m):
        x.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(hip):
    def create_status(w=64, h=48, maps=None, K=sr.SCENE_K, B=sr.SCENE_BASELINE, device=0, **cfg):
        try:
            StereoMatcher(hip, w, h, maps=maps, K_rect=K, baseline_m=B, device=device, **cfg).close()
        except CoxError as e:
            return e.status
        return 0
    assert create_status() == 0
    for bad in (dict(w=0), dict(h=0), dict(w=-3), dict(w=2 ** 15 + 1, h=1), dict(w=1, h=2 ** 15 + 1), dict(w=2 ** 15, h=2 ** 10, n_disparities=128),
                dict(w=2 ** 15, h=2 ** 9 + 1, n_disparities=128), dict(w=2 ** 12 + 1, h=2 ** 12, n_disparities=128),
                dict(n_disparities=100), dict(n_disparities=32), dict(n_disparities=512), dict(n_paths=5), dict(n_paths=0), dict(p1=-1),
                dict(p1=90, p2=86), dict(p2=256), dict(uniqueness_percent=100), dict(uniqueness_percent=-1), dict(reserved=1), dict(min_depth_m=-1.0),
                dict(min_depth_m=2.0, max_depth_m=1.0), dict(max_depth_m=np.nan), dict(K=np.array([0, 120, 80, 48], np.float32)),
                dict(K=np.array([np.inf, 120, 80, 48], np.float32)), dict(B=0.0), dict(B=-0.1), dict(B=np.nan), dict(device=99), dict(device=-1)):
        assert create_status(**bad) == -1, bad
    # one map without the other
    ident = identity_maps(64, 48)
    h_ = C.c_void_p()
    K = np.ascontiguousarray(sr.SCENE_K)
    for a, b in ((capi._fp(ident), None), (None, capi._fp(ident))):
        assert hip.fn("stereo_create")(0, 64, 48, None, a, b, capi._fp(K), C.c_float(0.1), C.byref(h_)) == -1 and not h_
    assert hip.fn("stereo_create")(0, 64, 48, None, None, None, None, C.c_float(0.1), C.byref(h_)) == -1 and not h_
    assert hip.fn("stereo_create")(0, 64, 48, None, None, None, capi._fp(K), C.c_float(0.1), None) == -1

    left, right, _ = sr.scene(160, 96)
    want = reference(left, right, n_disparities=64)
    m = matcher(hip, 160, 96, n_disparities=64)
    buf = np.zeros(160 * 96 * 64, np.uint16)
    assert m.last_stats() == dict.fromkeys(COUNTS, 0) | dict.fromkeys(("remap_ms", "census_ms", "paths_ms", "winner_ms", "depth_ms", "frame_ms"), 0.0)
    assert hip.fn("stereo_download")(m.h_, 0, capi._fp(buf), C.c_uint64(buf.nbytes)) == -1       # before the first frame
    depth = np.zeros((96, 160), np.float32)
    for args in ((None, capi._fp(right), capi._fp(depth)), (capi._fp(left), None, capi._fp(depth)), (capi._fp(left), capi._fp(right), None)):
        assert hip.fn("stereo_compute")(m.h_, *args, None, None) == -1
        assert hip.fn("stereo_compute_dev")(m.h_, *args, None, None, None) == -1
    assert hip.fn("stereo_compute")(None, capi._fp(left), capi._fp(right), capi._fp(depth), None, None) == -1
    assert hip.fn("stereo_sync")(None) == -1 and hip.fn("stereo_last_stats")(m.h_, None) == -1 and hip.fn("stereo_last_stats")(None, None) == -1
    assert hip.fn("stereo_download")(m.h_, 0, capi._fp(buf), C.c_uint64(buf.nbytes)) == -1       # the refused calls enqueued no frame
    check_frame(m, want, *m.compute(left, right))                                                # usable afterwards
    for which, need in ((0, 160 * 96), (1, 160 * 96), (2, 160 * 96 * 64 * 2), (3, 160 * 96 * 2)):
        assert hip.fn("stereo_download")(m.h_, which, capi._fp(buf), C.c_uint64(need - 1)) == -7
        assert hip.fn("stereo_download")(m.h_, which, capi._fp(buf), C.c_uint64(need)) == 0
    assert hip.fn("stereo_download")(m.h_, 4, capi._fp(buf), C.c_uint64(buf.nbytes)) == -1
    assert hip.fn("stereo_download")(m.h_, -1, capi._fp(buf), C.c_uint64(buf.nbytes)) == -1
    assert hip.fn("stereo_download")(m.h_, 0, None, C.c_uint64(buf.nbytes)) == -1
    # compute without rgba and disparity
    assert hip.fn("stereo_compute")(m.h_, capi._fp(left), capi._fp(right), capi._fp(depth), None, None) == 0
    m.sync()
    assert same_depth(depth, want["depth"])
    check_frame(m, want, *m.compute(left, right))
    m.close()
    m.close()   # twice is fine


# ---- 7. C++ ------------------------------------------------------------------------------------------------------------------------
def test_cpp_dense_stereo_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "stereo_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "stereo_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
