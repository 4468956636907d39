"""Dense stereo as far as it goes without a GPU: the C ABI of include/coxgraph_hip_stereo.h (symbols, layouts,
defaults, the device check), cox_stereo_rectify_maps against its numpy twin on the EuRoC camchain, properties of step R, the
matcher's reference on the shared scene, and the C++ wrapper."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stereo_ref as sr
from coxgraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cox_stereo_compute", "cox_stereo_compute_dev", "cox_stereo_config_default", "cox_stereo_create", "cox_stereo_destroy",
           "cox_stereo_download", "cox_stereo_last_stats", "cox_stereo_rectify_maps", "cox_stereo_stream", "cox_stereo_sync"]
W, H = 752, 480


# ---- 1. the header -----------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "coxgraph_hip_stereo.h")).read()


def test_stereo_header_symbols_are_exported(hip):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))
    assert syms == SYMBOLS
    assert not [s for s in syms if not hasattr(hip.lib, s)]


def test_default_config_is_the_references(hip):
    c = capi.stereo_config(hip)
    for k, v in sr.DEFAULTS.items():
        got = getattr(c, k)
        assert got == (np.float32(v) if isinstance(v, float) else v), (k, got, v)
    assert [n for n, _ in capi.StereoConfig._fields_] == list(sr.DEFAULTS)
    assert (c.n_disparities, c.n_paths, c.p1, c.p2, c.uniqueness_percent, c.lr_max_diff, c.min_depth_m, c.max_depth_m) == (128, 8, 7, 86, 10, 1, 0.0, np.inf)


@pytest.mark.parametrize("mine,ref,size", [(capi.StereoConfig, sr.Config, 36), (capi.StereoStats, sr.Stats, 80), (capi.StereoCamera, sr.Camera, 72),
                                           (capi.StereoCalibration, sr.Calibration, 272)], ids=["config", "stats", "camera", "calibration"])
def test_structures_have_the_references_layout(mine, ref, size):
    assert C.sizeof(mine) == C.sizeof(ref) == size
    assert [n for n, _ in mine._fields_] == [n for n, _ in ref._fields_]
    for n, _ in ref._fields_:
        assert getattr(mine, n).offset == getattr(ref, n).offset and getattr(mine, n).size == getattr(ref, n).size, n


def test_the_header_states_the_structures_in_that_order():
    text = _header()
    for name, ref in (("cox_stereo_config", sr.Config), ("cox_stereo_stats", sr.Stats), ("cox_stereo_camera", sr.Camera),
                      ("cox_stereo_calibration", sr.Calibration)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [n for n, _ in ref._fields_]
    for name, value in (("COX_STEREO_RECT_LEFT", sr.RECT_LEFT), ("COX_STEREO_RECT_RIGHT", sr.RECT_RIGHT), ("COX_STEREO_COST_SUM", sr.COST_SUM),
                        ("COX_STEREO_DISPARITY", sr.DISPARITY)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
        assert capi.STEREO_BUFFERS[name[len("COX_STEREO_"):].lower()] == value


def test_create_fails_cleanly_without_a_gpu(hip):
    h = C.c_void_p()
    K = np.array([100, 100, 40, 30], np.float32)
    if hip.device_count() > 0:   # with a device the argument check is reached
        assert hip.fn("stereo_create")(0, 0, 10, None, None, None, capi._fp(K), C.c_float(0.1), C.byref(h)) == -1 and not h
        return
    assert hip.fn("stereo_create")(0, 64, 48, None, None, None, capi._fp(K), C.c_float(0.1), C.byref(h)) == -2 and not h
    with pytest.raises(capi.CoxError) as e:
        capi.StereoMatcher(hip, 64, 48, K_rect=K, baseline_m=0.1)
    assert e.value.status == -2
    assert hip.fn("stereo_sync")(None) == -2
    assert hip.fn("stereo_compute")(None, None, None, None, None, None) == -2
    assert hip.fn("stereo_compute_dev")(None, None, None, None, None, None, None) == -2
    assert hip.fn("stereo_last_stats")(None, None) == -2
    assert hip.fn("stereo_download")(None, 0, None, C.c_uint64(0)) == -2
    assert not hip.fn("stereo_stream", C.c_void_p)(None)
    hip.fn("stereo_destroy", None)(None)


# ---- 2. cox_stereo_rectify_maps against the twin ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def euroc(hip):
    chain = sr.euroc_camchain()
    return chain, capi.rectify_maps(hip, chain, W, H), sr.rectify_maps(chain, W, H)


def test_rectify_maps_equal_the_twins_on_the_euroc_camchain(euroc):
    chain, got, want = euroc
    assert chain["cam0"]["resolution"] == [W, H] and chain["cam1"]["resolution"] == [W, H]
    for g, r in zip(got[:2], want[:2]):
        assert g.shape == r.shape == (H, W, 2) and g.dtype == np.float32
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(r))
        err = float(np.max(np.abs(g.astype(np.float64) - r.astype(np.float64))))
        print("largest map difference [px]:", err)
        assert err <= 2.0 ** -13
    # B and f: both sides narrow a float64 that agrees to 1e-9 to float32, so the float32 values are equal or one ulp apart ...
    assert abs(float(got[2][0]) - float(want[2][0])) <= 2.0 ** -15 and abs(got[3] - float(want[3])) <= 2.0 ** -27
    # ... and the float64 values behind them are those of the issue
    _, f, cx, cy, B, _, _ = sr.rectification(chain)
    assert abs(B - 0.110078) < 1e-6 and abs(f - 457.41775) < 1e-9 * f
    assert abs(float(got[2][0]) - f) <= 1e-7 * f and abs(got[3] - B) <= 1e-7 * B   # float32 of them
    assert np.array_equal(got[2], want[2]) and got[2][0] == got[2][1]
    assert np.max(np.abs(got[4] - want[4])) <= 1e-7 and np.all(got[4][4:] == 0) and abs(np.linalg.norm(got[4][:4]) - 1) < 1e-6


def test_every_euroc_pixel_maps_inside_its_source_image(euroc):
    _, got, _ = euroc
    for m in got[:2]:
        assert m[..., 0].min() >= 0 and m[..., 0].max() <= W - 1 and m[..., 1].min() >= 0 and m[..., 1].max() <= H - 1


def test_rectify_maps_with_a_scale_and_its_statuses(hip):
    chain = sr.euroc_camchain()
    got, want = capi.rectify_maps(hip, chain, 376, 240, 0.5), sr.rectify_maps(chain, 376, 240, 0.5)
    assert max(float(np.nanmax(np.abs(g.astype(np.float64) - r))) for g, r in zip(got[:2], want[:2])) <= 2.0 ** -13
    assert np.array_equal(got[2], want[2])

    def status(chain, w=16, h=12, scale=1.0):
        try:
            capi.rectify_maps(hip, chain, w, h, scale)
        except capi.CoxError as e:
            return e.status
        return 0
    assert status(chain) == 0
    assert status(dict(chain, cam0=dict(chain["cam0"], distortion_model="equidistant"))) == -6
    assert status(dict(chain, cam1=dict(chain["cam1"], camera_model="omni"))) == -6
    assert status(dict(chain, cam1=dict(chain["cam1"], distortion_model="no such model"))) == -6
    assert status(chain, w=0) == -1 and status(chain, h=2 ** 15 + 1) == -1 and status(chain, scale=0.0) == -1 and status(chain, scale=np.nan) == -1
    assert status(dict(chain, cam0=dict(chain["cam0"], intrinsics=[0.0, 457.0, 367.0, 248.0]))) == -1
    assert status(dict(chain, cam1=dict(chain["cam1"], T_cn_cnm1=np.eye(4).tolist()))) == -1   # no baseline
    K, B, T = np.zeros(4, np.float32), C.c_float(), np.zeros(7, np.float32)
    assert hip.fn("stereo_rectify_maps")(None, 4, 4, C.c_double(1.0), None, None, capi._fp(K), C.byref(B), capi._fp(T)) == -1


# ---- 3. properties of step R, on the twin ----------------------------------------------------------------------------------------
def test_an_ideal_pair_gives_identity_maps_exactly(hip):
    chain = sr.ideal_camchain()
    u, v = np.meshgrid(np.arange(80, dtype=np.float32), np.arange(60, dtype=np.float32))
    for maps in (sr.rectify_maps(chain, 80, 60), capi.rectify_maps(hip, chain, 80, 60)):
        for m in maps[:2]:
            assert np.array_equal(m[..., 0], u) and np.array_equal(m[..., 1], v)
        assert np.array_equal(maps[2], np.array([100, 100, 40, 30], np.float32)) and maps[3] == np.float32(0.1)
        assert np.array_equal(maps[4], np.array([1, 0, 0, 0, 0, 0, 0], np.float32))


def test_the_maps_are_the_raw_projections_of_rectified_points():
    chain = sr.euroc_camchain()
    Rr, f, cx, cy, B, R, t = sr.rectification(chain)
    assert np.max(np.abs(Rr @ Rr.T - np.eye(3))) < 1e-12 and abs(np.linalg.det(Rr) - 1) < 1e-12   # rows orthonormal, right-handed
    rng = np.random.default_rng(5)
    P = np.stack([rng.uniform(-1.5, 1.5, 100), rng.uniform(-1.0, 1.0, 100), rng.uniform(2.0, 8.0, 100)], 1)   # in the rectified left frame
    u0, v0 = f * P[:, 0] / P[:, 2] + cx, f * P[:, 1] / P[:, 2] + cy
    # the same points seen from the rectified right camera: moved by the baseline along x
    u1, v1 = f * (P[:, 0] - B) / P[:, 2] + cx, v0
    assert np.max(np.abs((u0 - u1) - f * B / P[:, 2])) <= 1e-9 * np.max(u0 - u1)   # the disparity is f B / Z
    P0 = P @ Rr            # rows: R_rect^T P, in cam0
    P1 = P0 @ R.T + t      # in cam1
    worst = 0.0
    for i, (Pc, u, v) in enumerate(((P0, u0, v0), (P1, u1, v1))):
        raw = sr.distort_project(chain["cam%d" % i], Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2])
        got = sr.map_at(chain, i, u, v)
        worst = max(worst, float(np.max(np.abs(np.stack(got) - np.stack(raw)))))
    print("largest projection difference [px]:", worst)
    assert worst <= 1e-6


# ---- 4. the matcher's reference on the scene -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_paths", [8, 4])
def test_the_reference_finds_the_scene(n_paths):
    left, right, truth = sr.scene(160, 96)
    out = sr.match(left, right, sr.SCENE_K, sr.SCENE_BASELINE, n_disparities=64, n_paths=n_paths)
    d = out["disparity"]
    valid = d != sr.INVALID
    share, close = float(valid.mean()), float((np.abs(d[valid].astype(np.int64) - 16 * truth[valid]) <= 16).mean())
    print("valid: %.1f %%, of them within 1 px: %.1f %%" % (100 * share, 100 * close))
    assert share >= 0.70 and close >= 0.95
    assert np.array_equal(np.isnan(out["depth"]), ~valid) and out["stats"]["n_valid_pixels"] == int(valid.sum())
    fB16 = np.float32(float(sr.SCENE_K[0]) * float(sr.SCENE_BASELINE) * 16.0)
    assert np.array_equal(out["depth"][valid], fB16 / d[valid].astype(np.float32))
    assert out["cost_sum"].max() <= n_paths * (62 + 86) + 62 and out["cost_sum"].max() <= 2536
    assert np.array_equal(out["rgba"][..., 0], left) and np.all(out["rgba"][..., 3] == 255)


def test_subpixel_division_truncates_toward_zero():
    S = np.array([[[30, 10, 12, 40], [12, 10, 30, 40]]], np.int32)   # num = 18 * 16 + 22 = 310; num = -18 * 16 + 22 = -266
    d0, m0, _ = sr.winner(S, 0)
    assert np.array_equal(sr.subpixel(S, d0, m0.astype(np.int64)), [[16 + 310 // 44, 16 - (266 // 44)]])


# ---- 5. edge inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [sr.constant_pair, sr.stripes_pair], ids=["constant", "stripes"])
def test_ambiguous_pairs_give_no_valid_pixel(pair):
    left, right = pair(160, 96)
    out = sr.match(left, right, sr.SCENE_K, sr.SCENE_BASELINE, n_disparities=64)
    assert not np.any(out["disparity"] != sr.INVALID) and np.all(np.isnan(out["depth"])) and out["stats"]["n_valid_pixels"] == 0


def test_images_too_small_for_a_census_give_nothing():
    left, right, _ = sr.scene(8, 6)
    out = sr.match(left, right, sr.SCENE_K, sr.SCENE_BASELINE, n_disparities=64)
    assert np.all(out["disparity"] == sr.INVALID) and np.all(out["cost_sum"] == 8 * 62)


# ---- 6. the C++ wrapper ------------------------------------------------------------------------------------------------------------
def test_cpp_dense_stereo_compiles_and_its_maps_are_the_c_entrys(hip, tmp_path):
    exe = str(tmp_path / "stereo_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "stereo_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    # 0: all of it, on a GPU; 77: the host part passed and there is no GPU
    assert out.returncode == (0 if hip.device_count() > 0 else 77), out.stdout + out.stderr
