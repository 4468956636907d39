"""Scan-to-map registration without a GPU: the C ABI of include/coxgraph_hip_track.h and the known answers of the numpy
reference (tests/track_ref.py) that the GPU tests compare against."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import map_ref
import track_ref as R
from coxgraph_amd import synth
from coxgraph_amd.capi import TrackConfig, TrackResult, track_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_track.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def test_track_header_symbols_are_exported(hip):
    syms = _declared_symbols()
    assert syms == ["cox_track_config_default", "cox_track_create", "cox_track_destroy", "cox_track_evaluate_dev", "cox_track_normal_eq_depth_dev",
                    "cox_track_normal_eq_dev", "cox_track_refine", "cox_track_refine_depth_dev", "cox_track_refine_dev"]
    missing = [s for s in syms if not hasattr(hip.lib, s)]
    assert not missing, missing


def test_config_defaults_and_struct_sizes(hip):
    c = track_config(hip)
    got = {n: getattr(c, n) for n, _ in TrackConfig._fields_ if n != "reserved"}
    assert got == R.DEFAULTS
    assert C.sizeof(TrackConfig) == 64 and C.sizeof(TrackResult) == 136  # the layouts of the header


def test_entry_points_fail_cleanly(hip):
    """Without a GPU every call reports COX_ERR_NO_DEVICE (checked first); with one, NULL handles are COX_ERR_INVALID_ARG."""
    f = hip.fn
    want = -2 if hip.device_count() == 0 else -1
    h = C.c_void_p()
    T = (C.c_float * 7)(1, 0, 0, 0, 0, 0, 0)
    K = (C.c_float * 4)(100, 100, 8, 8)
    assert f("track_create")(None, None, C.byref(h)) == want and not h
    assert f("track_evaluate_dev")(None, T, None, C.c_uint64(0), None, None) == want
    assert f("track_normal_eq_dev")(None, T, None, C.c_uint64(0), None, None, None, None) == want
    assert f("track_normal_eq_depth_dev")(None, T, None, C.c_int(16), C.c_int(16), K, None, None, None, None) == want
    assert f("track_refine_dev")(None, T, None, C.c_uint64(0), None, None) == want
    assert f("track_refine")(None, T, None, C.c_uint64(0), None, None) == want
    assert f("track_refine_depth_dev")(None, T, None, C.c_int(16), C.c_int(16), K, None, None) == want
    f("track_destroy", None)(None)


# ---- the reference's known answers ---------------------------------------------------------------------------------------------
def _plane_scan(rng, n_pairs):
    """Points u, -u around the sensor in the plane through it perpendicular to the affine field's gradient a: every point has the
    same distance, and the centroid of the scan is the sensor, so rotations and translations decouple."""
    a = map_ref.AFFINE_A.astype(np.float64)
    e1 = np.cross(a, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    e2 /= np.linalg.norm(e2)
    uv = rng.uniform(-0.9, 0.9, size=(n_pairs, 2))
    u = uv[:, :1] * e1 + uv[:, 1:] * e2
    return np.concatenate([u, -u]).astype(np.float32)


@pytest.mark.parametrize("dof", [4, 6])
def test_reference_on_an_affine_field(dof):
    """d = a . x + c: the trilinear value and its derivative are exact up to float32 rounding, H is the closed form
    sum [a; x_i x a] [a; x_i x a]^T, and one damped step from a scan centred on the sensor is a translation that cancels the
    residual along a.  (With the rule's damping, H + damping diag(H), the step solves (a a^T + damping diag(a a^T)) dt = -r a:
    dt_k = -r / ((3 + damping) a_k), so a . dt = -3 r / (3 + damping); it is parallel to a only under a damping of the identity.)"""
    idx, words = map_ref.affine_layer_arrays()
    L = R.RefLayer(map_ref.AFFINE_VS, idx, words)
    a, c = map_ref.AFFINE_A.astype(np.float64), float(map_ref.AFFINE_C)
    t = np.array([1.6, 1.55, 1.65])
    T = np.array([1, 0, 0, 0, *t], np.float32)
    pts = _plane_scan(np.random.default_rng(1), 500)
    cfg = R.config(dof=dof, min_points=1)
    pp = L.per_point(T, pts)
    assert np.all(pp["status"] == 3)
    exact = pp["pG"].astype(np.float64) @ a + c
    assert np.max(np.abs(pp["d"] - exact)) < 2e-6
    assert np.max(np.abs(pp["g"] - map_ref.AFFINE_A)) < 2e-5
    ne = L.normal_eq(T, pts, cfg)
    assert ne["n_used"] == ne["n_considered"] == len(pts)
    x = pp["pG"].astype(np.float64) - T[4:].astype(np.float64)
    xa = np.cross(x, a)
    J = np.concatenate([np.tile(a, (len(pts), 1)), xa if dof == 6 else xa[:, 2:]], 1)
    H, rbar = J.T @ J, float(a @ T[4:].astype(np.float64) + c)
    assert np.max(np.abs(ne["H"] - H)) < 1e-4 * np.max(np.abs(H))
    assert np.max(np.abs(ne["H"][:3, :3] - len(pts) * np.outer(a, a))) < 1e-4 * len(pts)
    assert abs(ne["cost"] - len(pts) * rbar * rbar) < 1e-4 * len(pts) * rbar * rbar
    delta = np.array(R.solve(ne["H"], ne["b"], cfg["damping"]))
    want = -rbar / ((3.0 + cfg["damping"]) * a)
    assert np.max(np.abs(delta[:3] - want)) < 1e-3 * np.max(np.abs(want))
    assert abs(a @ delta[:3] + 3.0 * rbar / (3.0 + cfg["damping"])) < 1e-4 * abs(rbar)
    assert np.max(np.abs(delta[3:])) < 1e-4  # no rotation
    # ... and the step lands on the zero set: the next evaluation's cost is ~ (damping / 3)^2 of the first one's
    out = L.refine(T, pts, R.config(dof=dof, min_points=1, max_iterations=2))
    assert out["last_cost"] < 1e-8 * out["first_cost"]


@functools.lru_cache(maxsize=None)
def analytic_layer(voxel):
    return R.RefLayer(voxel, *R.analytic_layer_arrays(voxel))


@functools.lru_cache(maxsize=None)
def scan(frame):
    T, pts, _, _ = synth.make_frame(frame)
    return T, pts


@pytest.mark.parametrize("voxel", [0.10, 0.05])
@pytest.mark.parametrize("dof", [4, 6])
def test_reference_recovers_the_corner_view(voxel, dof):
    """Frame 100 sees the front wall, the side wall and the floor / ceiling edge: from 0.5 voxels / 1 degree and from 1.5 voxels /
    3 degrees off, both parameterisations end within 0.1 voxel and 0.05 degrees of the truth, at the same place."""
    L = analytic_layer(voxel)
    T, pts = scan(100)
    ends = []
    for voxels, degrees, sign in ((0.5, 1.0, 1), (1.5, 3.0, -1)):
        T0 = R.start_pose(T, voxel, dof, voxels, degrees, sign)
        out = L.refine(T0, pts, R.config(dof=dof, stride=16))
        et, er = R.pose_error(out["T"], T)
        print(f"voxel {voxel} dof {dof} start {voxels} voxels / {degrees} deg: {out['iterations']} iterations, error {et * 1e3:.2f} mm {er:.4f} deg")
        assert out["status"] == R.CONVERGED and out["iterations"] <= 8
        assert et < 0.1 * voxel and er < 0.05
        assert out["last_cost"] < out["first_cost"] and out["last_n_used"] == out["last_n_considered"] == len(pts[::16])
        ends.append(out["T"])
    dt, dr = R.pose_error(ends[0], ends[1])
    assert dt < 1e-4 and np.radians(dr) < 1e-4  # the stop tolerances


def test_reference_converges_on_the_wall_and_sphere_view_with_4_dof():
    """Frame 25 sees one wall and the sphere: x, y, z and yaw are constrained (6 DoF is not: the smallest eigenvalue of H is
    four orders below the largest, and nothing is asserted about it)."""
    L = analytic_layer(0.10)
    T, pts = scan(25)
    out = L.refine(R.start_pose(T, 0.10, 4, 0.5, 1.0), pts, R.config(dof=4, stride=16))
    et, er = R.pose_error(out["T"], T)
    print(f"{out['iterations']} iterations, error {et * 1e3:.2f} mm {er:.4f} deg")
    assert out["status"] == R.CONVERGED and et < 0.1 * 0.10 and er < 0.05
    ne = L.normal_eq(T, pts, R.config(dof=6, stride=16))
    ev = np.linalg.eigvalsh(ne["H"])
    assert ev[0] < 1e-3 * ev[-1]


def test_reference_reports_lost_outside_the_layer_and_degenerate_on_one_plane():
    L = analytic_layer(0.10)
    T, pts = scan(100)
    far = np.array(T)
    far[4:] += np.float32(50.0)
    out = L.refine(far, pts, R.config(stride=16))
    assert out["status"] == R.LOST and out["iterations"] == 1 and out["last_n_used"] == 0 and out["last_n_considered"] == len(pts[::16])
    assert np.array_equal(out["T"], far.astype(np.float64))
    # non-finite points are not considered; none considered -> lost as well
    out = L.refine(T, np.full((64, 3), np.nan, np.float32), R.config())
    assert out["status"] == R.LOST and out["last_n_considered"] == 0
    # H = 0 (min_points 0 lets it through): the first pivot is not positive
    out = L.refine(far, pts, R.config(stride=16, min_points=0, min_inlier_ratio=0.0))
    assert out["status"] == R.DEGENERATE and np.array_equal(out["T"], far.astype(np.float64))
    # max_iterations reached
    out = L.refine(R.start_pose(T, 0.10, 4, 1.5, 3.0), pts, R.config(stride=16, max_iterations=2))
    assert out["status"] == R.MAX_ITERATIONS and out["iterations"] == 2


def test_reference_options():
    """Huber weights, the distance gate and the stride do what the rule says."""
    L = analytic_layer(0.10)
    T, pts = scan(100)
    T0 = R.start_pose(T, 0.10, 6, 1.0, 2.0)
    plain = L.normal_eq(T0, pts, R.config(dof=6, stride=97))
    pp = L.per_point(T0, pts, 97)
    used = (pp["status"] & R.USED) != 0
    assert plain["n_considered"] == len(pts[::97]) and plain["n_used"] == int(used.sum())
    d = pp["d"][used].astype(np.float64)
    assert abs(plain["cost"] - float(np.sum(d * d))) <= 1e-12 * plain["cost"]
    hub = L.normal_eq(T0, pts, R.config(dof=6, stride=97, huber_delta=0.05))
    w = np.where(np.abs(d) > 0.05, 0.05 / np.abs(d), 1.0)
    assert (w < 1).any() and abs(hub["cost"] - float(np.sum(w * d * d))) <= 1e-12 * hub["cost"] and hub["n_used"] == plain["n_used"]
    gate = L.normal_eq(T0, pts, R.config(dof=6, stride=97, max_abs_distance=0.05))
    assert gate["n_used"] == int((np.abs(pp["d"][used]) <= np.float32(0.05)).sum()) < plain["n_used"] and gate["n_considered"] == plain["n_considered"]
    # the order of the sum changes the last bits at the most
    rev = L.normal_eq(T0, pts, R.config(dof=6, stride=97), "reverse")
    bound = plain["n_used"] * 2.0 ** -52 * plain["abs"][0]
    assert np.all(np.abs(rev["H"] - plain["H"]) <= bound)
