"""Scan-to-map registration on the GPU (coxgraph_amd/csrc/cox_track.hip) against the numpy reference (tests/track_ref.py).

Compared exactly: every per-point value and decision (status, p_G, d, g -- float32 on both sides), n_used and n_considered,
status and iteration count of a refinement, and -- bit for bit -- two runs of the same call.  Compared within a bound: the
float64 sums H, b and cost, per entry n * 2^-52 * sum |terms| (what reordering a float64 sum of n terms can do; the terms
themselves are the same products on both sides), and the refined pose.  The bound of a pose is 8 times the reference's own spread
under reversed summation order on that case, measured on the CPU and written down below, and never less than the stop tolerances:
two runs that stop by the same rule may differ by a step the rule accepts.  It never comes from the GPU's result.

`PYTHONPATH=.:tests python tests/test_gpu_track.py` prints the measured spreads and decision margins below (no GPU needed; the
fused layer is then fused by the CPU checker).
"""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import track_ref as R
from coxgraph_amd import synth
from coxgraph_amd.capi import TRACK_GRID_PASS, CoxError, Integrator, Layer, Tracker
from util import run_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAME = 100   # the corner view: front wall, side wall, floor / ceiling edge
STRIDE = 16
# Starts (voxels off, degrees off, sign) per case for track_ref.start_pose, or explicit (dt [m], rotation vector [rad]); chosen
# so that no step of the reference's run is within a factor 2 of a stop tolerance (decision_margin below).
STARTS = {
    ("analytic", 0.10, 4): [(0.5, 1.0, 1), (0.5, 1.0, -1)],
    ("analytic", 0.10, 6): [(0.5, 1.0, -1), (1.0, 2.0, 1)],
    ("analytic", 0.05, 4): [(0.5, 1.0, 1), (0.5, 1.0, -1)],
    ("analytic", 0.05, 6): [(0.5, 1.0, -1), (1.0, 2.0, 1)],
    ("fused", 0.10, 4): [((-0.091, -0.038, -0.022), (0.0, 0.0, 0.0298)), ((-0.034, 0.062, 0.119), (0.0, 0.0, 0.0275))],
    ("fused", 0.10, 6): [(0.7, 1.5, -1), ((-0.128, -0.03, -0.036), (0.0273, -0.0136, -0.0043))],
}
# Measured on the CPU with measure() below: per case and start, |forward - reverse| of the reference's end pose
# (translation [m], rotation [rad]) and the decision margin of the forward run.
MEASURED = {
    ("analytic", 0.10, 4): [(4.6e-15, 2.1e-15, 8.9), (7.9e-15, 2.7e-15, 9.6)],
    ("analytic", 0.10, 6): [(1.1e-14, 2.8e-15, 10.0), (1.9e-14, 6.0e-15, 9.5)],
    ("analytic", 0.05, 4): [(6.3e-15, 2.1e-15, 10.7), (7.9e-15, 2.7e-15, 19.6)],
    ("analytic", 0.05, 6): [(1.0e-14, 2.7e-15, 14.6), (4.6e-15, 1.5e-15, 12.2)],
    ("fused", 0.10, 4): [(6.0e-15, 1.9e-15, 2.3), (1.9e-14, 5.6e-15, 2.4)],
    ("fused", 0.10, 6): [(2.2e-15, 6.7e-16, 2.4), (3.0e-15, 1.8e-15, 2.2)],
}
CASES = sorted(STARTS)


def start(case, k, T):
    kind, voxel, dof = case
    s = STARTS[case][k]
    if len(s) == 3:
        return R.start_pose(T, voxel, dof, *s)
    return R.perturbed(T, s[0], s[1])


def pose_bound(case, k, cfg):
    st, sr, _ = MEASURED[case][k]
    return max(8.0 * st, cfg["translation_tolerance"]), max(8.0 * sr, cfg["rotation_tolerance"])


def pose_diff(Ta, Tb):
    dt, deg = R.pose_error(Ta, Tb)
    return dt, math.radians(deg)


@functools.lru_cache(maxsize=None)
def scan(frame=FRAME):
    T, pts, _, _ = synth.make_frame(frame)
    return T, pts


def fused_frames(eng):
    return run_frames(eng, "merged", 0.10, range(80, 121, 5), capacity_blocks=8192)[0]


def measure():
    from coxgraph_amd.capi import Engine
    oracle = Engine(os.path.join(ROOT, "oracle", "libcoxoracle.so"), "coxo_")
    T, pts = scan()
    layers = {("analytic", v): R.RefLayer(v, *R.analytic_layer_arrays(v)) for v in (0.10, 0.05)}
    layers[("fused", 0.10)] = R.RefLayer(0.10, *fused_frames(oracle).download())
    for case in CASES:
        L, row = layers[case[:2]], []
        for k in range(2):
            cfg = R.config(dof=case[2], stride=STRIDE)
            f, r = (L.refine(start(case, k, T), pts, cfg, o) for o in ("forward", "reverse"))
            dt, dr = pose_diff(f["T"], r["T"])
            row.append("(%.1e, %.1e, %.1f)" % (dt, dr, R.decision_margin(f["steps"], cfg)))
            assert f["status"] == r["status"] == R.CONVERGED and f["iterations"] == r["iterations"]
        print(f"    {case}: [{', '.join(row)}],")


if __name__ == "__main__":
    measure()


# ---- layers shared by the tests: the engine's and the reference's copy of each ------------------------------------------------------
@pytest.fixture(scope="module")
def layers(hip):
    out = {}
    for voxel in (0.10, 0.05):
        idx, words = R.analytic_layer_arrays(voxel)
        layer = Layer(hip, voxel, capacity_blocks=len(idx) + 8)
        layer.upload(idx, words)
        out[("analytic", voxel)] = (layer, R.RefLayer(voxel, idx, words))
    layer = fused_frames(hip)
    out[("fused", 0.10)] = (layer, R.RefLayer(0.10, *layer.download()))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- per point --------------------------------------------------------------------------------------------------------------------
def _point_sets(rng, voxel):
    bs = np.float32(voxel) * np.float32(16)
    uniform = rng.uniform([-5.5, -4.5, -1.5], [5.5, 4.5, 4.5], size=(6000, 3)).astype(np.float32)  # beyond the room on every side
    near = rng.uniform([-4.2, -3.2, -0.2], [4.2, 3.2, 3.2], size=(3000, 3)).astype(np.float32)
    near[np.arange(3000), rng.integers(0, 3, 3000)] = rng.choice(np.array([-4.0, 4.0, -3.0, 3.0, 0.0], np.float32), 3000)  # on a surface-ish plane
    face = rng.uniform([-4.2, -3.2, -0.2], [4.2, 3.2, 3.2], size=(1500, 3)).astype(np.float32)
    k = rng.integers(-4, 5, 1500).astype(np.float32) * bs  # exactly on a block face
    ax = rng.integers(0, 3, 1500)
    face[np.arange(1500), ax] = k
    up, down = face.copy(), face.copy()
    up[np.arange(1500), ax] = np.nextafter(k, np.float32(np.inf))
    down[np.arange(1500), ax] = np.nextafter(k, np.float32(-np.inf))
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan, np.nan, np.nan], [3e6, 0, 1], [0, -3e6, 1], [1, 1, 3.4e38],
                    [1e30, 1e30, 1e30]], np.float32)
    return np.concatenate([uniform, near, face, up, down, bad])


@pytest.mark.parametrize("kind,voxel", [("analytic", 0.10), ("analytic", 0.05), ("fused", 0.10)])
def test_evaluate_is_bit_identical_to_the_reference(hip, layers, kind, voxel):
    layer, ref = layers[(kind, voxel)]
    pts = _point_sets(np.random.default_rng(11), voxel)
    identity = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)  # p_G = p_C: the block faces are met exactly
    tilted = R.start_pose(scan()[0], voxel, 6, 1.0, 2.0)
    T_scan, scan_pts = scan()
    for T, p, cfg in ((identity, pts, {}), (identity, pts, dict(stride=3, max_abs_distance=0.5 * voxel)), (tilted, pts, {}),
                      (tilted, scan_pts[::7], dict(stride=2))):  # the last one: a scan, where every considered point may be used
        tr = Tracker(hip, layer, **cfg)
        got, exp = tr.evaluate(T, p), ref.per_point(T, p, cfg.get("stride", 1), cfg.get("max_abs_distance", 0.0))
        assert np.array_equal(got["status"], exp["status"])
        cons, used = (got["status"] & R.CONSIDERED) != 0, (got["status"] & R.USED) != 0
        assert np.array_equal(_bits(got["pG"][cons]), _bits(exp["pG"][cons])) and np.isnan(got["pG"][~cons]).all()
        assert np.array_equal(_bits(got["d"][used]), _bits(exp["d"][used])) and np.isnan(got["d"][~used]).all()
        assert np.array_equal(_bits(got["g"][used]), _bits(exp["g"][used])) and np.isnan(got["g"][~used]).all()
        q = layer.query(got["pG"][used], "interpolate")
        if not cfg.get("max_abs_distance"):
            # used <=> the interpolated query answers (for the finite, in-range p_G of considered points)
            qa = layer.query(np.nan_to_num(got["pG"][cons], nan=1e30, posinf=1e30, neginf=-1e30), "interpolate")
            assert np.array_equal((qa["status"] & 1) != 0, used[cons])
        assert np.all(q["status"] & 1) and np.array_equal(_bits(q["distance"]), _bits(got["d"][used]))
        print(f"{kind} {voxel} {cfg}: {int(cons.sum())} considered, {int(used.sum())} used of {len(p)}")
        assert 0 < used.sum() and (used.sum() < cons.sum() or p is not pts)
    assert (got["status"][1::2] == 0).all()  # stride 2: odd indices are not considered


# ---- normal equations ------------------------------------------------------------------------------------------------------------------
def _check_normal_eq(got, exp, n, what):
    assert got["n_used"] == exp["n_used"] and got["n_considered"] == exp["n_considered"], what
    aH, ab, ac = exp["abs"]
    eps = n * 2.0 ** -52
    eH, eb, ec = np.abs(got["H"] - exp["H"]), np.abs(got["b"] - exp["b"]), abs(got["cost"] - exp["cost"])
    print(f"{what}: used {got['n_used']} of {got['n_considered']}, max error / bound: H {np.max(eH / np.maximum(eps * aH, 1e-300)):.3g}, "
          f"b {np.max(eb / np.maximum(eps * ab, 1e-300)):.3g}, cost {ec / max(eps * ac, 1e-300):.3g}")
    assert np.all(eH <= eps * aH) and np.all(eb <= eps * ab) and ec <= eps * ac, what


VARIANTS = [dict(), dict(stride=3, huber_delta=0.05), dict(stride=97, max_abs_distance=0.1), dict(stride=3, huber_delta=0.02, max_abs_distance=0.15)]


@pytest.mark.parametrize("dof", [4, 6])
@pytest.mark.parametrize("kind", ["analytic", "fused"])
def test_normal_equations_match_the_reference(hip, layers, kind, dof):
    layer, ref = layers[(kind, 0.10)]
    T, pts = scan()
    T0 = R.start_pose(T, 0.10, dof, 1.0, 2.0)
    mid = len(pts) // 2 + 300  # a run of pixels across the middle of the image
    for var in VARIANTS:
        tr = Tracker(hip, layer, dof=dof, **var)
        cfg = R.config(dof=dof, **var)
        sizes = [0, 1, 63, 64, 65, 255, 256, 257] if not var else [257 * var["stride"]]
        for n in sizes + [20000]:
            p = pts[mid:mid + n]
            got = tr.normal_eq(T0, p)
            _check_normal_eq(got, ref.normal_eq(T0, p, cfg), len(p), f"{kind} dof {dof} {var} n {len(p)}")
            again = tr.normal_eq(T0, p)
            assert all(_same_bits(got[k], again[k]) for k in ("H", "b")) and got["cost"] == again["cost"]
            if n == 0:
                assert not got["H"].any() and not got["b"].any() and got["cost"] == 0.0 and got["n_considered"] == 0
    # more candidates than one pass of the grid covers: the same workgroups walk the scan twice
    tr = Tracker(hip, layer, dof=dof)
    p = pts[:TRACK_GRID_PASS + 300]
    got = tr.normal_eq(T0, p)
    _check_normal_eq(got, ref.normal_eq(T0, p, R.config(dof=dof)), len(p), f"{kind} dof {dof} n {len(p)} (two passes)")
    assert got["n_considered"] == TRACK_GRID_PASS + 300
    assert _same_bits(got["H"], tr.normal_eq(T0, p)["H"])


# ---- refine ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-dof{c[2]}")
def test_refine_follows_the_reference(hip, layers, case):
    kind, voxel, dof = case
    layer, ref = layers[(kind, voxel)]
    T, pts = scan()
    cfg = R.config(dof=dof, stride=STRIDE)
    tr = Tracker(hip, layer, dof=dof, stride=STRIDE)
    ends = []
    for k in range(2):
        T0 = start(case, k, T)
        exp = ref.refine(T0, pts, cfg)
        margin = R.decision_margin(exp["steps"], cfg)
        got = tr.refine(T0, pts)
        bt, br = pose_bound(case, k, cfg)
        dt, dr = pose_diff(got["T"], exp["T"])
        et, er = R.pose_error(got["T"], T)
        print(f"{case} start {k}: {got['status_name']} after {got['iterations']} iterations (reference {exp['iterations']}, margin {margin:.1f}), "
              f"|T - reference| {dt:.2e} m {dr:.2e} rad (bound {bt:.1e}, {br:.1e}), to truth {et * 1e3:.2f} mm {er:.4f} deg, {got['kernel_ms']:.3f} ms")
        assert margin > 2.0, "the start is too close to a stop decision for iteration counts to be compared"
        assert exp["status"] == R.CONVERGED
        assert got["status"] == exp["status"] and got["iterations"] == exp["iterations"]
        assert dt <= bt and dr <= br
        for key in ("first_n_used", "first_n_considered", "last_n_used", "last_n_considered"):
            assert got[key] == exp[key], key
        assert abs(got["first_cost"] - exp["first_cost"]) <= len(pts) * 2.0 ** -52 * exp["first_cost"]
        assert abs(got["last_step_translation"] - exp["last_step_translation"]) <= bt and abs(got["last_step_rotation"] - exp["last_step_rotation"]) <= br
        assert np.array_equal(got["T_refined"], got["T"].astype(np.float32)) and abs(np.linalg.norm(got["T"][:4]) - 1.0) < 1e-15
        if kind == "analytic":  # (nothing about the truth on a fused layer: its minimiser sits half a voxel away)
            assert et < 0.1 * voxel and er < 0.05
        again = tr.refine(T0, pts)
        assert _same_bits(got["T"], again["T"]) and got["iterations"] == again["iterations"] and got["last_cost"] == again["last_cost"]
        ends.append((got["T"], bt, br))
    dt, dr = pose_diff(ends[0][0], ends[1][0])
    assert dt <= max(ends[0][1], ends[1][1]) and dr <= max(ends[0][2], ends[1][2])


def test_refine_dev_and_host_points_agree(hip, layers):
    import torch
    layer, _ = layers[("analytic", 0.10)]
    T, pts = scan()
    tr = Tracker(hip, layer, dof=6, stride=5, huber_delta=0.05, max_abs_distance=0.25)
    T0 = R.start_pose(T, 0.10, 6, 1.0, 2.0)
    host = tr.refine(T0, pts)
    dev_pts = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    dev = tr.refine_dev(T0, dev_pts)
    assert host["status_name"] == "converged" and _same_bits(host["T"], dev["T"]) and host["iterations"] == dev["iterations"]
    short = Tracker(hip, layer, dof=6, stride=5, max_iterations=2).refine(T0, pts)
    assert short["status_name"] == "max_iterations" and short["iterations"] == 2
    none = Tracker(hip, layer, max_iterations=0).refine(T0, pts)
    assert none["status_name"] == "max_iterations" and none["iterations"] == 0 and np.array_equal(none["T_refined"], T0)


def test_refine_host_points_small_large_small_on_one_tracker(hip, layers):
    """cox_track_refine keeps one staging buffer that grows with the scan and never shrinks: 64, 4096 and 64 points through one
    tracker.  One iteration each (nothing near a stop decision): the counts and the cost of the reference, and bit for bit the
    pose a fresh tracker gets from the same points on the device."""
    import torch
    layer, ref = layers[("analytic", 0.10)]
    T, pts = scan()
    T0 = R.start_pose(T, 0.10, 6, 1.0, 2.0)
    cfg = R.config(dof=6, max_iterations=1)
    tr = Tracker(hip, layer, dof=6, max_iterations=1)
    outs = []
    for p in (pts[::4801][:64], pts[::75][:4096], pts[::4801][:64]):  # spread over the image: all three walls, full rank
        got, exp = tr.refine(T0, p), ref.refine(T0, p, cfg)
        assert got["status"] == exp["status"] == R.MAX_ITERATIONS and got["iterations"] == exp["iterations"] == 1
        for key in ("first_n_used", "first_n_considered", "last_n_used", "last_n_considered"):
            assert got[key] == exp[key], key
        assert len(p) in (64, 4096) and exp["first_n_used"] >= 32 and abs(got["first_cost"] - exp["first_cost"]) <= len(p) * 2.0 ** -52 * exp["first_cost"]
        dev_pts = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        torch.cuda.synchronize()
        fresh = Tracker(hip, layer, dof=6, max_iterations=1).refine_dev(T0, dev_pts)
        assert _same_bits(got["T"], fresh["T"]) and got["first_cost"] == fresh["first_cost"]
        outs.append(got)
    assert _same_bits(outs[0]["T"], outs[2]["T"]) and not _same_bits(outs[0]["T"], outs[1]["T"])


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_lost_and_degenerate(hip, layers):
    T, pts = scan()
    T0 = R.start_pose(T, 0.10, 4, 0.5, 1.0)
    empty = Layer(hip, 0.10, capacity_blocks=64)
    out = Tracker(hip, empty, stride=STRIDE).refine(T0, pts)
    assert out["status_name"] == "lost" and out["iterations"] == 1 and out["last_n_used"] == 0 and out["last_n_considered"] == len(pts[::STRIDE])
    assert np.array_equal(out["T_refined"], T0) and np.array_equal(out["T"], T0.astype(np.float64))
    layer, _ = layers[("analytic", 0.10)]
    tr = Tracker(hip, layer)
    out = tr.refine(T0, np.zeros((0, 3), np.float32))  # n = 0
    assert out["status_name"] == "lost" and out["last_n_considered"] == 0 and np.array_equal(out["T_refined"], T0)
    out = tr.refine(T0, np.full((1000, 3), np.nan, np.float32))
    assert out["status_name"] == "lost" and out["last_n_considered"] == 0 and np.array_equal(out["T_refined"], T0)
    far = np.array(T0)
    far[4:] += np.float32(50.0)
    out = Tracker(hip, layer, stride=STRIDE).refine(far, pts)
    assert out["status_name"] == "lost" and out["last_n_used"] == 0 and np.array_equal(out["T_refined"], far)
    out = Tracker(hip, layer, stride=STRIDE, min_points=0, min_inlier_ratio=0.0).refine(far, pts)  # H = 0: no positive pivot
    assert out["status_name"] == "degenerate" and out["iterations"] == 1 and np.array_equal(out["T_refined"], far)
    # a tracker is fine after those
    ok = Tracker(hip, layer, stride=STRIDE)
    assert ok.refine(T0, pts)["status_name"] == "converged"


def test_a_layer_grown_between_two_calls(hip, layers):
    src, _ = layers[("analytic", 0.10)]
    idx, vox = src.download()
    grown = Layer(hip, 0.10, capacity_blocks=len(idx) + 8)
    grown.upload(idx, vox)
    T, pts = scan()
    T0 = R.start_pose(T, 0.10, 6, 1.0, 2.0)
    tr = Tracker(hip, grown, dof=6, stride=STRIDE)
    before = tr.refine(T0, pts)
    grown.reserve(4 * len(idx) + 64)
    after = tr.refine(T0, pts)
    assert before["status_name"] == "converged" and _same_bits(before["T"], after["T"]) and before["iterations"] == after["iterations"]


def test_refine_sees_the_frames_enqueued_before_it(hip):
    voxel = 0.10
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, hip.default_config(**synth.integrator_overrides(voxel)), "merged")
    frames = []
    for t in range(80, 121, 10):
        Tf, p, rgba, _ = synth.make_frame(t)
        frames.append((Tf, np.ascontiguousarray(p[::2]), np.ascontiguousarray(rgba[::2])))
    T, pts = scan()
    T0 = R.start_pose(T, voxel, 4, 0.7, 1.5, -1)
    tr = Tracker(hip, layer, stride=STRIDE)
    for Tf, p, rgba in frames:
        integ.integrate_points_async(Tf, p.ctypes.data, rgba.ctypes.data, len(p))
    early = tr.refine(T0, pts)  # no sync in between
    integ.sync()
    late = tr.refine(T0, pts)
    assert _same_bits(early["T"], late["T"]) and early["iterations"] == late["iterations"] and early["last_cost"] == late["last_cost"]
    assert late["last_n_used"] > 0.5 * late["last_n_considered"] and late["status_name"] in ("converged", "max_iterations")


def test_depth_entry_equals_the_point_entry(hip, layers):
    import torch
    layer, ref = layers[("analytic", 0.10)]
    T = synth.camera_pose(FRAME)[2]
    depth = torch.zeros((480, 640), dtype=torch.float32, device="cuda")
    layer.render_dev(T, 640, 480, depth=depth)
    torch.cuda.synchronize()
    image = depth.cpu().numpy()
    assert np.isfinite(image).all() and (image > 0).all()  # every ray meets a wall of the analytic room
    pts = torch.from_numpy(synth.depth_to_points(image)).cuda()
    torch.cuda.synchronize()
    T0 = R.start_pose(T, 0.10, 6, 1.0, 2.0)
    for cfg in (dict(dof=6), dict(dof=4, stride=7, huber_delta=0.05)):  # stride 1: 307 200 candidates, five passes of the grid
        tr = Tracker(hip, layer, **cfg)
        a, b = tr.refine_depth_dev(T0, depth, 640, 480), tr.refine_dev(T0, pts)
        assert a["status_name"] == "converged" and _same_bits(a["T"], b["T"]) and a["iterations"] == b["iterations"]
        assert a["last_cost"] == b["last_cost"] and a["last_n_used"] == b["last_n_used"] and a["last_n_considered"] == -(-640 * 480 // cfg.get("stride", 1))
    # a 2 % NaN mask: the masked pixels are not considered; counts exact, sums within the bound
    _, _, _, masked = synth.make_frame(FRAME, nan_fraction=0.02)
    masked = masked.copy()
    masked[5, 7], masked[100, 100] = 0.0, -1.0  # not positive: not considered either
    dm = torch.from_numpy(masked).cuda()
    torch.cuda.synchronize()
    tr = Tracker(hip, layer, dof=6, stride=7)
    got = tr.normal_eq_depth_dev(T0, dm, 640, 480)
    as_points = synth.depth_to_points(np.where(masked > 0, masked, np.nan).astype(np.float32))
    exp = ref.normal_eq(T0, as_points, R.config(dof=6, stride=7))
    valid = np.isfinite(masked.reshape(-1)[::7]) & (masked.reshape(-1)[::7] > 0)
    assert exp["n_considered"] == int(valid.sum()) < len(valid)
    _check_normal_eq(got, exp, 640 * 480, "masked depth image")


def test_invalid_arguments(hip, layers):
    layer, _ = layers[("analytic", 0.10)]
    for cfg in (dict(dof=5), dict(dof=0), dict(stride=0), dict(translation_tolerance=-1e-4), dict(rotation_tolerance=-1.0), dict(damping=-1.0),
                dict(huber_delta=float("nan")), dict(max_abs_distance=-0.1), dict(min_inlier_ratio=float("nan"))):
        with pytest.raises(CoxError) as e:
            Tracker(hip, layer, **cfg)
        assert e.value.status == -1, cfg
    tr = Tracker(hip, layer)
    f = hip.fn
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    T, K = np.array(synth.camera_pose(0)[2], np.float32), np.array([100, 100, 8, 8], np.float32)
    pts = np.zeros((4, 3), np.float32)
    bad = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(np.float32)  # noqa: E731
    assert f("track_refine")(tr.h, p(T), p(pts), C.c_uint64(4), None, None) == 0
    assert f("track_refine")(tr.h, None, p(pts), C.c_uint64(4), None, None) == -1
    assert f("track_refine")(tr.h, p(T), None, C.c_uint64(4), None, None) == -1
    assert f("track_refine")(tr.h, p(T), p(pts), C.c_uint64(1 << 31), None, None) == -1
    assert f("track_refine")(tr.h, p(bad(T, 5, np.nan)), p(pts), C.c_uint64(4), None, None) == -1
    assert f("track_refine")(tr.h, p(np.zeros(7, np.float32)), p(pts), C.c_uint64(4), None, None) == -1  # a zero quaternion
    assert f("track_refine_dev")(tr.h, p(T), None, C.c_uint64(4), None, None) == -1
    assert f("track_evaluate_dev")(tr.h, p(T), None, C.c_uint64(4), None, None) == -1
    assert f("track_normal_eq_dev")(tr.h, p(bad(T, 0, np.inf)), None, C.c_uint64(0), None, None, None, None) == -1
    import torch
    d = torch.ones((16, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dp = C.c_void_p(d.data_ptr())
    assert f("track_refine_depth_dev")(tr.h, p(T), dp, C.c_int(16), C.c_int(16), p(K), None, None) == 0
    for kw in (dict(w=0), dict(h=-1), dict(w=65536, h=32768), dict(K=bad(K, 0, 0.0)), dict(K=bad(K, 1, 0.0)), dict(K=bad(K, 2, np.nan)), dict(K=None),
               dict(depth=None)):
        a = dict(depth=dp, w=16, h=16, K=K)
        a.update(kw)
        assert f("track_refine_depth_dev")(tr.h, p(T), a["depth"], C.c_int(a["w"]), C.c_int(a["h"]), p(a["K"]) if a["K"] is not None else None, None, None) == -1, kw


def test_cpp_scan_to_map_registerer_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "track_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "track_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
