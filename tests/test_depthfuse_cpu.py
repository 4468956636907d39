"""The two references of the pinhole depth integrator against each other and against closed forms (no GPU).  DESIGN.md section 7m."""
import numpy as np
import pytest

import depthfuse_ref as dr
from render_ref import voxel_centres
from util import TOL


@pytest.fixture(scope="module")
def ref32(tmp_path_factory):
    return dr.build(tmp_path_factory.mktemp("depthfuse_ref"))


@pytest.fixture(scope="module")
def frames():
    return dr.scene_frames(3)


@pytest.mark.parametrize("case", dr.matrix_cases(), ids=dr.case_id)
def test_float32_reference_agrees_with_float64(ref32, frames, case):
    cfg = dr.case_config(case)
    a, b = ref32.layer(dr.VOXEL, **cfg), dr.Ref64(dr.VOXEL, **cfg)
    for T, depth, rgba, K in frames:
        rc, _ = a.integrate(T, depth, rgba if case["colour"] else None, K)
        assert rc == 0
        b.integrate(T, depth, rgba if case["colour"] else None, K)
    idx, vox = a.download()
    rep = b.check(idx, vox, TOL)
    print(rep)
    assert rep["checked"] > 1000 and rep["blocks"] >= 8  # (not an empty comparison)
    assert rep["ambiguous_fraction"] <= dr.MAX_AMBIGUOUS_FRACTION


# ---- a fronto-parallel wall at z = Z0: D = Z0 everywhere, so sdf = (Z0 - z) |q| / z in closed form ---------------------------------
Z0 = 2.0
T_AXIS = np.array([1, 0, 0, 0, 0.05, 0.05, 0.0], np.float32)  # camera axes = world axes, on a line of voxel centres


def wall_layer(ref32, n_frames=1, rgba=None, **cfg):
    lay = ref32.layer(dr.VOXEL, **{**dr.BASE, **cfg})
    depth = np.full((dr.H, dr.W), Z0, np.float32)
    for _ in range(n_frames):
        rc, st = lay.integrate(T_AXIS, depth, rgba)
        assert rc == 0
    idx, vox = lay.download()
    c = voxel_centres(idx, dr.VOXEL).astype(np.float64) - T_AXIS[4:].astype(np.float64)  # camera frame
    d = vox[..., 0].copy().view(np.float32).astype(np.float64)
    w = vox[..., 1].copy().view(np.float32).astype(np.float64)
    return c, d, w, vox[..., 2], st


def test_wall_axis_voxels_hold_the_distance_to_the_wall(ref32):
    c, d, w, _, _ = wall_layer(ref32, use_const_weight=1, use_weight_dropoff=0)
    axis = (np.abs(c[..., 0]) < 1e-6) & (np.abs(c[..., 1]) < 1e-6) & (c[..., 2] >= 0.3) & (c[..., 2] <= Z0 + 0.3)
    assert axis.sum() >= 20
    assert np.all(w[axis] > 0)
    assert np.max(np.abs(d[axis] - np.clip(Z0 - c[..., 2][axis], -0.3, 0.3))) <= TOL


def test_wall_nothing_behind_the_truncation_is_observed(ref32):
    c, d, w, _, _ = wall_layer(ref32)
    assert (w > 0).sum() > 1000
    assert not np.any(w[c[..., 2] > Z0 + 0.3 + 1e-6] > 0)
    # every observed voxel holds the closed form
    q = np.linalg.norm(c, axis=-1)
    obs = w > 0
    want = np.clip((Z0 - c[..., 2]) * q / c[..., 2], -0.3, 0.3)
    assert np.max(np.abs(d[obs] - want[obs])) <= TOL


def test_wall_without_carving_only_the_truncation_band_is_observed(ref32):
    c, d, w, _, _ = wall_layer(ref32, voxel_carving_enabled=0)
    obs = w > 0
    assert obs.sum() > 500
    sdf = (Z0 - c[..., 2]) * np.linalg.norm(c, axis=-1) / c[..., 2]
    assert np.all(sdf[obs] <= 0.3 + 1e-6) and np.all(sdf[obs] >= -0.3 - 1e-6)
    assert np.all(c[..., 2][obs] >= Z0 - 0.3 - 1e-6)


@pytest.mark.parametrize("n", [1, 3])
def test_wall_weights_count_the_frames(ref32, n):
    _, _, w, _, _ = wall_layer(ref32, n_frames=n, use_const_weight=1, use_weight_dropoff=0)
    assert np.max(np.abs(w[w > 0] - n)) <= TOL
    _, _, w, _, _ = wall_layer(ref32, n_frames=n, use_const_weight=0, use_weight_dropoff=0)
    assert np.max(np.abs(w[w > 0] - n / Z0 ** 2)) <= TOL


def test_wall_colours_follow_the_image_halves(ref32):
    rgba = np.zeros((dr.H, dr.W, 4), np.uint8)
    rgba[:, : dr.W // 2] = (255, 0, 0, 255)
    rgba[:, dr.W // 2:] = (0, 0, 255, 255)
    c, d, w, col, st = wall_layer(ref32, rgba=rgba, use_const_weight=1, use_weight_dropoff=0)
    K = dr.scaled_intrinsics(dr.W, dr.H).astype(np.float64)
    u = K[0] * c[..., 0] / c[..., 2] + K[2]
    sdf = (Z0 - c[..., 2]) * np.linalg.norm(c, axis=-1) / c[..., 2]
    obs = w > 0
    inside = obs & (np.abs(sdf) < 0.3 - 1e-6)
    red = np.uint32(255 | (255 << 24))    # wire word a | b << 8 | g << 16 | r << 24
    blue = np.uint32(255 | (255 << 8))
    left, right = inside & (u < dr.W // 2 - 0.5 - 1e-3), inside & (u > dr.W // 2 - 0.5 + 1e-3)
    assert left.sum() > 100 and right.sum() > 100
    assert np.all(col[left] == red) and np.all(col[right] == blue)
    assert np.all(col[obs & (sdf > 0.3 + 1e-6)] == 0)  # carved free space takes no colour
    assert st["n_coloured_voxels"] == int((col != 0).sum())


# ---- the interpolation schemes at a step edge and next to a hole ----------------------------------------------------------------------
K_WIDE = np.array([12.0, 12.0, 23.5, 17.5], np.float32)  # a pixel is 8 cm wide at 1 m: several 0.1 m voxels project into one cell


def _project(idx):
    c = voxel_centres(idx, dr.VOXEL).astype(np.float64) - T_AXIS[4:].astype(np.float64)
    K = K_WIDE.astype(np.float64)
    return c, K[0] * c[..., 0] / c[..., 2] + K[2], K[1] * c[..., 1] / c[..., 2] + K[3]


def test_adaptive_scheme_takes_the_near_side_of_a_step_edge(ref32):
    edge = 20  # columns < edge see 1 m, the others 2 m: a gap of 1 m > adaptive_gap_m
    depth = np.full((dr.H, dr.W), 2.0, np.float32)
    depth[:, :edge] = 1.0
    got = {}
    for scheme in (2, 3):
        lay = ref32.layer(dr.VOXEL, **dict(dr.BASE, interpolation_scheme=scheme, use_const_weight=1, use_weight_dropoff=0))
        assert lay.integrate(T_AXIS, depth, K=K_WIDE)[0] == 0
        got[scheme] = lay.download()
    for scheme, (idx, vox) in got.items():
        c, u, v = _project(idx)
        du = u - (edge - 1)
        straddle = (du > 0.2) & (du < 0.8) & (v > 1) & (v < dr.H - 2) & (c[..., 2] > 0.8) & (c[..., 2] < 1.2)
        assert straddle.sum() >= 5
        D = np.ones_like(u) if scheme == 3 else 1.0 + du
        want = np.clip((D - c[..., 2]) * np.linalg.norm(c, axis=-1) / c[..., 2], -0.3, 0.3)
        d = vox[..., 0].copy().view(np.float32).astype(np.float64)
        w = vox[..., 1].copy().view(np.float32)
        assert np.all(w[straddle] > 0)
        assert np.max(np.abs(d[straddle] - want[straddle])) <= TOL


@pytest.mark.parametrize("scheme", [2, 3])
def test_an_invalid_pixel_in_the_cell_falls_back_to_the_nearest_pixel(ref32, scheme):
    hole = (10, 12)  # (u, v)
    depth = (1.5 + 0.01 * np.arange(dr.W, dtype=np.float64))[None, :].repeat(dr.H, 0).astype(np.float32)
    depth[hole[1], hole[0]] = np.nan
    lay = ref32.layer(dr.VOXEL, **dict(dr.BASE, interpolation_scheme=scheme, use_const_weight=1, use_weight_dropoff=0))
    assert lay.integrate(T_AXIS, depth, K=K_WIDE)[0] == 0
    idx, vox = lay.download()
    c, u, v = _project(idx)
    d = vox[..., 0].copy().view(np.float32).astype(np.float64)
    w = vox[..., 1].copy().view(np.float32)
    u0, v0 = np.floor(u), np.floor(v)
    in_cell = (u0 >= hole[0] - 1) & (u0 <= hole[0]) & (v0 >= hole[1] - 1) & (v0 <= hole[1])
    un, vn = np.floor(u + 0.5), np.floor(v + 0.5)
    fu, fv = np.abs(u - un), np.abs(v - vn)
    clear = (fu > 0.2) & (fu < 0.45) & (fv < 0.45) & (c[..., 2] > 1.45) & (c[..., 2] < 1.75)  # far from every border, where nearest and bilinear differ
    on_hole = (un == hole[0]) & (vn == hole[1])
    near_valid = in_cell & ~on_hole & clear
    assert near_valid.sum() >= 3
    want = np.clip(((1.5 + 0.01 * un) - c[..., 2]) * np.linalg.norm(c, axis=-1) / c[..., 2], -0.3, 0.3)
    assert np.all(w[near_valid] > 0)
    assert np.max(np.abs(d[near_valid] - want[near_valid])) <= TOL
    # ... which is not what bilinear interpolation gives there
    bil = np.clip(((1.5 + 0.01 * u) - c[..., 2]) * np.linalg.norm(c, axis=-1) / c[..., 2], -0.3, 0.3)
    assert np.min(np.abs(bil[near_valid] - want[near_valid])) > 10 * TOL
    # a voxel whose nearest pixel is the hole is not observed
    gone = in_cell & on_hole & (fu < 0.45) & (fv < 0.45) & (c[..., 2] > 0.3) & (c[..., 2] < 3.0)
    assert gone.sum() >= 3 and not np.any(w[gone] > 0)
