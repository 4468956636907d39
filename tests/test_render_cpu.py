"""The renderer's C ABI (include/coxgraph_hip_render.h) and the test-side reference's known answers and physics -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_ref
from coxgraph_amd import synth
from render_ref import R_BUDGET, R_COLOR, R_HIT, R_NORMAL
from util import run_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return render_ref.build(tmp_path_factory.mktemp("renderref"))


def test_render_header_symbols_are_exported(hip):
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_render.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["cox_layer_render", "cox_layer_render_dev", "cox_render_config_default"]
    missing = [s for s in syms if not hasattr(hip.lib, s)]
    assert not missing, missing


def test_render_defaults_and_clean_failure(hip):
    """The defaults of the issue; without a GPU every call reports COX_ERR_NO_DEVICE, with one a NULL layer is COX_ERR_INVALID_ARG."""
    from coxgraph_amd.capi import RenderConfig
    c = RenderConfig()
    hip.fn("render_config_default", None)(C.byref(c))
    assert (c.step_scale, c.min_step_voxels, c.min_depth, c.max_depth, c.max_samples) == (0.75, 0.25, np.float32(0.1), 10.0, 4096)
    T = (C.c_float * 7)(1, 0, 0, 0, 0, 0, 0)
    K = (C.c_float * 4)(100, 100, 4, 4)
    d = (C.c_float * 64)()
    want = -2 if hip.device_count() == 0 else -1
    assert hip.fn("layer_render")(None, T, C.c_int(8), C.c_int(8), K, None, d, None, None, None, None) == want
    assert hip.fn("layer_render_dev")(None, T, C.c_int(8), C.c_int(8), K, None, d, None, None, None, None) == want


# ---- hand-derived known answers ------------------------------------------------------------------------------------------------
# Layer: one block of 0.125 m voxels (edge 2 m) with d = 1.5 - z at every voxel centre.  Camera at (1.0625, 1.0625, 0) with the
# world's axes, central pixel (4, 4) of a 9 x 9 image: the ray is p(t) = (1.0625, 1.0625, t) and len = 1.  x and y sit on a
# voxel centre, so the trilinear value is the linear interpolation of 1.5 - zc along z: exactly 1.5 - t.
def test_known_answer_of_the_central_ray(ref):
    idx, words = render_ref.plane_layer_arrays()
    L = ref.layer(render_ref.PLANE_VS, idx, words)
    out = L.render(render_ref.PLANE_T, 9, 9, render_ref.PLANE_K, min_depth=0.25)
    # step = max(0.75 |d|, 0.25 * 0.125 = 0.03125):
    #   t = 0.25        d = 1.25         step 0.9375
    #   t = 1.1875      d = 0.3125       step 0.234375
    #   t = 1.421875    d = 0.078125     step 0.05859375
    #   t = 1.48046875  d = 0.01953125   step max(0.0146484375, 0.03125) = 0.03125
    #   t = 1.51171875  d = -0.01171875  hit: t* = 1.48046875 + 0.03125 * 0.01953125 / (0.01953125 + 0.01171875) = 1.5
    assert out["samples"][4, 4] == 5
    assert out["depth"][4, 4] == np.float32(1.5)
    # gradient at (1.0625, 1.0625, 1.5), h = 0.125: x and y samples are all 0; z: (-(0.125) + (-0.125)) / 0.25 = -1: towards the camera
    assert out["normal"][4, 4].tolist() == [0.0, 0.0, -1.0]
    assert out["rgba"][4, 4].tolist() == [10, 20, 30, 255]
    assert out["status"][4, 4] == R_HIT | R_NORMAL | R_COLOR
    # the whole image sees the plane: z-depth 1.5 for every pixel, whatever its ray's length
    assert np.all(out["status"] & R_HIT) and np.max(np.abs(out["depth"] - 1.5)) < 1e-6
    assert out["stats"]["n_hits"] == 81 and out["stats"]["n_budget"] == 0 and out["stats"]["n_block_skips"] == 0
    assert out["stats"]["n_samples"] == int(out["samples"].sum())


def test_known_answer_of_a_ray_through_unallocated_blocks(ref):
    idx, words = render_ref.plane_layer_arrays()
    L = ref.layer(render_ref.PLANE_VS, idx, words)
    # half a turn about x: the camera at (1.0625, 1.0625, -0.5) looks along -z, below the only block
    T = np.array([0, 1, 0, 0, 1.0625, 1.0625, -0.5], np.float32)
    out = L.render(T, 9, 9, render_ref.PLANE_K, min_depth=0.25)
    # central ray p(t) = (., ., -0.5 - t): blocks z = -1 (z in [-2, 0)), -2, ...; exit of block b at t = -2 b - 0.5, plus half a
    # voxel 0.0625: samples at t = 0.25, 1.5625, 3.5625, 5.5625, 7.5625, 9.5625, then 11.5625 > max_depth
    assert out["samples"][4, 4] == 6
    assert np.all(out["status"] == 0) and np.isnan(out["depth"]).all() and np.isnan(out["normal"]).all() and not out["rgba"].any()
    assert out["stats"]["n_hits"] == 0 and out["stats"]["n_block_skips"] == out["stats"]["n_samples"]
    assert out["samples"].max() <= 8  # oblique rays may clip one more block in x or y


def test_a_ray_that_starts_behind_the_plane_reports_nothing(ref):
    idx, words = render_ref.plane_layer_arrays()
    L = ref.layer(render_ref.PLANE_VS, idx, words)
    out = L.render(render_ref.PLANE_T, 9, 9, render_ref.PLANE_K, min_depth=1.625)
    # central ray: t = 1.625 d = -0.125 step 0.09375; t = 1.71875 d = -0.21875 step 0.1640625; t = 1.8828125 d = -0.3828125 step
    # 0.287109375; t = 2.169921875 and on: unallocated blocks z = 1 .. 4 (exits 4, 6, 8, 10, plus 0.0625): samples at 2.169921875,
    # 4.0625, 6.0625, 8.0625, then 10.0625 > max_depth.  Never a positive sample: no hit.
    assert out["samples"][4, 4] == 7
    assert np.all(out["status"] == 0) and np.isnan(out["depth"]).all()


def test_a_crossing_over_an_unobserved_gap_is_not_a_hit(ref):
    idx, words = render_ref.plane_layer_arrays()
    z_index = np.arange(4096) >> 8
    gap = (z_index >= 9) & (z_index <= 12)  # centres 1.1875 .. 1.5625: the zero crossing lies inside the gap
    words[0, gap, 1] = 0
    L = ref.layer(render_ref.PLANE_VS, idx, words)
    out = L.render(render_ref.PLANE_T, 9, 9, render_ref.PLANE_K, min_depth=0.25)
    # central ray: t = 0.25 (d = 1.25, step 0.9375); t = 1.1875, 1.3125, 1.4375, 1.5625 unobserved (one voxel each, the positive
    # sample is forgotten); t = 1.6875 d = -0.1875 (first sample after the gap: remembered, not a hit), step 0.140625;
    # t = 1.828125 d = -0.328125, step 0.24609375; t = 2.07421875 and 4.0625, 6.0625, 8.0625: unallocated blocks
    assert out["samples"][4, 4] == 11
    assert out["status"][4, 4] == 0 and np.isnan(out["depth"][4, 4])
    assert out["stats"]["n_hits"] == 0
    # control: a gap in front of the crossing (centres 1.1875 and 1.3125) only delays the hit: t = 0.25; 1.1875 and 1.3125
    # unobserved; t = 1.4375 d = 0.0625 step max(0.046875, 0.03125); t = 1.484375 d = 0.015625 step 0.03125; t = 1.515625
    # d = -0.015625: t* = 1.484375 + 0.03125 * 0.015625 / 0.03125 = 1.5.  The gradient sample at z = 1.5 - 0.125 needs the unobserved
    # centre 1.3125: depth and colour without a normal
    words2 = render_ref.plane_layer_arrays()[1]
    words2[0, (z_index >= 9) & (z_index <= 10), 1] = 0
    out2 = ref.layer(render_ref.PLANE_VS, idx, words2).render(render_ref.PLANE_T, 9, 9, render_ref.PLANE_K, min_depth=0.25)
    assert out2["samples"][4, 4] == 6 and out2["depth"][4, 4] == np.float32(1.5) and out2["status"][4, 4] == R_HIT | R_COLOR
    assert np.isnan(out2["normal"][4, 4]).all() and out2["rgba"][4, 4].tolist() == [10, 20, 30, 255]


def test_budget_bit(ref):
    idx, words = render_ref.plane_layer_arrays()
    L = ref.layer(render_ref.PLANE_VS, idx, words)
    out = L.render(render_ref.PLANE_T, 9, 9, render_ref.PLANE_K, min_depth=0.25, max_samples=1)
    assert np.all(out["status"] == R_BUDGET) and np.isnan(out["depth"]).all() and out["stats"]["n_budget"] == 81
    out = L.render(render_ref.PLANE_T, 9, 9, render_ref.PLANE_K, min_depth=0.25, max_samples=4)
    assert out["status"][4, 4] == R_BUDGET  # the central ray needs 5
    out = L.render(render_ref.PLANE_T, 9, 9, render_ref.PLANE_K, min_depth=0.25, max_samples=5)
    assert out["status"][4, 4] == R_HIT | R_NORMAL | R_COLOR


# ---- physics: the fused map seen from a pose is the scene --------------------------------------------------------------------
# Measured with this reference on the oracle-fused submaps (frames 0 .. 140 step 10, every second point), 640 x 480, default
# configuration; thresholds are the worst measured value over the poses listed in PHYSICS_MEASURED plus 25 % for other seeds and
# poses (share: 25 % more of the missing part).
PHYSICS_MEASURED = {
    # voxel: {frame: (share of pixels hit, median, 95th percentile of |depth - analytic| in voxels)}
    0.10: {70: (0.9997, 0.0269, 1.7250), 75: (0.9995, 0.0238, 1.6370)},
    0.05: {70: (0.9995, 0.0153, 0.6485), 75: (0.9994, 0.0143, 0.6313)},
}
PHYSICS_BOUNDS = {
    # voxel: (min share, max median, max p95): 1 - 1.25 (1 - worst share), 1.25 worst median, 1.25 worst p95
    0.10: (0.9993, 0.0336, 2.156),
    0.05: (0.9992, 0.0191, 0.811),
}


@pytest.fixture(scope="module", params=[0.10, 0.05])
def fused(request, oracle, ref):
    voxel = request.param
    layer, _, _ = run_frames(oracle, method="merged", voxel=voxel, frames=range(0, 150, 10), subsample=2, capacity_blocks=8192)
    idx, vox = layer.download()
    return voxel, ref.layer(voxel, idx, vox)


@pytest.mark.parametrize("frame", [70, 75])
def test_rendered_depth_of_the_fused_map_is_the_analytic_depth(fused, frame):
    """A fused pose (frame 70) and one between two fused poses (75): pixel -> ray -> layer -> depth against synth.render_depth."""
    voxel, L = fused
    R, origin, T = synth.camera_pose(frame)
    out = L.render(T, 640, 480)
    share, med, p95 = render_ref.error_in_voxels(out["depth"], synth.render_depth(R, origin), voxel)
    print(f"voxel {voxel} frame {frame}: hit {share:.4f}, |depth - analytic| median {med:.4f} p95 {p95:.4f} voxels, "
          f"{out['stats']['n_samples'] / (640 * 480):.1f} samples per ray, {out['stats']['seconds']:.1f} s")
    lo_share, hi_med, hi_p95 = PHYSICS_BOUNDS[voxel]
    assert share >= lo_share and med <= hi_med and p95 <= hi_p95
    assert out["stats"]["n_budget"] == 0


# ---- exact field: an analytic sphere sampled into a layer ----------------------------------------------------------------------
def test_sphere_depth_and_normal_within_the_interpolation_error(ref):
    """d = |x - c| - r at every voxel centre, no fusion error.  What remains is the trilinear interpolant's error: for a field f
    with second derivatives f_ii it is at most (h^2 / 8) sum |f_ii|; for the distance to a point sum f_ii = 2 / rho, so near the
    surface e_f <= h^2 / (4 (r - h)).  The renderer's hit is a root of the interpolant F (the last step is the minimum step
    h / 4 because a step of 0.75 |d| cannot cross a surface d away; the linear interpolation over it adds (h / 4)^2 / 8 times
    F's second derivative along the ray, below e_f / 16), so |f(p*)| <= e_f (1 + 1/16) and the distance along the ray is off by
    that over cos(incidence).  The normal: central differences of F with step h differ from grad f by at most
    2 e_f / (2 h) + (h^2 / 6) |f'''| <= e_f / h + h^2 / (2 (r - h)^2) per component, sqrt(3) times that in angle (|grad f| = 1),
    plus the angle between the radial directions at p* and at the true hit, depth error / r."""
    vs, c, r = 0.05, np.array([0.8 + 0.013, 0.8 - 0.021, 0.8 + 0.007]), 0.35
    idx, words = render_ref.sphere_layer_arrays(vs, c, r, trunc=5 * vs)
    L = ref.layer(vs, idx, words)
    K = np.array([200.0, 200.0, 79.5, 59.5], np.float32)
    e_f = vs * vs / (4 * (r - vs))
    for origin in ([0.8, -0.9, 0.8], [-0.7, 0.3, 1.3], [1.2, 1.4, -0.8]):
        Rm, o, T = render_ref.look_at_pose(origin, c)
        # the camera stands outside the layer: the first 0.3 m are unallocated, the rest is the truncated field
        out = L.render(T, 160, 120, K)
        u, v = np.meshgrid(np.arange(160, dtype=np.float64), np.arange(120, dtype=np.float64))
        dc = np.stack([(u - float(K[2])) / float(K[0]), (v - float(K[3])) / float(K[1]), np.ones_like(u)], -1)
        length = np.linalg.norm(dc, axis=-1)
        dirs = (dc @ Rm.T) / length[..., None]
        oc = o - c
        b = np.einsum("ijk,k->ij", dirs, oc)
        disc = b * b - (oc @ oc - r * r)
        with np.errstate(invalid="ignore"):
            s_true = -b - np.sqrt(disc)
            p_true = o + dirs * s_true[..., None]
            cos_inc = -np.einsum("ijk,ijk->ij", dirs, (p_true - c) / r)
        sel = (disc > 0) & (cos_inc >= 0.5)
        hit = (out["status"] & R_HIT) != 0
        assert sel.sum() > 1000 and hit[sel].all()
        err = np.abs(out["depth"].astype(np.float64) * length - s_true)[sel]
        bound_d = e_f * (1 + 1 / 16) / cos_inc[sel] + 1e-5
        print(f"sphere from {origin}: {sel.sum()} rays, depth error max {err.max():.5f} m (bound at that ray {bound_d[err.argmax()]:.5f}), e_f {e_f:.5f}")
        assert np.all(err <= bound_d)
        assert np.all((out["status"][sel] & R_NORMAL) != 0)
        n = out["normal"][sel].astype(np.float64)
        assert np.max(np.abs(np.linalg.norm(n, axis=1) - 1)) < 1e-5
        radial = (p_true - c)[sel] / r
        ang = np.arccos(np.clip(np.einsum("ij,ij->i", n, radial), -1, 1))
        bound_a = np.sqrt(3) * (e_f / vs + vs * vs / (2 * (r - vs) ** 2)) + bound_d / r
        print(f"  normal angle max {np.degrees(ang.max()):.2f} deg (bound {np.degrees(bound_a.max()):.2f})")
        assert np.all(ang <= bound_a)
