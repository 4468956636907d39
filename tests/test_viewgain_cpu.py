"""The view-gain C ABI (include/coxgraph_hip_gain.h) and the test-side reference's hand-counted answers -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_ref
import viewgain_ref
from viewgain_ref import COUNTS, FREE, FRONTIER, OCCUPIED, UNKNOWN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return viewgain_ref.build(tmp_path_factory.mktemp("viewgainref"))


def test_gain_header_symbols_are_exported(hip):
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_gain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["cox_viewgain_config_default", "cox_viewgain_create", "cox_viewgain_destroy", "cox_viewgain_evaluate", "cox_viewgain_evaluate_dev",
                    "cox_viewgain_view_bytes", "cox_viewgain_visible"]
    missing = [s for s in syms if not hasattr(hip.lib, s)]
    assert not missing, missing


def test_gain_defaults_and_clean_failure(hip):
    """The defaults of reconstruction_planner.yaml; without a GPU every call reports COX_ERR_NO_DEVICE before it looks at its
    arguments, with one a NULL layer / handle is COX_ERR_INVALID_ARG."""
    from coxgraph_amd.capi import ViewGainConfig, ViewGainRecord, viewgain_config
    c = viewgain_config(hip)
    f32 = np.float32
    assert (c.w, c.h, list(c.K)) == (35, 96, [64.0, 64.0, 17.0, 48.0])
    assert (c.frontier_voxel_weight, c.new_voxel_weight, c.min_impact_factor) == (1.0, 0.0, f32(0.01))
    assert (c.ray_angle_x, c.ray_angle_y, c.ray_length, c.min_range, c.ray_step) == (f32(0.002454), f32(0.002681), 5.0, 0.0, 0.0)
    assert (c.accurate_frontiers, c.surface_frontiers, c.use_box, c.min_weight, c.surface_distance, c.workspace_bytes) == (1, 1, 0, 0.0, 0.0, 0)
    assert C.sizeof(ViewGainConfig) == C.sizeof(viewgain_ref.Config) and C.sizeof(ViewGainRecord) == 48
    want = -2 if hip.device_count() == 0 else -1
    h = C.c_void_p()
    T = (C.c_float * 7)(1, 0, 0, 0, 0, 0, 0)
    rec = ViewGainRecord()
    n = C.c_uint64()
    assert hip.fn("viewgain_create")(None, None, C.byref(h)) == want
    assert hip.fn("viewgain_evaluate")(None, T, C.c_uint64(1), C.byref(rec), None) == want
    assert hip.fn("viewgain_evaluate_dev")(None, None, C.c_uint64(1), None, None) == want
    assert hip.fn("viewgain_visible")(None, T, C.c_uint64(0), None, None, None, C.byref(n)) == want
    assert hip.fn("viewgain_view_bytes", C.c_uint64)(None) == 0
    hip.fn("viewgain_destroy", None)(None)


# ---- hand-counted answers ------------------------------------------------------------------------------------------------------
# Layer: one block of 0.125 m voxels (edge 2 m), d = 1.5 - z at every voxel centre, weight 1.  Voxel z index k has its centre at
# (k + 0.5) / 8: d > 0 for k <= 11 (free), d = -0.0625 for k = 12 (occupied): a wall at z index 12.  The camera has the world's
# axes (it looks along +z) and stands at (1.0625, 1.0625, 0), the centre line of voxel column (8, 8).  ray_step = 0: 0.125.
VS = 0.125
ORIGIN = (1.0625, 1.0625, 0.0)
K1 = (64.0, 64.0, 0.0, 0.0)  # 1 x 1 grid: the one ray is the optical axis
K3 = (16.0, 16.0, 1.0, 1.0)  # 3 x 3 grid: neighbouring rays 1/16 apart at unit depth


def wall_arrays(hole=False, unobserved_from=16):
    idx, words = render_ref.field_layer_arrays(VS, [(0, 0, 0)], lambda c: 1.5 - c[:, 2])
    lin = np.arange(4096)
    x, y, z = lin & 15, (lin >> 4) & 15, lin >> 8
    words[0, z >= unobserved_from, 1] = 0
    if hole:
        words[0, (x == 8) & (y == 8) & (z == 12), 1] = 0
    return idx, words


def _one(out, i=0):
    return {k: int(out[k][i]) for k in COUNTS + ("n_samples",)}


def test_wall_head_on_through_one_ray(ref):
    L = ref.layer(VS, *wall_arrays())
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1)
    # samples at z = 0, 0.125, ...: z index k at sample k; k = 0 .. 11 free, k = 12 occupied and the ray ends
    assert _one(out) == dict(n_visible=13, n_free=12, n_occupied=1, n_surface_counted=1, n_unknown=0, n_frontier=0, n_samples=13)
    # the wall voxel's centre is 1.5625 m away: a = 2 atan2(0.125, 3.125), nw = a^2 / (rx ry) / 1.5625^2, weight 1
    a = 2 * np.arctan2(0.125, 3.125)
    nw = a * a / (np.float32(0.002454) * np.float32(0.002681)) / 1.5625 ** 2
    imp = nw / (nw + 1)
    assert abs(out["surface_gain"][0] - imp) < 1e-6 and out["gain"][0] == out["surface_gain"][0]
    assert out["surface_gain_q32"][0] == int(out["surface_gain"][0] * 2 ** 32) and out["n_borderline"][0] == 0
    vis = L.visible(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1)
    assert vis["voxel_xyz"].tolist() == [[8, 8, k] for k in range(13)]  # ascending (z, y, x)
    assert vis["cls"].tolist() == [FREE] * 12 + [OCCUPIED] and vis["value"][:12].tolist() == [0.0] * 12
    assert abs(vis["value"][12] - imp) < 1e-6


def test_wall_head_on_through_three_by_three_rays(ref):
    L = ref.layer(VS, *wall_arrays())
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=3, h=3, K=K3)
    # The centre ray: column (8, 8), z 0 .. 12 as above, 13 samples.  An edge ray (x = +-1/16, y = 0; or the other way round) has
    # n = sqrt(1 + 1/256) = 1.00195: sample k lies at depth 0.125 k / n (z index k - 1 for k >= 1) and 0.0077976 k m off the
    # centre line, so it leaves column 8 (half width 0.0625) between k = 8 (0.06238) and k = 9: z 0 .. 7 in column (8, 8), shared
    # with the centre ray, then z 8 .. 12 in its own column (9, 8): 5 new voxels, the last one occupied; 14 samples.  A corner ray
    # (n = sqrt(1 + 2/256) = 1.0039, 0.0077822 k m off on both axes) does the same into column (9, 9).
    assert _one(out) == dict(n_visible=13 + 4 * 5 + 4 * 5, n_free=12 + 8 * 4, n_occupied=9, n_surface_counted=9, n_unknown=0, n_frontier=0,
                             n_samples=13 + 8 * 14)
    vis = L.visible(viewgain_ref.at(ORIGIN), w=3, h=3, K=K3)
    occ = vis["voxel_xyz"][vis["cls"] == OCCUPIED]
    assert occ.tolist() == [[x, y, 12] for y in (7, 8, 9) for x in (7, 8, 9)]  # one per ray, in (z, y, x) order
    assert np.array_equal(np.unique(vis["voxel_xyz"], axis=0).shape, vis["voxel_xyz"].shape)  # each voxel once


def test_frontiers_behind_a_free_corridor(ref):
    # the slab z >= 12 unobserved, the wall with it: the ray runs through 12 free voxels, then 4 unobserved ones inside the block
    # and 24 in unallocated space (z index 16 .. 39: d = 4.875 is the last sample below ray_length 5)
    L = ref.layer(VS, *wall_arrays(unobserved_from=12))
    T = viewgain_ref.at(ORIGIN)
    want = dict(n_visible=40, n_free=12, n_occupied=0, n_surface_counted=0, n_unknown=28, n_frontier=0, n_samples=40)
    out = L.evaluate(T, w=1, h=1, K=K1)
    assert _one(out) == want and out["gain"][0] == 0.0  # nothing occupied anywhere: no surface frontier
    out = L.evaluate(T, w=1, h=1, K=K1, surface_frontiers=0)
    assert _one(out) == {**want, "n_frontier": 1} and out["gain"][0] == 1.0  # z index 12 touches the observed z index 11
    out = L.evaluate(T, w=1, h=1, K=K1, surface_frontiers=0, frontier_voxel_weight=2.5, new_voxel_weight=0.5)
    assert out["gain"][0] == 2.5 * 1 + 0.5 * 27
    out = L.evaluate(T, w=1, h=1, K=K1, surface_frontiers=0, frontier_voxel_weight=0.0, new_voxel_weight=1.0)
    assert _one(out) == want and out["gain"][0] == 28.0  # no voxel is classed a frontier
    vis = L.visible(T, w=1, h=1, K=K1, surface_frontiers=0)
    assert vis["cls"].tolist() == [FREE] * 12 + [FRONTIER] + [UNKNOWN] * 27 and vis["voxel_xyz"][-1].tolist() == [8, 8, 39]


def test_accurate_frontiers_on_a_voxel_with_only_a_diagonal_occupied_neighbour(ref):
    # the wall at z index 12 with a hole at (8, 8), nothing observed behind it: the ray passes through the hole.  (8, 8, 12) has
    # the wall voxels (7, 8, 12), (9, 8, 12), ... as face neighbours; (8, 8, 13) has the hole below it and reaches the wall only
    # over an edge, e.g. (7, 8, 12); (8, 8, 14) reaches nothing.
    L = ref.layer(VS, *wall_arrays(hole=True, unobserved_from=13))
    T = viewgain_ref.at(ORIGIN)
    want = dict(n_visible=40, n_free=12, n_occupied=0, n_surface_counted=0, n_unknown=28, n_frontier=2, n_samples=40)
    assert _one(L.evaluate(T, w=1, h=1, K=K1)) == want
    assert _one(L.evaluate(T, w=1, h=1, K=K1, accurate_frontiers=0)) == {**want, "n_frontier": 1}
    vis = L.visible(T, w=1, h=1, K=K1)
    assert vis["cls"][12:15].tolist() == [FRONTIER, FRONTIER, UNKNOWN] and vis["value"][12:15].tolist() == [1.0, 1.0, 0.0]


def test_an_empty_layer_is_all_unknown(ref):
    L = ref.layer(VS, np.zeros((0, 3), np.int32), np.zeros((0, 4096, 3), np.uint32))
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1)
    assert _one(out) == dict(n_visible=40, n_free=0, n_occupied=0, n_surface_counted=0, n_unknown=40, n_frontier=0, n_samples=40)
    # 3 x 3 rays: the distinct voxels of the samples o + (k / 8) dir, recomputed in float32
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=3, h=3, K=K3)
    f = np.float32
    seen = set()
    for v in range(3):
        for u in range(3):
            x, y = (f(u) - f(1)) / f(16), (f(v) - f(1)) / f(16)
            n = np.sqrt(x * x + y * y + f(1))
            dirs = (x / n, y / n, f(1) / n)  # the identity quaternion leaves the direction as it is
            for k in range(40):
                p = [f(o) + f(k) * f(VS) * d for o, d in zip(ORIGIN, dirs)]
                seen.add(tuple(int(np.floor(c * f(8) + f(1e-6))) for c in p))
    assert _one(out) == dict(n_visible=len(seen), n_free=0, n_occupied=0, n_surface_counted=0, n_unknown=len(seen), n_frontier=0, n_samples=360)
    assert out["gain"][0] == 0.0 and len(seen) > 40


def test_a_view_whose_first_sample_is_occupied(ref):
    L = ref.layer(VS, *wall_arrays())
    # the origin is the centre of the wall voxel (8, 8, 12): distance 0, the impact is NaN and does not count
    out = L.evaluate(viewgain_ref.at((1.0625, 1.0625, 1.5625)), w=3, h=3, K=K3)
    assert _one(out) == dict(n_visible=1, n_free=0, n_occupied=1, n_surface_counted=0, n_unknown=0, n_frontier=0, n_samples=9)
    assert out["gain"][0] == 0.0
    # a little below the centre the same voxel counts: nw = (2 atan2(0.125, 0.0625))^2 / (rx ry) / 0.03125^2 = 7.6e8, so the
    # impact nw / (nw + 1) is 1 to float precision
    out = L.evaluate(viewgain_ref.at((1.0625, 1.0625, 1.53125)), w=1, h=1, K=K1)
    assert _one(out)["n_surface_counted"] == 1 and 0.999999 < out["gain"][0] <= 1.0


def test_the_box_cuts_the_set_but_not_the_ray(ref):
    L = ref.layer(VS, *wall_arrays())
    # centres with 0.5 <= z <= 1.0: z index 4 .. 7 (0.5625 .. 0.9375); the ray still runs to the wall (13 samples)
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1, use_box=1, box_min=(0, 0, 0.5), box_max=(2, 2, 1.0))
    assert _one(out) == dict(n_visible=4, n_free=4, n_occupied=0, n_surface_counted=0, n_unknown=0, n_frontier=0, n_samples=13)
    vis = L.visible(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1, use_box=1, box_min=(0, 0, 0.5), box_max=(2, 2, 1.0))
    assert vis["voxel_xyz"].tolist() == [[8, 8, k] for k in (4, 5, 6, 7)]
    # a box that holds the wall voxel only
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1, use_box=1, box_min=(0, 0, 1.5), box_max=(2, 2, 1.6))
    assert _one(out) == dict(n_visible=1, n_free=0, n_occupied=1, n_surface_counted=1, n_unknown=0, n_frontier=0, n_samples=13)


def test_min_range_and_half_steps(ref):
    L = ref.layer(VS, *wall_arrays())
    # min_range 0.5: samples k = 4 .. 12
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1, min_range=0.5)
    assert _one(out) == dict(n_visible=9, n_free=8, n_occupied=1, n_surface_counted=1, n_unknown=0, n_frontier=0, n_samples=9)
    # half a voxel per step: every voxel sampled twice, the wall once (the ray ends on its first sample): the same set
    out = L.evaluate(viewgain_ref.at(ORIGIN), w=1, h=1, K=K1, ray_step=0.0625)
    assert _one(out) == dict(n_visible=13, n_free=12, n_occupied=1, n_surface_counted=1, n_unknown=0, n_frontier=0, n_samples=25)
