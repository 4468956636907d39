"""Committed fixture of the projective integrator (tests/golden/projective_golden.npz, made by
`python tests/golden/make_golden.py projective`).

Like oracle_golden.npz it is NOT a reference output: it freezes this repository's oracle, so that oracle and kernels
drifting together shows (CPU: the oracle still reproduces it; GPU: the HIP engine reproduces it with no oracle in the loop).
Per case: sha256 of the serialised layer, the per-frame counters, 64 sampled voxel words."""
import hashlib
import os

import numpy as np
import pytest

from coxgraph_amd import synth
from coxgraph_amd.capi import Layer, Integrator
from test_oracle_projective import lidar_cloud, proj_config, IDENT

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projective_golden.npz")
COUNTERS = ("n_points", "n_valid", "n_rays", "n_updates", "n_touched_voxels", "n_touched_blocks", "n_new_blocks")
CASES = ("lidar_wall_adaptive", "depth_stream_1280x960_invr2", "deintegration")
POSE = np.array([0.9990482, 0, 0, 0.0436194, 0.2, -0.1, 0.05], np.float32)


def case_frames(name):
    """-> (voxel, config overrides, [(T_G_C, points, deintegrate)])"""
    if name == "lidar_wall_adaptive":
        return 0.1, dict(projective_interpolation_scheme=3), [(IDENT, lidar_cloud(), False), (POSE, lidar_cloud(wall_x=2.8), False)]
    ov = synth.integrator_overrides(0.1)
    cam = dict(sensor_horizontal_resolution=1280, sensor_vertical_resolution=960, sensor_vertical_field_of_view_degrees=360.0,
               default_truncation_distance=ov["default_truncation_distance"], min_ray_length_m=ov["min_ray_length_m"], max_ray_length_m=ov["max_ray_length_m"])
    stream = [(T, np.ascontiguousarray(p[::4]), False) for T, p in (synth.make_frame(t)[:2] for t in (0, 10, 20))]
    if name == "depth_stream_1280x960_invr2":
        return 0.1, dict(cam, use_const_weight=0), stream
    return 0.1, dict(cam), stream + [(stream[0][0], stream[0][1], True)]  # frame 0 taken out again


def run_case(eng, name):
    voxel, kw, frames = case_frames(name)
    layer = Layer(eng, voxel, capacity_blocks=4096)
    integ = Integrator(eng, layer, proj_config(eng, **kw), "projective")
    stats = []
    for T, p, de in frames:
        if de:
            integ.deintegrate_points(T, p)
        else:
            integ.integrate_points(T, p, None)
        s = integ.last_stats()
        stats.append([s[k] for k in COUNTERS])
    idx, vox = layer.download()
    return idx, vox, np.array(stats, np.int64)


def sha(idx, vox):
    return np.frombuffer(hashlib.sha256(idx.tobytes() + vox.tobytes()).digest(), np.uint8)


def build_golden(eng):
    g = {}
    for name in CASES:
        idx, vox, stats = run_case(eng, name)
        nz = np.argwhere(vox[..., 1] != 0)
        assert len(nz) >= 1000, (name, len(nz))
        pick = nz[np.linspace(0, len(nz) - 1, 64).astype(np.int64)]
        g[f"{name}_sha256"], g[f"{name}_stats"] = sha(idx, vox), stats
        g[f"{name}_n_blocks_observed"] = np.array([len(idx), len(nz)], np.int64)
        g[f"{name}_sample_block"] = idx[pick[:, 0]]
        g[f"{name}_sample_voxel"] = pick[:, 1].astype(np.int32)
        g[f"{name}_sample_words"] = vox[pick[:, 0], pick[:, 1]]
    return g


def check(eng, name):
    G = np.load(PATH, allow_pickle=False)
    idx, vox, stats = run_case(eng, name)
    assert np.array_equal(stats, G[f"{name}_stats"]), (stats.tolist(), G[f"{name}_stats"].tolist())
    assert [len(idx), int((vox[..., 1] != 0).sum())] == G[f"{name}_n_blocks_observed"].tolist()
    row = {tuple(b): i for i, b in enumerate(idx.tolist())}
    rows = np.array([row[tuple(b)] for b in G[f"{name}_sample_block"].tolist()])
    assert np.array_equal(vox[rows, G[f"{name}_sample_voxel"]], G[f"{name}_sample_words"])
    assert np.array_equal(sha(idx, vox), G[f"{name}_sha256"])


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_golden_projective(oracle, name):
    check(oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_reproduces_golden_projective(hip, name):
    """Bit-identical layer (sha256 of block indices and voxel words) and counters, without the oracle in the loop."""
    check(hip, name)
