"""Committed fixture of finishSubmap() (tests/golden/submap_golden.npz, made by `python tests/golden/make_golden.py submap`).

Like the other fixtures it is NOT a reference output: it freezes this repository's oracle, so that the oracle and the kernels
drifting together shows (CPU: the oracle still reproduces it; GPU: the HIP engine reproduces it with no oracle in the loop).
Per case (at most 8 blocks): the input layer in full (block indices, distance and weight words; colours are zero), the sha256 of the
ESDF's words and 256 sampled voxels, the sha256 of the isosurface points, 32 of them and their three counts, the surface box
and 64 sampler draws."""
import hashlib
import os

import numpy as np
import pytest

from coxgraph_amd.capi import Layer, RegPoints, Registration

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "submap_golden.npz")
LIN = np.arange(4096)
LOC = np.stack([LIN % 16, (LIN // 16) % 16, LIN // 256], axis=1)
# name -> (voxel, block indices, seed, ESDF configuration, isosurface min_weight, proximity threshold)
CASES = {
    "box_blobs_5cm": (0.05, [[x, y, z] for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)], 1, dict(max_distance_m=2.0, min_distance_m=0.075), 1.0, 0.025),
    "corners_only_10cm": (0.1, [[-2, -2, -2], [-1, -1, -1], [0, 0, 0], [1, 1, 1], [1, -1, 1], [0, -2, 0]], 2,
                          dict(max_distance_m=4.0, min_distance_m=0.1, default_distance_m=2.0), 1e-4, 0.05),
    "gapped_salt_20cm": (0.2, [[3, 0, 0], [4, 0, 0], [6, 0, 0], [6, 1, 0], [6, 1, 1], [3, -1, 0]], 3,
                         dict(max_distance_m=0.5, min_distance_m=0.2, default_distance_m=1.0, min_weight=1.0), 1.0, 1e-3),
}


def _hash24(g, seed):
    """integer hash of the global voxel index -> [0, 2^24): no random generator whose stream could change"""
    h = (g[..., 0] * 73856093 + g[..., 1] * 19349663 + g[..., 2] * 83492791 + seed * 2654435761).astype(np.uint64)
    h = (h ^ (h >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9)
    return ((h ^ (h >> np.uint64(32))) & np.uint64(0xFFFFFF)).astype(np.int64)


def case_input(name):
    voxel, idx, seed, _, _, _ = CASES[name]
    idx = np.array(idx, np.int32)
    g = idx[:, None, :].astype(np.int64) * 16 + LOC[None]
    d = np.zeros(g.shape[:2])
    for k in range(3):   # three fixed waves, 11 .. 27 voxels long
        kv = np.array([np.cos(1.0 + seed + 2.1 * k), np.sin(0.5 + seed + 1.3 * k), np.cos(2.0 * seed + 0.7 * k)]) * (2 * np.pi / (11.0 + 8.0 * k))
        d += 2.0 * voxel * np.sin(g @ kv + seed + k)
    d = (np.round(np.clip(d, -3 * voxel, 3 * voxel) / voxel * 4096.0) / 4096.0 * voxel).astype(np.float32)   # (libm's last bit rounded away)
    h = _hash24(g, seed)
    w = np.choose(np.searchsorted([0.03, 0.10, 0.70], h / 2.0 ** 24, side="right"), np.array([0.5, 1.0, 3.0, 20.0], np.float32)).astype(np.float32)
    if "blobs" in name:
        w[np.linalg.norm(g - g[0, 1234], axis=2) < 6] = 0.0
    if "salt" in name:
        w[_hash24(g, seed + 100) < 0.02 * 2 ** 24] = 0.0
    vox = np.zeros(d.shape + (3,), np.uint32)
    vox[..., 0], vox[..., 1] = d.view(np.uint32), w.view(np.uint32)
    return voxel, idx, vox


def sha(*arrays):
    return np.frombuffer(hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).digest(), np.uint8)


def run_case(eng, name, idx, vox):
    voxel, _, _, esdf_cfg, min_w, thr = CASES[name]
    layer = Layer(eng, voxel, capacity_blocks=64)
    layer.upload(idx, vox)
    eidx, evox = layer.esdf(**esdf_cfg).download()
    pts = RegPoints.from_isosurface(eng, layer, min_weight=min_w, vertex_proximity_threshold=thr)
    p = pts.download()
    mn, mx, n = layer.surface_obb()
    g = Registration(eng, pts, layer)
    g.draw_samples(64, 7)
    pick = np.linspace(0, evox[..., 0].size - 1, 256).astype(np.int64)
    return dict(input_sha256=sha(idx, vox), esdf_sha256=sha(eidx, evox), esdf_sample_words=evox.reshape(-1, 3)[pick],
                iso_sha256=sha(p), iso_sample_points=p[np.linspace(0, len(p) - 1, 32).astype(np.int64)],
                iso_counts=np.array([pts.n_mesh_vertices, pts.n_connected_vertices, pts.n], np.int64),
                box=np.concatenate([mn, mx]).astype(np.float32), box_count=np.array([n], np.int64), draws=g.get_samples())


def build_golden(eng):
    out = {}
    for name in CASES:
        _, idx, vox = case_input(name)
        r = run_case(eng, name, idx, vox)
        moved = len(np.unique(r["esdf_sample_words"][:, 0]))
        assert len(idx) <= 8 and r["iso_counts"][2] >= 100 and moved > 50, (name, r["iso_counts"], moved)
        out[f"{name}_idx"], out[f"{name}_distance_words"], out[f"{name}_weight_words"] = idx, vox[..., 0].copy(), vox[..., 1].copy()
        for k, v in r.items():
            out[f"{name}_{k}"] = v
    return out


def check(eng, name):
    """The inputs are read from the fixture (case_input() only serves make_golden.py), so libm and numpy play no part."""
    G = np.load(PATH, allow_pickle=False)
    idx = G[f"{name}_idx"]
    vox = np.zeros(G[f"{name}_distance_words"].shape + (3,), np.uint32)
    vox[..., 0], vox[..., 1] = G[f"{name}_distance_words"], G[f"{name}_weight_words"]
    r = run_case(eng, name, idx, vox)
    for k in ("input_sha256", "iso_counts", "box_count", "box", "draws", "esdf_sample_words", "iso_sample_points", "esdf_sha256", "iso_sha256"):
        v, want = r[k], G[f"{name}_{k}"]
        assert v.shape == want.shape and v.tobytes() == want.tobytes(), (name, k)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reproduces_golden_submap(oracle, name):
    check(oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_reproduces_golden_submap(hip, name):
    """Bit-identical ESDF, isosurface points, box and draws, without the oracle in the loop."""
    check(hip, name)
