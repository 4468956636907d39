"""The projective integrator's CPU oracle (oracle/cox_oracle_projective.hpp) against the independent float64 reference of
tests/proj_ref.py: values, block sets and counters, on a matrix of small scenes.  The oracle and the HIP kernels were written
by one hand, statement by statement parallel; the reference is a separate restatement of the rules (numpy, float64, matrices),
so a misreading shared by oracle and kernel (rows / columns swapped, the altitude's sign, the wrong pose inverse ...) shows here.

What is compared, and what is not: proj_ref marks a voxel AMBIGUOUS when a discrete decision on the way to its value lies within
2^-18 (relative) of its threshold -- float32 may take it the other way.  Those are skipped; the test asserts that they are
few (<= 2 % of the updated voxels) and that >= 1000 compared voxels remain, in every case.
"""
import numpy as np
import pytest

import proj_ref
from coxgraph_amd.capi import Layer, Integrator, words_to_fields
from util import TOL

MAX_AMBIGUOUS_FRACTION = 0.02
MIN_COMPARED = 1000


def engine_kwargs(cfg, fov_deg):
    return dict(default_truncation_distance=cfg["truncation"], use_const_weight=int(cfg["const_weight"]), min_ray_length_m=cfg["min_ray"],
                max_ray_length_m=cfg["max_ray"], max_weight=cfg["max_weight"], voxel_carving_enabled=int(cfg["carving"]),
                use_weight_dropoff=int(cfg["dropoff"]), sensor_horizontal_resolution=cfg["cols"], sensor_vertical_resolution=cfg["rows"],
                sensor_vertical_field_of_view_degrees=float(fov_deg), projective_interpolation_scheme=cfg["scheme"],
                projective_adaptive_gap_m=cfg["adaptive_gap"])


def pose(yaw_deg, pitch_deg, roll_deg, t):
    """(qw, qx, qy, qz, tx, ty, tz) of Rz(yaw) Ry(pitch) Rx(roll)."""
    y, p, r = np.radians([yaw_deg, pitch_deg, roll_deg]) / 2.0
    qz, qy, qx = np.array([np.cos(y), 0, 0, np.sin(y)]), np.array([np.cos(p), 0, np.sin(p), 0]), np.array([np.cos(r), np.sin(r), 0, 0])

    def mul(a, b):
        return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])
    return np.concatenate([mul(mul(qz, qy), qx), t]).astype(np.float32)


def scan(T, rows, cols, fov_deg, scene, seed, step=1):
    """A range scan of a world scene from pose T: one return per pixel (every `step`-th), its bearing at the pixel's centre
    +- 0.3 pixel (so that no point sits on a pixel border), in the sensor frame.  scene: ("wall", x) the plane x = const, or
    ("sphere", centre, radius)."""
    rng = np.random.default_rng(seed)
    hh, ww = np.meshgrid(np.arange(0, rows - 1, step), np.arange(1, cols - 2, step), indexing="ij")
    h = hh.reshape(-1) + 0.5 + rng.uniform(-0.3, 0.3, hh.size)
    w = ww.reshape(-1) + 0.5 + rng.uniform(-0.3, 0.3, hh.size)
    alt = (0.5 - h / (rows - 1)) * np.radians(fov_deg)
    az = w / cols * 2.0 * np.pi
    keep = np.abs(alt) < np.radians(88.0)
    alt, az = alt[keep], az[keep]
    b = np.stack([np.cos(alt) * np.cos(az), np.cos(alt) * np.sin(az), np.sin(alt)], axis=1)
    R, t = proj_ref.rotation_matrix(T[:4].astype(np.float64)), T[4:7].astype(np.float64)
    d = b @ R.T
    if scene[0] == "wall":
        with np.errstate(divide="ignore"):
            s = (scene[1] - t[0]) / d[:, 0]
        hit = (d[:, 0] > 0.25) & (s > 0)
    else:
        c, rad = np.asarray(scene[1], np.float64) - t, scene[2]
        bc = d @ c
        disc = bc * bc - (c @ c - rad * rad)
        hit = disc > 0
        s = bc - np.sqrt(np.where(hit, disc, 0.0))
        hit &= s > 0
    return (b[hit] * s[hit, None]).astype(np.float32)


P0 = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
P1 = pose(25.0, -12.0, 8.0, [0.35, -0.2, 0.15])
P2 = pose(-18.0, 9.0, -15.0, [-0.25, 0.3, -0.1])
WALL, SPHERE = ("wall", 3.1), ("sphere", (3.4, 0.3, 0.2), 1.3)
NARROW, FULL = (64, 512, 40.0), (128, 512, 360.0)  # rows, cols, vertical field of view

# (id, voxel, cfg overrides, sensor, scene, [(pose, deintegrate, scan seed)])
CASES = [
    ("nearest-const-identity", 0.1, dict(scheme=0, dropoff=False), NARROW, WALL, [(P0, False, 1)]),
    ("minneighbour-dropoff-pose", 0.1, dict(scheme=1), NARROW, WALL, [(P1, False, 2)]),
    ("bilinear-invr2-nocarve-two-frames", 0.1, dict(scheme=2, const_weight=False, carving=False), FULL, WALL, [(P1, False, 3), (P2, False, 4)]),
    ("bilinear-sphere", 0.05, dict(scheme=2, dropoff=False), NARROW, SPHERE, [(P2, False, 5)]),
    ("adaptive-const-two-frames-360", 0.1, dict(scheme=3), FULL, WALL, [(P1, False, 6), (P2, False, 7)]),
    ("adaptive-small-gap-sphere", 0.05, dict(scheme=3, adaptive_gap=0.05, const_weight=False), NARROW, SPHERE, [(P1, False, 8)]),
    ("adaptive-nocarve-nodropoff-360", 0.05, dict(scheme=3, carving=False, dropoff=False), FULL, SPHERE, [(P2, False, 9), (P1, False, 10)]),
    ("integrate-then-deintegrate-invr2", 0.1, dict(scheme=3, const_weight=False), NARROW, WALL, [(P1, False, 21), (P2, False, 12), (P1, True, 21)]),
    ("integrate-deintegrate-const", 0.1, dict(scheme=2), FULL, WALL, [(P1, False, 13), (P1, True, 13), (P2, False, 14)]),
    ("max-weight-clamp", 0.1, dict(scheme=3, max_weight=1.5), NARROW, WALL, [(P1, False, 15), (P1, False, 15), (P2, False, 16)]),
]


def build_case(case):
    _, voxel, over, (rows, cols, fov), scene, seq = case
    kw = dict(truncation=3 * voxel, rows=rows, cols=cols, fov_deg=fov, min_ray=0.4, max_ray=6.0)
    kw.update(over)
    cfg = proj_ref.make_cfg(voxel, **kw)
    frames = [(T, scan(T, rows, cols, fov, scene, seed, step=2 if scene[0] == "wall" and cols * rows > 40000 else 1), de) for T, de, seed in seq]
    return cfg, fov, frames


def run_engine(eng, cfg, fov, frames):
    layer = Layer(eng, cfg["voxel_size"])
    integ = Integrator(eng, layer, eng.default_config(**engine_kwargs(cfg, fov)), "projective")
    stats = []
    for T, pts, de in frames:
        if de:
            integ.deintegrate_points(T, pts)
        else:
            integ.integrate_points(T, pts, None)
        stats.append(integ.last_stats())
    return layer, stats


def check_against_reference(layer, stats, cfg, frames, label):
    """The rule of this file, shared with the GPU test that compares the HIP engine to proj_ref directly."""
    idx, vox = layer.download()
    d, w, _ = words_to_fields(vox)
    cand = proj_ref.candidate_blocks(frames, cfg)
    ref = proj_ref.run(frames, cfg, idx, candidates=cand)
    have = {tuple(int(v) for v in b) for b in idx}
    required = {tuple(int(v) for v in b) for b in cand[ref["required"]]}
    allowed = {tuple(int(v) for v in b) for b in cand[ref["allowed"]]}
    assert required <= have, (label, "blocks the rays cross are missing", sorted(required - have)[:5])
    assert have <= allowed, (label, "blocks no ray comes near", sorted(have - allowed)[:5])
    for f, (st, rf) in enumerate(zip(stats, ref["frames"])):
        assert not rf["counts_ambiguous"], (label, f, "the cloud has points on a decision border: pick another")
        assert st["n_valid"] == rf["n_valid"] and st["n_rays"] == rf["n_rays"], (label, f, st["n_valid"], rf["n_valid"], st["n_rays"], rf["n_rays"])
    amb, upd = ref["ambiguous"], ref["updated"]
    n_upd, n_amb = int(upd.sum()), int((upd & amb).sum())
    n_cmp = int((upd & ~amb).sum())
    print(f"{label}: blocks {len(idx)} (required {len(required)}, allowed {len(allowed)}), updated {n_upd}, ambiguous {n_amb}, compared {n_cmp}")
    assert n_amb <= MAX_AMBIGUOUS_FRACTION * n_upd, (label, n_amb, n_upd)
    assert n_cmp >= MIN_COMPARED, (label, n_cmp)
    ok = ~amb
    obs_diff = ok & ((w > 0) != (ref["weight"] > 0))
    assert not obs_diff.any(), (label, "observed-ness differs", int(obs_diff.sum()), np.argwhere(obs_diff)[:3].tolist())
    err_d = np.abs(d.astype(np.float64) - ref["distance"])[ok]
    err_w = (np.abs(w.astype(np.float64) - ref["weight"]) / np.maximum(1.0, ref["weight"]))[ok]
    print(f"{label}: max |d - d_ref| {err_d.max():.3e}, max |w - w_ref| (relative to max(1, w)) {err_w.max():.3e}, observed {int((ref['weight'] > 0).sum())}")
    assert err_d.max() <= TOL, (label, "distance", float(err_d.max()))
    assert err_w.max() <= TOL, (label, "weight", float(err_w.max()))
    return dict(updated=n_upd, ambiguous=n_amb, compared=n_cmp, err_d=float(err_d.max()), err_w=float(err_w.max()))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_matches_the_float64_reference(oracle, case):
    cfg, fov, frames = build_case(case)
    layer, stats = run_engine(oracle, cfg, fov, frames)
    rep = check_against_reference(layer, stats, cfg, frames, case[0])
    if any(de for _, _, de in frames):
        assert stats[[de for _, _, de in frames].index(True)]["n_updates"] > 0


def test_the_matrix_covers_what_it_claims():
    schemes = {c[2].get("scheme", 3) for c in CASES}
    assert schemes == {0, 1, 2, 3}
    for key in ("const_weight", "carving", "dropoff"):
        assert any(c[2].get(key, True) is False for c in CASES) and any(c[2].get(key, True) for c in CASES)
    assert {c[3] for c in CASES} == {NARROW, FULL}
    assert any(len(c[5]) == 1 for c in CASES) and any(len(c[5]) == 2 for c in CASES) and any(s[1] for c in CASES for s in c[5])
    q = P1[:4].astype(np.float64)
    assert abs(np.linalg.norm(q) - 1) < 1e-6 and all(abs(v) > 0.05 for v in q[1:]) and np.any(P1[4:] != 0)  # all three axes and a translation
