"""Phase 1 of the tile apply (classify_records in coxgraph_amd/csrc/cox_apply_tile.hpp) at the record counts where its loop changes
shape.  A workgroup of 512 threads classifies a tile's records with D records per thread in flight (kClassifyDepth), so a trip of the
loop takes D * 512 records: the counts r around one thread round (511, 512, 513), around one trip (D * 512 - 1, D * 512, D * 512 + 1),
past two trips (2 * D * 512 + 1) and a tile of a single record are the cases.

Frames of ONE-POINT bundles at 5 cm, so every ray is known here: the sensor sits in the corner voxel of a tile (one z slab of a block:
16 x 16 x 1 voxels) and looks along that slab, a ray crosses 16 - 31 voxels of the sensor's tile, and the rays of a frame are chosen
-- with the oracle's `raycast` entry, called the way tests/golden/make_golden.py calls it -- so that the sensor's tile holds exactly
the frame's target.  The test counts the records of every tile of every frame from those paths, asserts that all targets occur and
that the counts add up to the oracle's n_updates, and compares the fused layer and the statistics with the CPU oracle bit for bit,
for COX_WALK=raygen and update.  One frame touches more than 255 blocks (a bucket of the one-pass partition then holds two
tiles and more); one stream has a frame that COX_RECORD_CAP drops.
"""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

from coxgraph_amd.capi import CoxError, Integrator, Layer
from util import compare_layers, compare_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = 0.05
INV = float(np.float32(1.0) / np.float32(VOXEL))
ORIGIN = np.array([0.025, 0.025, 0.025], np.float32)  # centre of voxel (0, 0, 0): the corner of block (0, 0, 0), slab 0
POSE = np.array([1, 0, 0, 0, *ORIGIN], np.float32)
CFG = dict(default_truncation_distance=0.1, min_ray_length_m=0.05, max_ray_length_m=4.0, use_const_weight=1, allow_clear=1,
           voxel_carving_enabled=1, max_weight=10000.0, use_weight_dropoff=1)
WALKS = ("raygen", "update")
COX_ERR_INTERNAL = -8
BT = 512  # threads of the tile apply's workgroup (kBT)
_cache = {}


def classify_depth():
    """D as the engine is built: kClassifyDepth of cox_apply_tile.hpp."""
    text = open(os.path.join(ROOT, "coxgraph_amd", "csrc", "cox_apply_tile.hpp")).read()
    (d,) = re.findall(r"constexpr u32 kClassifyDepth = (\d+);", text)
    assert re.search(r"constexpr u32 kBT = 512\b", text)
    return int(d)


def targets():
    d = classify_depth()
    return [1, BT - 1, BT, BT + 1, d * BT - 1, d * BT, d * BT + 1, 2 * d * BT + 1]


def point_g(oracle, p):
    out = (C.c_float * 3)()
    oracle.fn("transform_point")((C.c_float * 7)(*POSE), (C.c_float * 3)(*p), out)
    return np.array(out[:], np.float32)


def raycast(oracle, pg):
    """The voxels the integrator updates for a ray to point_G (make_golden.py's call: not clearing, carving, cast from the origin)."""
    cap = 4096
    out = (C.c_int64 * (3 * cap))()
    n = C.c_uint64()
    oracle.fn("raycast")((C.c_float * 3)(*ORIGIN), (C.c_float * 3)(*pg), 0, 1, C.c_float(CFG["max_ray_length_m"]), C.c_float(INV),
                         C.c_float(CFG["default_truncation_distance"]), 1, out, C.c_uint64(cap), C.byref(n))
    assert n.value <= cap
    return np.array(out[:3 * n.value], np.int64).reshape(-1, 3)


def tiles_of(path):
    """records per tile of one ray: tile = (block x, block y, z voxel)"""
    return collections.Counter((int(x) >> 4, int(y) >> 4, int(z)) for x, y, z in path)


class Candidate:
    def __init__(self, oracle, p):
        self.p = np.asarray(p, np.float32)
        pg = point_g(oracle, self.p)
        self.voxel = tuple(int(v) for v in np.floor(pg.astype(np.float64) * INV + 1e-6))  # (points keep away from voxel faces)
        self.tiles = tiles_of(raycast(oracle, pg))
        self.home = self.tiles[(0, 0, 0)]  # records in the sensor's tile


def slab_candidates(oracle):
    """Rays inside slab 0 into the quadrant x, y > 0, each with a terminal voxel of its own: long ones (they cross the sensor's tile,
    16 - 31 records there) and short ones that end inside it (a few records: the change for the exact count)."""
    if "slab" not in _cache:
        rng = np.random.default_rng(7)
        seen, long_, short = set(), [], []
        for length, angle in [(l, a) for l in np.arange(1.3, 3.9, 0.13) for a in np.linspace(0.06, 1.51, 48)] + \
                             [(l, a) for l in np.arange(0.08, 0.8, 0.03) for a in (0.2, 0.5, 0.8, 1.1, 1.4)]:
            a = angle + rng.uniform(-0.01, 0.01)
            c = Candidate(oracle, [length * np.cos(a), length * np.sin(a), 0.0])
            if c.voxel in seen or any(t[2] != 0 for t in c.tiles):
                continue
            seen.add(c.voxel)
            (long_ if length > 1.0 else short).append(c)
        _cache["slab"] = (long_, short)
    return _cache["slab"]


def lone_record_ray(oracle):
    """A ray into the opposite quadrant whose last tile holds exactly one record (and which no ray of the quadrant x, y > 0 meets)."""
    if "lone" not in _cache:
        for length in np.arange(1.0, 2.0, 0.004):
            c = Candidate(oracle, [-length * 0.94, -length * 0.34, 0.0])
            if 1 in [n for t, n in c.tiles.items() if t != (0, 0, 0)]:
                _cache["lone"] = c
                break
    return _cache["lone"]


def frame_with(oracle, r, lone=False):
    """Rays that put exactly r records into the sensor's tile."""
    long_, short = slab_candidates(oracle)
    chosen = [lone_record_ray(oracle)] if lone else []
    left = r - sum(c.home for c in chosen)
    pool = list(long_)
    while left > 80:  # whole crossings first
        c = pool.pop()
        chosen.append(c)
        left -= c.home
    # the change: one, two or three of the remaining candidates (every ray that starts here leaves at least its first voxel)
    rest = pool + short
    by_home = {}
    for c in rest:
        by_home.setdefault(c.home, []).append(c)
    pick = None
    homes = sorted(by_home)
    for a in homes:
        if a == left:
            pick = [by_home[a][0]]
            break
        for b in homes:
            if a + b == left and (a != b or len(by_home[a]) > 1):
                pick = [by_home[a][0], by_home[b][-1]]
                break
            rem = left - a - b
            if rem in by_home and len({a, b, rem}) == 3:
                pick = [by_home[a][0], by_home[b][0], by_home[rem][0]]
                break
        if pick:
            break
    assert pick is not None, (r, left)
    chosen += pick
    assert sum(c.home for c in chosen) == r and len({c.voxel for c in chosen}) == len(chosen)
    return chosen


def fan_frame(oracle):
    """Rays in all directions: more than 255 touched blocks."""
    if "fan" not in _cache:
        rng = np.random.default_rng(3)
        seen, out = set(), []
        for _ in range(700):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            c = Candidate(oracle, d * rng.uniform(3.0, 3.9))
            if c.voxel not in seen:
                seen.add(c.voxel)
                out.append(c)
        _cache["fan"] = out
    return _cache["fan"]


def cloud_of(cands, seed):
    """(points, colours, records per tile) of a frame"""
    rng = np.random.default_rng(seed)
    pts = np.ascontiguousarray(np.stack([c.p for c in cands]).astype(np.float32))
    rgba = rng.integers(0, 256, (len(cands), 4), dtype=np.uint8)
    tiles = collections.Counter()
    for c in cands:
        tiles.update(c.tiles)
    return pts, rgba, tiles


def the_frames(oracle):
    """The fan first (an empty layer: its new blocks are its touched blocks), then one frame per target."""
    if "frames" not in _cache:
        frames = [cloud_of(fan_frame(oracle), 0)]
        for k, r in enumerate(t for t in targets() if t > 1):
            frames.append(cloud_of(frame_with(oracle, r, lone=(k == 0)), 1 + k))
        _cache["frames"] = frames
    return _cache["frames"]


def run(eng, clouds, env=None, monkeypatch=None):
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    layer = Layer(eng, VOXEL, capacity_blocks=4096)
    integ = Integrator(eng, layer, eng.default_config(integrator_threads=1, **CFG), "merged")  # (the switches are read here)
    for name in env or {}:
        monkeypatch.delenv(name)
    stats = []
    for pts, rgba, _ in clouds:
        integ.integrate_points(POSE, pts, rgba)
        stats.append(integ.last_stats())
    return layer, stats


def oracle_run(oracle, key, clouds):
    if key not in _cache:
        _cache[key] = run(oracle, clouds)
    return _cache[key]


def test_the_frames_hold_every_target(oracle):
    """What the cases claim, on the paths and on the oracle: every target is the record count of a tile of some frame, a frame's
    rays are bundles of one point, its tile counts add up to the oracle's updates, and the first frame touches more than 255 blocks."""
    frames = the_frames(oracle)
    _, so = oracle_run(oracle, "all", frames)
    counts = set()
    for (pts, _, tiles), s in zip(frames, so):
        assert s["n_rays"] == s["n_valid"] == len(pts) and s["max_bundle_points"] == 1
        assert sum(tiles.values()) == s["n_updates"]
        counts |= set(tiles.values())
    missing = [r for r in targets() if r not in counts]
    assert not missing, missing
    for (_, _, tiles), r in zip(frames[1:], [t for t in targets() if t > 1]):
        assert tiles[(0, 0, 0)] == r == max(tiles.values())
    assert so[0]["n_new_blocks"] > 255 and len({t[:2] + (t[2] >> 4,) for t in frames[0][2]}) == so[0]["n_new_blocks"]


@pytest.mark.parametrize("walk", WALKS)
def test_tiles_at_the_loop_edges_equal_the_oracle(hip, oracle, monkeypatch, walk):
    frames = the_frames(oracle)
    lo, so = oracle_run(oracle, "all", frames)
    lh, sh = run(hip, frames, dict(COX_WALK=walk), monkeypatch)
    compare_stats(sh, so)
    assert sh[0]["n_touched_blocks"] > 255
    rep = compare_layers(lh, lo)
    assert rep["bitexact_d"] and rep["bitexact_w"] and rep["n_diff_color"] == 0, rep


def _blocks(layer):
    idx, vox = layer.download()
    return {tuple(int(x) for x in i): v for i, v in zip(idx, vox)}


@pytest.mark.parametrize("walk", WALKS)
def test_a_dropped_frame_between_them(hip, oracle, monkeypatch, walk):
    """COX_RECORD_CAP between the target frames' records and the fan's: the fan is dropped as a whole and reported once; it still
    allocates its blocks and writes no voxel, and the frames around it are the oracle's."""
    frames = the_frames(oracle)
    fan, rest = frames[0], frames[1:]
    fed = rest[:3] + [fan] + rest[3:]
    lk, sk = oracle_run(oracle, "kept", rest)
    lf, sf = oracle_run(oracle, "fed", fed)
    most, full = max(s["n_updates"] for s in sk), sf[3]["n_updates"]
    cap = (most + full) // 2
    assert most < cap < full
    env = dict(COX_WALK=walk, COX_RECORD_CAP=str(cap))
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    layer = Layer(hip, VOXEL, capacity_blocks=4096)
    integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **CFG), "merged")
    for name in env:
        monkeypatch.delenv(name)
    for k, (pts, rgba, _) in enumerate(fed):
        if k == 3:
            with pytest.raises(CoxError) as e:
                integ.integrate_points(POSE, pts, rgba)
            assert e.value.status == COX_ERR_INTERNAL
        else:
            integ.integrate_points(POSE, pts, rgba)
    # the last frame is the oracle's of the stream without the dropped frame -- but for its new blocks: the dropped frame allocated
    # what it touched, so that count is the one of the stream that fused it
    keys = ("n_points", "n_valid", "n_rays", "n_updates", "n_touched_voxels", "max_bundle_points", "max_voxel_updates")
    compare_stats([integ.last_stats()], [sk[-1]], keys)
    assert integ.last_stats()["n_new_blocks"] == sf[-1]["n_new_blocks"]
    got, voxels, blocks = _blocks(layer), _blocks(lk), _blocks(lf)
    assert set(got) == set(blocks)
    for key, vox in got.items():
        if key in voxels:
            assert np.array_equal(vox, voxels[key]), key
        else:
            assert not vox[:, 1].any(), key  # allocated by the dropped frame only: no voxel observed
