"""Bundle boundaries of the merged integrator, at the shapes where they can go wrong.

A merged frame sorts its points by (clearing, first visit of the bundle) and needs, for every bundle, its ordinal and the start of
its run in the sorted array.  Both come from the bundle's HEAD -- the point visited first -- which is known before the sort: its rank
among the heads of its class is counted per tile of 2048 consecutive visits, and the sort's last scatter pass writes the start when
it places the head.  The cases below put heads on tile and wave edges, make both head classes occur, interleave
invalid points, take the one-pass and the two-pass key widths, and reuse every buffer set.

Every cloud is designed in VISITING order (sequence numbers; the engine visits point mixed_index(seq, n) at step seq) from a list of
(class, voxel id) per visit, so the bundle structure of a case is known here without running anything: `model()` derives the bundles
and their heads from that list, each test asserts the property it is meant to cover on the model, and the oracle's bundle count
(n_rays) must equal the model's.  The fused layer is compared with the oracle's bit for bit.
"""
import numpy as np
import pytest

from coxgraph_amd.capi import Layer, Integrator
from util import compare_layers, compare_stats

pytestmark = pytest.mark.gpu

VOXEL = 0.1
TILE = 2048  # visits per tile of the head count (= the radix sort's tile)
POSE = np.array([1, 0, 0, 0, 0.013, 0.021, 0.007], np.float32)
CFG = dict(default_truncation_distance=0.3, min_ray_length_m=0.2, max_ray_length_m=4.0, use_const_weight=1, allow_clear=1,
           voxel_carving_enabled=1, max_weight=10000.0, use_weight_dropoff=1)
PLAIN, CLEAR, NAN, NEAR = 0, 1, 2, 3  # class of a visit: inside the range, beyond max_ray_length_m, not finite, nearer than min_ray_length_m
VOXELS_PER_CLASS = 16 * 25 * 17


def mixed_index(seq, n):
    """voxblox MixedThreadSafeIndex: the point visited at step seq."""
    seq = np.asarray(seq, np.int64)
    groups = n >> 10
    if groups == 0:
        return seq
    return np.where(seq >= (groups << 10), seq, (seq % groups) * 1024 + seq // groups)


def make_cloud(cls, vid, seed):
    """Points (sensor frame, in the order the caller passes them) and colours for visits of class cls[s] in voxel vid[s].
    PLAIN voxels lie 0.8 - 2.8 m from the sensor, CLEAR ones 4.5 - 6.3 m; points keep 0.03 m away from their voxel's faces."""
    cls, vid = np.asarray(cls), np.asarray(vid)
    n = len(cls)
    assert n == 0 or int(vid.max()) < VOXELS_PER_CLASS
    rng = np.random.default_rng(seed)
    ix = np.where(cls == CLEAR, 45, 8) + vid % 16
    iy = -12 + (vid // 16) % 25
    iz = -8 + vid // 400
    centre = (np.stack([ix, iy, iz], axis=-1) + 0.5) * VOXEL
    p = centre + rng.uniform(-0.02, 0.02, (n, 3)) - POSE[4:].astype(np.float64)
    near = rng.uniform(0.02, 0.05, (n, 3))
    p[cls == NEAR] = near[cls == NEAR]
    nan_rows = np.flatnonzero(cls == NAN)
    p[nan_rows, nan_rows % 3] = np.nan
    pts = np.empty((n, 3), np.float32)
    rgba = np.empty((n, 4), np.uint8)
    idx = mixed_index(np.arange(n), n)
    pts[idx] = p.astype(np.float32)
    rgba[idx] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    return pts, rgba


def model(cls, vid, allow_clear=True):
    """Bundles of a frame from its visit list: heads (sequence numbers), their classes, bundle sizes."""
    cls, vid = np.asarray(cls), np.asarray(vid)
    valid = (cls == PLAIN) | ((cls == CLEAR) & allow_clear)
    seq = np.flatnonzero(valid)
    key = cls[seq].astype(np.int64) * VOXELS_PER_CLASS + vid[seq]
    _, first, counts = np.unique(key, return_index=True, return_counts=True)
    heads = seq[first]
    order = np.argsort(heads)
    return dict(n_valid=int(valid.sum()), n_bundles=len(heads), heads=heads[order], head_cls=cls[heads[order]], sizes=counts[order])


def sort_passes(n):
    """Passes of the bundling sort: key bits = clearing bit + log2(smallest power of two > n), digits of at most 11 bits."""
    bits = 1 + int(n).bit_length()
    return (bits + 10) // 11


def fuse(eng, clouds, overrides=None):
    cfg_kw = dict(CFG)
    cfg_kw.update(overrides or {})
    layer = Layer(eng, VOXEL, capacity_blocks=4096)
    integ = Integrator(eng, layer, eng.default_config(**cfg_kw), "merged")
    stats = []
    for pts, rgba in clouds:
        integ.integrate_points(POSE, pts, rgba)
        stats.append(integ.last_stats())
    return layer, stats


def check(hip, oracle, frames, overrides=None):
    """frames: [(cls, vid)] per frame.  Layer bit for bit, bundle counts per frame against the oracle and against the model."""
    allow_clear = bool((overrides or {}).get("allow_clear", 1))
    clouds = [make_cloud(c, v, seed=11 + k) for k, (c, v) in enumerate(frames)]
    lo, so = fuse(oracle, clouds, overrides)
    for (c, v), s in zip(frames, so):
        m = model(c, v, allow_clear)
        assert (s["n_rays"], s["n_valid"]) == (m["n_bundles"], m["n_valid"]), (s, m["n_bundles"], m["n_valid"])
    lh, sh = fuse(hip, clouds, overrides)
    print([s["n_rays"] for s in sh], [s["n_rays"] for s in so])
    compare_stats(sh, so)
    rep = compare_layers(lh, lo)
    assert rep["bitexact_d"] and rep["bitexact_w"] and rep["n_diff_color"] == 0, rep


def mixed_visits(n, seed=0):
    """Both classes interleaved, bundles of many sizes spread over the whole frame, and a bundle of its own for the visits on the
    wave, tile and frame edges (so each of them is a head)."""
    rng = np.random.default_rng(100 + seed + n)
    m = max(1, min(n // 3, 600))
    vid = rng.integers(0, m, n)
    cls = (vid % 3 == 1).astype(np.int64)  # a third of the voxels are CLEAR ones
    edges = [s for s in (0, 63, 64, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1) if 0 <= s < n]
    for j, s in enumerate(edges):
        vid[s] = m + j
        cls[s] = j % 2
    return cls, vid


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_cloud_sizes_around_wave_and_tile_edges(hip, oracle, n):
    cls, vid = mixed_visits(n)
    m = model(cls, vid)
    assert sort_passes(n) == (1 if n <= 65 else 2)
    heads = set(m["heads"].tolist())
    assert n - 1 in heads  # a head on the frame's last position
    if n > 65:
        assert {63, 64} <= heads and set(m["head_cls"][np.isin(m["heads"], [63, 64])].tolist()) == {PLAIN, CLEAR}
    if n > TILE:
        assert {TILE - 1, TILE} <= heads  # last position of a tile, first of the next one
    if n >= 64:
        assert (m["head_cls"] == PLAIN).sum() > 1 and (m["head_cls"] == CLEAR).sum() > 1
        # heads of the clearing class in front of heads of the other one: the class base is needed
        assert m["heads"][m["head_cls"] == CLEAR].min() < m["heads"][m["head_cls"] == PLAIN].max()
    check(hip, oracle, [(cls, vid)])


def test_one_bundle_longer_than_a_tile(hip, oracle):
    n = TILE + 452
    cls, vid = np.zeros(n, np.int64), np.full(n, 77)
    m = model(cls, vid)
    assert m["n_bundles"] == 1 and m["sizes"][0] > TILE
    check(hip, oracle, [(cls, vid)])


def test_every_point_its_own_bundle(hip, oracle):
    n = 2 * TILE + 1
    cls, vid = np.arange(n) % 2, np.arange(n) // 2
    m = model(cls, vid)
    assert m["n_bundles"] == n and np.array_equal(m["heads"], np.arange(n))
    check(hip, oracle, [(cls, vid)])


def test_classes_interleaved_with_bundles_across_tiles(hip, oracle):
    """Alternating classes; every bundle has a member in each of the three tiles, all heads sit in the first one."""
    n = 2 * TILE + 300
    s = np.arange(n)
    cls, vid = s % 2, (s // 2) % 150
    m = model(cls, vid)
    assert m["n_bundles"] == 300 and m["heads"].max() < TILE and m["sizes"].min() > 6
    assert (m["head_cls"] == CLEAR).sum() == 150
    check(hip, oracle, [(cls, vid)])


def _with_invalid(n_valid, where, kinds):
    """Visit list of n_valid valid visits (mixed_visits) with invalid ones of the given kinds placed first / last / between."""
    vc, vv = mixed_visits(n_valid, seed=5)
    if CLEAR in kinds:  # (allow_clear = 0: a CLEAR visit is an invalid one, so the valid ones are all PLAIN)
        vc = np.zeros_like(vc)
    if where == "first":
        k = len(kinds) * 40
        cls = np.concatenate([np.resize(kinds, k), vc])
        vid = np.concatenate([np.arange(k) % 50, vv])
    elif where == "last":
        k = len(kinds) * 40
        cls = np.concatenate([vc, np.resize(kinds, k)])
        vid = np.concatenate([vv, np.arange(k) % 50])
    else:  # between every two valid visits
        cls = np.empty(2 * n_valid - 1, np.int64)
        vid = np.empty(2 * n_valid - 1, np.int64)
        cls[0::2], vid[0::2] = vc, vv
        cls[1::2] = np.resize(kinds, n_valid - 1)
        vid[1::2] = np.arange(n_valid - 1) % 50
    return cls, vid


@pytest.mark.parametrize("allow_clear", [1, 0])
def test_invalid_points_first_last_between_and_alone(hip, oracle, allow_clear):
    """NaN and too-near points (and, with allow_clear = 0, the points beyond the maximum range: the reject path) in front of,
    behind and between the valid ones; a cloud without a valid point; an empty cloud between two normal frames."""
    kinds = [NAN, NEAR] if allow_clear else [NAN, NEAR, CLEAR]
    frames = [_with_invalid(1500, w, kinds) for w in ("first", "last", "between")]
    frames.append((np.resize(kinds, 300), np.arange(300) % 50))  # no valid point at all
    frames.append(mixed_visits(900, seed=1))
    frames.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))  # empty
    frames.append(mixed_visits(2500, seed=2))
    for (c, v), where in zip(frames[:3], ("first", "last", "between")):
        m = model(c, v, bool(allow_clear))
        bad = ~((c == PLAIN) | ((c == CLEAR) & bool(allow_clear)))
        assert set(c[bad].tolist()) == set(kinds) and m["n_bundles"] > 100
        assert {"first": bad[0] and not bad[-1], "last": bad[-1] and not bad[0], "between": bad[1::2].all() and not bad[0::2].any()}[where]
        assert len(c) > TILE or where != "between"
    assert model(*frames[3], bool(allow_clear))["n_bundles"] == 0
    check(hip, oracle, frames, dict(allow_clear=allow_clear))


@pytest.mark.parametrize("anti_grazing", [0, 1])
def test_every_buffer_set_is_reused(hip, oracle, anti_grazing):
    """Thirteen different frames through one integrator (six frame sets, three bundle sets): one-pass and two-pass key widths in
    turn, the same voxels hit again in another order -- a hash slot left behind by an earlier frame would give a bundle the wrong
    first visit.  With the frame's own clean-up of the hash, and with anti-grazing (the hash is cleared by a memset instead)."""
    sizes = [700, 3000, 64, 2048, 5000, 1, 2049, 900, 4097, 333, 2500, 1023, 1024]
    frames = [mixed_visits(n, seed=k) for k, n in enumerate(sizes)]
    assert {sort_passes(n) for n in sizes} == {1, 2} and sort_passes(1023) == 1 and sort_passes(1024) == 2
    check(hip, oracle, frames, dict(enable_anti_grazing=anti_grazing))


def test_depth_entry_point_with_count_on_the_device(hip, oracle):
    """cox_integrate_depth_dev: the frame's point count never visits the host.  80 x 60 pixels (4 800 > two tiles), with NaN, zero,
    too-near and beyond-range pixels."""
    import torch
    w, h = 80, 60
    fx, fy, cx, cy = (np.float32(x) for x in (76.4, 76.2, 40.4, 30.6))
    rng = np.random.default_rng(3)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    depth = (1.6 + 0.5 * np.sin(uu / 9.0) * np.cos(vv / 7.0)).astype(np.float32)
    r = rng.random((h, w))
    depth[r < 0.05] = np.nan
    depth[(r >= 0.05) & (r < 0.08)] = 0.0
    depth[(r >= 0.08) & (r < 0.11)] = 0.1   # nearer than min_ray_length_m
    depth[(r >= 0.11) & (r < 0.25)] = 5.5 + 0.3 * np.sin(uu / 5.0)[(r >= 0.11) & (r < 0.25)]  # beyond max_ray_length_m: clearing
    rgba = rng.integers(0, 256, (h * w, 4), dtype=np.uint8)
    xn = ((np.arange(w, dtype=np.float32) - cx) / fx).astype(np.float32)
    yn = ((np.arange(h, dtype=np.float32) - cy) / fy).astype(np.float32)
    pts = np.stack([depth * xn[None, :], depth * yn[:, None], depth], axis=-1).astype(np.float32).reshape(-1, 3)
    keep = np.isfinite(depth.reshape(-1)) & (depth.reshape(-1) > 0)
    pts, cols = np.ascontiguousarray(pts[keep]), np.ascontiguousarray(rgba[keep])
    assert 2 * TILE < len(pts) < h * w
    lo, so = fuse(oracle, [(pts, cols)])
    assert 100 < so[0]["n_rays"] < so[0]["n_valid"] < len(pts)
    lh = Layer(hip, VOXEL, capacity_blocks=4096)
    ih = Integrator(hip, lh, hip.default_config(**CFG), "merged")
    d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(rgba).cuda()
    torch.cuda.synchronize()
    ih.integrate_depth_dev(POSE, d.data_ptr(), c.data_ptr(), w, h, np.array([fx, fy, cx, cy], np.float32))
    ih.sync()
    compare_stats([ih.last_stats()], so)
    rep = compare_layers(lh, lo)
    assert rep["bitexact_d"] and rep["bitexact_w"] and rep["n_diff_color"] == 0, rep
