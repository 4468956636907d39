"""Edges of finishSubmap() on the GPU, each against the oracle and the numpy references (tests/submap_ref.py): the places where
a tiled relaxation with halos, a neighbour table and a launch cap goes wrong without the room scene noticing."""
import numpy as np
import pytest

from coxgraph_amd import synth
from coxgraph_amd.capi import CoxError, Integrator, Layer
from test_gpu_submap_fuzz import compare_engines, oracle_twin
from test_submap_ref_cpu import check_box, check_esdf, check_exact_thresholds, check_iso, check_sampler, ref_mesh, unit_weight_points  # noqa: F401

pytestmark = pytest.mark.gpu
LIN = np.arange(4096)
LOC = np.stack([LIN % 16, (LIN // 16) % 16, LIN // 256], axis=1)


def words(d, w):
    v = np.zeros(d.shape + (3,), np.uint32)
    v[..., 0], v[..., 1] = np.asarray(d, np.float32).view(np.uint32), np.asarray(w, np.float32).view(np.uint32)
    return v


def layers(hip, oracle, voxel, idx, vox):
    lh = Layer(hip, voxel, capacity_blocks=max(64, len(idx)))
    if len(idx):
        lh.upload(np.asarray(idx, np.int32), vox)
    return lh, oracle_twin(oracle, lh)


def wave_field(idx, voxel, trunc, seed, local=False):
    """smooth field with zero crossings every few voxels; local = from the voxel's coordinates inside the block pair only
    (blocks at the ends of the index range: their world coordinates have no float32 resolution left)"""
    rng = np.random.default_rng(seed)
    idx = np.asarray(idx, np.int64)
    g = (idx - idx.min(axis=0) if local else idx)[:, None, :] * 16 + LOC[None]
    d = np.zeros(g.shape[:2])
    for _ in range(3):
        d += 2.0 * voxel * np.sin(g @ rng.normal(size=3) * (2 * np.pi / rng.uniform(10, 30)) + rng.uniform(0, 6.28))
    return np.clip(d, -trunc, trunc).astype(np.float32)


ESDF = dict(max_distance_m=2.0, min_distance_m=0.075)


def test_empty_layer(hip, oracle, ref_mesh):  # noqa: F811
    lh, lo = layers(hip, oracle, 0.05, np.zeros((0, 3), np.int32), np.zeros((0, 4096, 3), np.uint32))
    ph, _, eh, _ = compare_engines(hip, oracle, lh, lo, ESDF, dict(min_weight=1.0))
    assert ph.n == 0 and eh.n_blocks() == 0
    mn, mx, n = lh.surface_obb()
    assert n == 0 and np.all(np.isinf(mn)) and np.all(np.isinf(mx))


def test_blocks_with_nothing_observed(hip, oracle, ref_mesh):  # noqa: F811
    idx = np.array([[0, 0, 0], [1, 0, 0], [-1, -1, -1]], np.int32)
    d = wave_field(idx, 0.05, 0.15, 1)
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, np.zeros_like(d)))
    ph, _, _, _ = compare_engines(hip, oracle, lh, lo, ESDF, dict(min_weight=1e-4))
    ref, _, n_moved, _ = check_esdf(lh, ESDF, "unobserved")
    assert ph.n == 0 and ph.n_mesh_vertices == 0 and not ref.observed.any() and n_moved == 0
    assert check_box(lh) == 0


def test_observed_without_a_fixed_voxel_stays_at_the_default(hip, oracle):
    idx = np.array([[x, y, 0] for x in range(2) for y in range(2)], np.int32)
    d = np.where(wave_field(idx, 0.05, 0.15, 2) > 0, np.float32(0.15), np.float32(-0.15))
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, np.full_like(d, 3.0)))
    cfg = dict(max_distance_m=2.0, min_distance_m=0.1, default_distance_m=1.5)
    compare_engines(hip, oracle, lh, lo, cfg, dict(min_weight=1.0))
    ref, e, n_moved, _ = check_esdf(lh, cfg, "no fixed voxel")
    assert not ref.fixed.any() and n_moved == 0 and set(np.unique(ref.distance)) == {np.float32(-1.5), np.float32(1.5)}


def test_nan_distances_and_weights_are_observed_and_negative(hip, oracle):
    """Pinned: NaN fails `w < min_weight` (observed) and `|d| < min_d` and `d > 0` (starts at -default)."""
    idx = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
    d = wave_field(idx, 0.05, 0.15, 3)
    w = np.full_like(d, 2.0)
    r = np.random.default_rng(3).random(d.shape)
    d[r < 0.02] = np.nan
    w[(r > 0.02) & (r < 0.04)] = np.nan
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, w))
    eh, eo = lh.esdf(**ESDF), lo.esdf(**ESDF)
    assert np.array_equal(eh.download()[1], eo.download()[1])
    ref, _, n_moved, _ = check_esdf(lh, ESDF, "NaN")
    assert ref.observed[np.isnan(w)].all() and np.all(ref.initial[np.isnan(d)] == np.float32(-2.0)) and n_moved > 1000
    assert not np.isnan(ref.distance).any()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_blocks_at_the_ends_of_the_index_range(hip, oracle, axis):
    """k_esdf_neighbors' range guard: the lowest / highest block index a layer accepts (-2^20 + 1 and 2^20 - 2), each with a
    neighbour next to it; their outer neighbours (-2^20, 2^20 - 1) are valid keys that hold no block.  The two indices beyond
    are refused by the layer."""
    lo_i, hi_i = -(1 << 20) + 1, (1 << 20) - 2
    idx = np.zeros((4, 3), np.int32)
    idx[:, axis] = [lo_i, lo_i + 1, hi_i - 1, hi_i]
    idx[:, (axis + 1) % 3] = [5, 5, -7, -7]
    d = wave_field(idx, 0.05, 0.15, 10 + axis, local=True)
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, np.full_like(d, 2.0)))
    eh, eo = lh.esdf(**ESDF), lo.esdf(**ESDF)
    assert np.array_equal(eh.download()[0], eo.download()[0]) and np.array_equal(eh.download()[1], eo.download()[1])
    ref, _, n_moved, n_neg = check_esdf(lh, ESDF, f"index range axis {axis}")
    assert n_moved > 1000 and n_neg > 50
    check_box(lh)
    a, b = lh.surface_obb(), lo.surface_obb()
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for bad in (-(1 << 20), (1 << 20) - 1):
        out = np.zeros((1, 3), np.int32)
        out[0, axis] = bad
        with pytest.raises(CoxError):
            Layer(hip, 0.05).upload(out, words(d[:1], np.full_like(d[:1], 2.0)))


def test_two_blocks_sharing_only_a_corner(hip, oracle, ref_mesh):  # noqa: F811
    """The only way across is the (+1, +1, +1) halo entry: a fixed band in the first block, none in the second."""
    idx = np.array([[-1, -1, -1], [0, 0, 0]], np.int32)
    g = idx[:, None, :].astype(np.int64) * 16 + LOC[None]
    # distance to the plane x + y + z = -6 voxels (through the first block), clamped: the second block holds +trunc only
    d = np.clip((g.sum(axis=2) + 1.5 + 6) / np.sqrt(3.0) * 0.05, -0.15, 0.15).astype(np.float32)
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, np.full_like(d, 2.0)))
    compare_engines(hip, oracle, lh, lo, ESDF, dict(min_weight=1.0))
    ref, _, _, _ = check_esdf(lh, ESDF, "corner")
    second = ref.distance[np.all(lh.download()[0] == 0, axis=1)][0]
    assert not ref.fixed[np.all(lh.download()[0] == 0, axis=1)].any()
    assert (second != np.float32(2.0)).sum() > 1000           # the wavefront arrived through the corner voxel
    check_iso(hip, lh, ref_mesh, 1.0, 0.025, "corner")


def serpentine(n_blocks):
    """A one-voxel corridor of observed voxels through unobserved space, in the plane z = 8 of a chain of blocks along x: in
    every block rows y = 0, 2, .. 12 over x = 1 .. 14 joined at alternating ends, entered at x = 0 and left at x = 15 (106
    voxels); neighbouring blocks touch only where the corridor passes."""
    idx = np.array([[b, 0, 0] for b in range(n_blocks)], np.int32)
    w = np.zeros((n_blocks, 16, 16, 16), np.float32)   # [block, z, y, x]
    for b in range(n_blocks):
        rows = list(range(0, 13, 2))
        if b % 2:
            rows.reverse()
        for k, y in enumerate(rows):
            w[b, 8, y, 1:15] = 1.0
            if k + 1 < len(rows):
                w[b, 8, (y + rows[k + 1]) // 2, 14 if k % 2 == 0 else 1] = 1.0
        w[b, 8, rows[0], 0] = w[b, 8, rows[-1], 15] = 1.0
    d = np.full_like(w, 0.15)
    d[0, 8, 0, 0] = 0.01                                 # the only fixed voxel: the corridor's entrance
    return idx, words(d.reshape(n_blocks, 4096), w.reshape(n_blocks, 4096)), int(w.sum())


def test_serpentine_corridor_needs_many_iterations_and_launches(hip, oracle):
    """106 voxels of corridor per block (> the 64 in-tile iterations of one launch) and 12 blocks in a chain (the wavefront
    crosses one block per launch at best): the relaunch loop has to carry it to the end.  The engine does not report its
    launch count; that 2-3 launches per block stay far below the `+ 4096` cap is an argument, not a measurement.  What is
    asserted: esdf() returns (it fails with COX_ERR_INTERNAL at the cap) and gives the reference's bits."""
    idx, vox, length = serpentine(12)
    assert length == 12 * 106
    lh, lo = layers(hip, oracle, 0.05, idx, vox)
    cfg = dict(max_distance_m=1000.0, min_distance_m=0.075, default_distance_m=1000.0)
    eh, eo = lh.esdf(**cfg), lo.esdf(**cfg)            # returns: converged (COX_ERR_INTERNAL otherwise)
    assert np.array_equal(eh.download()[1], eo.download()[1])
    ref, _, n_moved, _ = check_esdf(lh, cfg, "serpentine")
    assert n_moved == length - 1
    end = ref.distance[11].reshape(16, 16, 16)[8, 0, 15]
    print(f"[serpentine] corridor {length} voxels, far end at {end:.3f} m")
    # every row was walked: a diagonal step cuts a corner by one voxel, twice per turn, 6 turns and 2 doors per block
    assert 0.05 * (length - 12 * 14) <= end < 0.05 * np.sqrt(2.0) * length


def test_thick_negative_region(hip, oracle, ref_mesh):  # noqa: F811
    """A solid sphere several blocks across: the negative wavefront runs 20 voxels deep through four blocks per axis."""
    idx = np.array([[x, y, z] for z in range(-2, 2) for y in range(-2, 2) for x in range(-2, 2)], np.int32)
    c = ((idx[:, None, :].astype(np.int64) * 16 + LOC[None]) + 0.5) * 0.05
    d = np.clip(np.linalg.norm(c - np.array([0.03, -0.02, 0.01]), axis=2) - 1.3, -0.15, 0.15).astype(np.float32)
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, np.full_like(d, 2.0)))
    cfg = dict(max_distance_m=2.0, min_distance_m=0.1)
    compare_engines(hip, oracle, lh, lo, cfg, dict(min_weight=1.0))
    ref, _, n_moved, n_neg = check_esdf(lh, cfg, "solid sphere")
    assert n_neg > 50000 and ref.distance.min() < -1.2


def test_esdf_with_frames_in_flight_and_called_twice(hip):
    """esdf() of a layer whose frames are still in flight equals esdf() after a wait; a second call gives the same bits and
    leaves the TSDF as it was, word for word."""
    import torch
    cfg = hip.default_config(**synth.integrator_overrides(0.10))
    layer = Layer(hip, 0.10, capacity_blocks=4096)
    integ = Integrator(hip, layer, cfg, "merged")
    dev = [(T, torch.from_numpy(np.ascontiguousarray(p[::4])).cuda(), torch.from_numpy(np.ascontiguousarray(c[::4])).cuda())
           for T, p, c, _ in (synth.make_frame(t) for t in range(0, 60, 10))]
    torch.cuda.synchronize()
    for T, xyz, rgba in dev:
        integ.integrate_points_dev(T, xyz.data_ptr(), rgba.data_ptr(), xyz.shape[0])
    kw = dict(max_distance_m=2.0, min_distance_m=0.15)
    e1 = layer.esdf(**kw).download()
    integ.sync()
    before = layer.download()
    e2 = layer.esdf(**kw).download()
    e3 = layer.esdf(**kw).download()
    after = layer.download()
    assert int((before[1][..., 1] != 0).sum()) > 10000        # a fused room, not an empty layer
    assert np.array_equal(e1[0], e2[0]) and np.array_equal(e1[1], e2[1]) and np.array_equal(e2[1], e3[1])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    check_esdf(layer, kw, "after the stream")


def test_isosurface_merge_with_crowded_cells_and_without_survivors(hip, oracle, ref_mesh):  # noqa: F811
    """A proximity threshold of 4 voxels (hundreds of vertices per hash cell) on blocks at negative indices (the `- 4` margin
    of the cell origin), one cell for the whole mesh (every probe of the table lands on one key), a field without a
    zero crossing (no vertex at all), and a mesh all of whose vertices fail the interpolation's validity rule."""
    idx = np.array([[x, y, -2] for x in range(-3, -1) for y in range(-3, -1)], np.int32)
    d = wave_field(idx, 0.05, 0.15, 7)
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, np.full_like(d, 2.0)))
    for thr in (0.2, 1000.0):
        ph, _, _, _ = compare_engines(hip, oracle, lh, lo, ESDF, dict(min_weight=1.0, vertex_proximity_threshold=thr))
        r, _ = check_iso(hip, lh, ref_mesh, 1.0, thr, f"threshold {thr}")
        assert r.n_mesh_vertices > 50 * max(r.n_connected, 1)
    assert ph.n_connected_vertices == 1
    lh, lo = layers(hip, oracle, 0.05, idx, words(np.abs(d) + np.float32(0.01), np.full_like(d, 2.0)))
    ph, _, _, _ = compare_engines(hip, oracle, lh, lo, ESDF, dict(min_weight=1.0))
    assert (ph.n_mesh_vertices, ph.n_connected_vertices, ph.n) == (0, 0, 0)
    assert check_iso(hip, lh, ref_mesh, 1.0, 0.025, "no crossing")[0].n_mesh_vertices == 0
    # vertices exist but none survives: every weight is 0, which a negative min_weight lets the mesher accept (0 > -1) while
    # the interpolation's validity rule (weight > 0) rejects all 8 neighbours of every vertex
    lh, lo = layers(hip, oracle, 0.05, idx, words(d, np.zeros_like(d)))
    ph, _, _, _ = compare_engines(hip, oracle, lh, lo, ESDF, dict(min_weight=-1.0))
    assert ph.n_mesh_vertices > 1000 and ph.n_connected_vertices > 100 and ph.n == 0
    r, _ = check_iso(hip, lh, ref_mesh, -1.0, 0.025, "all rejected")
    assert r.n_connected == ph.n_connected_vertices and len(r.xyz32) == 0


def test_thresholds_hit_exactly(hip):
    """|d| == max_distance does not propagate, |d| == voxel_size is inside the surface box"""
    check_exact_thresholds(hip)


def test_draw_samples_edges(hip, oracle):
    """all-zero weights (every draw is index 0), one non-zero weight, n_res = 0"""
    layer_h, layer_o = Layer(hip, 0.1), Layer(oracle, 0.1)
    zero = np.zeros((40, 5), np.float32)
    one = zero.copy()
    one[23, 4] = 0.75
    for eng, layer in ((hip, layer_h), (oracle, layer_o)):
        assert np.all(check_sampler(eng, zero, layer, n_res=500) == 0)
        assert np.all(check_sampler(eng, one, layer, n_res=500) == 23)
        assert len(check_sampler(eng, zero, layer, n_res=0)) == 0
        assert len(check_sampler(eng, one, layer, n_res=0)) == 0
    draws = check_sampler(hip, unit_weight_points(), layer_h, n_res=2000)   # every draw lands exactly on a cumulative sum
    assert np.all(draws % 2 == 0) and len(np.unique(draws)) == 30
    rng = np.random.default_rng(9)
    many = np.zeros((5000, 5), np.float32)
    many[:, 4] = rng.choice(np.array([0.0, 9.5367431640625e-07, 1e-7, 0.3, 1.0, 77.25, -1.0, np.nan], np.float32), 5000)
    assert np.array_equal(check_sampler(hip, many, layer_h, n_res=3000), check_sampler(oracle, many, layer_o, n_res=3000))
