"""The pinhole depth integrator on the GPU (cox_depthfuse.hip) against the float32 reference of
tests/cpp/depthfuse_reference.cpp fed the same inputs, BIT FOR BIT: the same pool order, the same words per block, the same five
counters.  Unless noted the shapes are the reference's own (48 x 36, 0.1 m voxels, dr.BASE)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depthfuse_ref as dr
import util
from coxgraph_amd import capi, synth
from coxgraph_amd.capi import CoxError, Integrator, Layer
from render_ref import voxel_centres

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# candidate counts at which the frame's scans take another path: exclusive_scan_u32's tile (cox_sort.hpp kScanTile); the scan of
# the tile sums works in chunks of 1024 tiles = 2^21 candidates, which is COX_DEPTHFUSE_MAX_CANDIDATES, so a frame never has two
SCAN_TILE = 2048
MAX_CANDIDATES = 1 << 21
ACROSS = 2600   # a count that leaves more than one z slab of the box beyond the first tile


@pytest.fixture(scope="module")
def ref32(tmp_path_factory):
    return dr.build(tmp_path_factory.mktemp("depthfuse_ref"))


@pytest.fixture(scope="module")
def frames():
    return dr.scene_frames(3)


def fuse(di, ref, T, depth, rgba=None, K=None, expect=0, max_blocks=-1):
    """one frame on both sides: same status, same counters"""
    if K is None:
        K = dr.scaled_intrinsics(depth.shape[1], depth.shape[0])
    rc, want = ref.integrate(T, depth, rgba, K, max_blocks=max_blocks)
    assert rc == expect
    try:
        di.integrate(T, depth, rgba, K)
        got_rc = 0
    except CoxError as e:
        got_rc = e.status
    assert got_rc == expect
    got = di.last_stats()
    assert {k: got[k] for k in dr.COUNTERS} == want, (got, want)
    return got


def same_layer(di, layer, ref):
    """bit for bit: pool order, then the words block by block"""
    di.sync()
    ridx, rvox = ref.pool()
    order = di.pool_order()
    assert order.shape == ridx.shape and np.array_equal(order, ridx), "pool order differs"
    idx, vox = layer.download()
    sidx, svox = dr.sort_blocks(ridx, rvox)
    assert np.array_equal(idx, sidx)
    bad = vox != svox
    assert not bad.any(), f"{int(bad.sum())} words differ in {int(bad.any((1, 2)).sum())} blocks"
    return idx, vox


def pair(hip, ref32, voxel=dr.VOXEL, capacity=0, **cfg):
    cfg = {**dr.BASE, **cfg}
    layer = Layer(hip, voxel, capacity_blocks=capacity)
    return layer, layer.depth_integrator(**cfg), ref32.layer(voxel, **cfg)


# ---- 1. the matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.matrix_cases(), ids=dr.case_id)
def test_matrix_bit_for_bit(hip, ref32, frames, case):
    cfg = dr.case_config(case)
    layer, di, ref = pair(hip, ref32, **cfg)
    ref64 = dr.Ref64(dr.VOXEL, **cfg) if case["scheme"] == 3 else None
    n_upd = 0
    for T, depth, rgba, K in frames:
        n_upd += fuse(di, ref, T, depth, rgba if case["colour"] else None, K)["n_updated_voxels"]
        if ref64 is not None:
            ref64.integrate(T, depth, rgba if case["colour"] else None, K)
    idx, vox = same_layer(di, layer, ref)
    assert len(idx) >= 8 and n_upd > 1000
    if ref64 is not None:
        rep = ref64.check(idx, vox, util.TOL)
        print(rep)
        assert rep["checked"] > 1000
        assert rep["ambiguous_fraction"] <= dr.MAX_AMBIGUOUS_FRACTION


# ---- 2. closed forms on the GPU layer ---------------------------------------------------------------------------------------------
Z0 = 2.0
T_AXIS = np.array([1, 0, 0, 0, 0.05, 0.05, 0.0], np.float32)  # camera axes = world axes, on a line of voxel centres
K_WIDE = np.array([12.0, 12.0, 23.5, 17.5], np.float32)       # a pixel is 8 cm wide at 1 m


def _fields(layer):
    idx, vox = layer.download()
    c = voxel_centres(idx, dr.VOXEL).astype(np.float64) - T_AXIS[4:].astype(np.float64)
    return idx, c, vox[..., 0].copy().view(np.float32).astype(np.float64), vox[..., 1].copy().view(np.float32).astype(np.float64)


@pytest.mark.parametrize("n", [1, 3])
def test_wall_axis_voxels_and_weights(hip, ref32, n):
    depth = np.full((dr.H, dr.W), Z0, np.float32)
    for const in (1, 0):
        layer, di, ref = pair(hip, ref32, use_const_weight=const, use_weight_dropoff=0)
        for _ in range(n):
            fuse(di, ref, T_AXIS, depth)
        same_layer(di, layer, ref)
        _, c, d, w = _fields(layer)
        axis = (np.abs(c[..., 0]) < 1e-6) & (np.abs(c[..., 1]) < 1e-6) & (c[..., 2] >= 0.3) & (c[..., 2] <= Z0 + 0.3)
        assert axis.sum() >= 20 and np.all(w[axis] > 0)
        assert np.max(np.abs(d[axis] - np.clip(Z0 - c[..., 2][axis], -0.3, 0.3))) <= util.TOL
        assert not np.any(w[c[..., 2] > Z0 + 0.3 + 1e-6] > 0)
        assert (w > 0).sum() > 1000
        assert np.max(np.abs(w[w > 0] - (n if const else n / Z0 ** 2))) <= util.TOL


def test_step_edge_under_schemes_2_and_3(hip, ref32):
    edge = 20  # columns < edge see 1 m, the others 2 m: a gap of 1 m > adaptive_gap_m
    depth = np.full((dr.H, dr.W), 2.0, np.float32)
    depth[:, :edge] = 1.0
    for scheme in (2, 3):
        layer, di, ref = pair(hip, ref32, interpolation_scheme=scheme, use_const_weight=1, use_weight_dropoff=0)
        fuse(di, ref, T_AXIS, depth, K=K_WIDE)
        same_layer(di, layer, ref)
        _, c, d, w = _fields(layer)
        Kd = K_WIDE.astype(np.float64)
        u, v = Kd[0] * c[..., 0] / c[..., 2] + Kd[2], Kd[1] * c[..., 1] / c[..., 2] + Kd[3]
        du = u - (edge - 1)
        straddle = (du > 0.2) & (du < 0.8) & (v > 1) & (v < dr.H - 2) & (c[..., 2] > 0.8) & (c[..., 2] < 1.2)
        assert straddle.sum() >= 5 and np.all(w[straddle] > 0)
        D = np.ones_like(u) if scheme == 3 else 1.0 + du   # the near side; the mean
        want = np.clip((D - c[..., 2]) * np.linalg.norm(c, axis=-1) / c[..., 2], -0.3, 0.3)
        assert np.max(np.abs(d[straddle] - want[straddle])) <= util.TOL


# ---- 3. image edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", [(1, 1), (2, 2), (1, 5), (47, 35)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scheme", [0, 3])
def test_small_and_odd_images(hip, ref32, wh, scheme):
    w, h = wh
    K = dr.scaled_intrinsics(w, h)
    layer, di, ref = pair(hip, ref32, interpolation_scheme=scheme)
    for i in range(2):
        _, T = dr.look_at([0.13 + 0.07 * i, -0.21, 0.17], [2.2, 0.1 * i, 0.05])
        st = fuse(di, ref, T, dr.scene_depth(T, w, h, K), dr.scene_colors(w, h), K)
    assert st["n_valid_pixels"] == w * h
    idx, _ = same_layer(di, layer, ref)
    assert len(idx) >= 1


@pytest.mark.parametrize("colours", [(1, 1, 1), (0, 0, 0), (0, 1, 0)], ids=["rgba", "no-rgba", "rgba-for-the-large-one"])
def test_image_sizes_small_large_small_on_one_integrator(hip, ref32, colours):
    """The host entry keeps one staging buffer for depth and one for colour, which grow with the image and never shrink:
    8 x 8, 64 x 48 and 8 x 8 through one integrator."""
    layer, di, ref = pair(hip, ref32)
    for i, ((w, h), colour) in enumerate(zip([(8, 8), (64, 48), (8, 8)], colours)):
        K = dr.scaled_intrinsics(w, h)
        _, T = dr.look_at([0.13 + 0.07 * i, -0.21, 0.17], [2.2, 0.1 * i, 0.05])
        st = fuse(di, ref, T, dr.scene_depth(T, w, h, K), dr.scene_colors(w, h) if colour else None, K)
        assert st["n_valid_pixels"] > 0 and st["n_updated_voxels"] > 0
    idx, _ = same_layer(di, layer, ref)
    assert len(idx) >= 1


@pytest.mark.parametrize("K", [[39.0, 39.0, 80.0, 17.5], [39.0, 39.0, 23.5, -30.0], [39.0, 39.0, -15.0, 60.0]], ids=["right", "above", "corner"])
def test_principal_point_outside_the_image(hip, ref32, K):
    K = np.array(K, np.float32)
    layer, di, ref = pair(hip, ref32)
    T = dr.scene_frames(1)[0][0]
    st = fuse(di, ref, T, np.full((dr.H, dr.W), 1.7, np.float32), dr.scene_colors(dr.W, dr.H), K)
    assert st["n_updated_voxels"] > 100
    same_layer(di, layer, ref)


def test_all_nan_image_and_inverted_limits(hip, ref32, frames):
    T, depth, rgba, K = frames[0]
    layer, di, ref = pair(hip, ref32)
    st = fuse(di, ref, T, np.full((dr.H, dr.W), np.nan, np.float32), rgba, K)
    assert st["n_valid_pixels"] == 0 and st["n_touched_blocks"] == 0 and layer.n_blocks() == 0
    assert len(di.pool_order()) == 0
    layer2, di2, ref2 = pair(hip, ref32, min_depth_m=2.0, max_depth_m=1.0)  # min > max: nothing happens
    st = fuse(di2, ref2, T, depth, rgba, K)
    assert st["n_valid_pixels"] == int((np.isfinite(depth) & (depth > 0)).sum()) and st["n_updated_voxels"] == 0 and layer2.n_blocks() == 0


@pytest.mark.parametrize("scheme", [0, 1, 2, 3])
def test_invalid_pixels_scattered_over_a_valid_image(hip, ref32, frames, scheme):
    layer, di, ref = pair(hip, ref32, interpolation_scheme=scheme)
    rng = np.random.default_rng(17 + scheme)
    for T, depth, rgba, K in frames[:2]:
        depth = depth.copy()
        bad = rng.random(depth.shape)
        depth[bad < 0.05] = np.inf
        depth[(bad >= 0.05) & (bad < 0.10)] = 0.0
        depth[(bad >= 0.10) & (bad < 0.15)] = -1.5
        depth[(bad >= 0.15) & (bad < 0.20)] = np.nan
        depth[(bad >= 0.20) & (bad < 0.22)] = -np.inf
        st = fuse(di, ref, T, depth, rgba, K)
        assert st["n_valid_pixels"] == int((np.isfinite(depth) & (depth > 0)).sum())
    idx, _ = same_layer(di, layer, ref)
    assert len(idx) >= 8


# ---- 4. poses ---------------------------------------------------------------------------------------------------------------------
AXES = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1)}


def _depth_of(T, rng):
    """a bumpy surface 1.5 .. 2.1 m in front of wherever the camera looks (the rule does not care what the image shows)"""
    uu, vv = np.meshgrid(np.arange(dr.W), np.arange(dr.H))
    return (1.8 + 0.3 * np.sin(0.3 * uu + 0.1) * np.cos(0.25 * vv) + 0.002 * rng.random((dr.H, dr.W))).astype(np.float32)


@pytest.mark.parametrize("axis", list(AXES))
def test_optical_axis_along_the_world_axes(hip, ref32, axis):
    rng = np.random.default_rng(5)
    origin = np.array([0.13, -0.21, 0.17])
    _, T = dr.look_at(origin, origin + np.array(AXES[axis], np.float64))
    layer, di, ref = pair(hip, ref32)
    fuse(di, ref, T, _depth_of(T, rng), dr.scene_colors(dr.W, dr.H))
    origin2 = origin + 0.07
    _, T2 = dr.look_at(origin2, origin2 + np.array(AXES[axis], np.float64))
    fuse(di, ref, T2, _depth_of(T2, rng), dr.scene_colors(dr.W, dr.H))
    idx, _ = same_layer(di, layer, ref)
    assert len(idx) >= 8


def test_generic_rotation_and_negative_coordinates(hip, ref32):
    rng = np.random.default_rng(6)
    q = np.array([0.61, -0.37, 0.52, 0.47])
    T = np.concatenate([q / np.linalg.norm(q), [0.4, -0.3, 0.2]]).astype(np.float32)
    layer, di, ref = pair(hip, ref32)
    fuse(di, ref, T, _depth_of(T, rng), dr.scene_colors(dr.W, dr.H))
    same_layer(di, layer, ref)
    # a camera at negative coordinates whose frustum straddles block index 0 on all three axes
    _, T = dr.look_at([-0.9, -0.8, -0.7], [1.0, 0.9, 0.8])
    layer, di, ref = pair(hip, ref32)
    fuse(di, ref, T, _depth_of(T, rng), dr.scene_colors(dr.W, dr.H))
    idx, _ = same_layer(di, layer, ref)
    assert np.all(idx.min(0) < 0) and np.all(idx.max(0) >= 0)


# ---- 5. candidate counts across the scan's tile edges -----------------------------------------------------------------------------
def test_many_candidates_at_fine_voxels(hip, ref32, frames):
    """0.05 m voxels and 5 m of depth: at this pose and image that is a box of 9 x 9 x 8 = 648 candidates, well inside one scan tile;
    the larger counts are the tests' below"""
    T, depth, rgba, K = frames[0]
    layer, di, ref = pair(hip, ref32, voxel=0.05, max_depth_m=5.0)
    st = fuse(di, ref, T, depth, rgba, K)
    print(st)
    assert st["n_touched_blocks"] > 20 and st["n_candidate_blocks"] > 300
    same_layer(di, layer, ref)


def _box(hip, voxel, T, w, h, K, **cfg):
    """(lo, dims) of a frame's candidate box: cox_selftest_depthfuse_box, a host computation"""
    c = capi.depthfuse_config(hip, **cfg)
    T, K = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(K, np.float32)
    lo, dims = np.zeros(3, np.int32), np.zeros(3, np.uint32)
    assert hip.fn("selftest_depthfuse_box")(C.c_float(voxel), C.byref(c), capi._fp(T), C.c_int(w), C.c_int(h), capi._fp(K), capi._fp(lo), capi._fp(dims)) == 0
    return lo.astype(np.int64), dims.astype(np.int64)


def _candidate_index(blocks, lo, dims):
    """the candidate a block of the box is: x fastest"""
    rel = np.asarray(blocks, np.int64).reshape(-1, 3) - lo
    assert np.all((rel >= 0) & (rel < dims))
    return rel[:, 0] + dims[0] * (rel[:, 1] + dims[1] * rel[:, 2])


def _tile_edge_frames(hip):
    """(max_depth, candidate count) of three frames of frame 0's pose at 0.05 m: the closest its box comes to the scan tile from below
    and from above, and the first count past ACROSS.  The last z slab of a box is its widening and holds no block the rule can reach,
    so in the frame just above the tile every flag of the second tile is 0: it pins the scans' grid sizes and the tail tile's bounds,
    and only the third frame has touched and new blocks on the far side of the tile edge.  (Every multiple of the tile is the same
    edge of the same code; the reference walks ten times the candidates.)"""
    T, _, _, K = dr.scene_frames(1)[0]
    counts = {}
    for md in np.arange(3.0, 16.0, 0.02):
        _, dims = _box(hip, 0.05, T, dr.W, dr.H, K, **dict(dr.BASE, max_depth_m=float(md)))
        counts.setdefault(int(np.prod(dims)), float(md))
    below, above = max(n for n in counts if n <= SCAN_TILE), min(n for n in counts if n > SCAN_TILE)
    across = min(n for n in counts if n >= ACROSS)
    return [(counts[below], below), (counts[above], above), (counts[across], across)]


@pytest.mark.parametrize("k", range(2), ids=["below-2048", "above-2048"])
def test_candidate_counts_on_each_side_of_a_scan_tile(hip, ref32, frames, k):
    md, n = _tile_edge_frames(hip)[k]
    assert (n <= SCAN_TILE) == (k == 0) and abs(n - SCAN_TILE) < SCAN_TILE // 4, n
    T, _, rgba, K = frames[0]
    depth = np.full((dr.H, dr.W), 100.0, np.float32)   # nothing in the way: the frame carves, and so touches, blocks all over the box
    layer, di, ref = pair(hip, ref32, voxel=0.05, max_depth_m=md)
    st = fuse(di, ref, T, depth, rgba, K)
    assert st["n_candidate_blocks"] == n and st["n_touched_blocks"] > n // 8
    print(f"max_depth {md:.2f}: {n} candidates, {st['n_touched_blocks']} touched")
    order = same_layer(di, layer, ref)[0]
    # a second frame on the full pool: every touched block exists, none is new
    st = fuse(di, ref, T, depth, None, K)
    assert st["n_new_blocks"] == 0 and st["n_touched_blocks"] == len(order)
    same_layer(di, layer, ref)


def test_touched_and_new_blocks_on_both_sides_of_a_scan_tile_edge(hip, ref32, frames):
    """A frame whose second scan tile is not empty.  The pool starts with a seeded third of the box's blocks, holding seeded words
    (uploaded; the reference starts from the same arrays in the pool's order); then one frame with nothing in the way touches every
    block the frustum reaches.  Existing and new blocks alternate all over the box and on both sides of candidate SCAN_TILE, so
    the two scans differ, both carry a tile offset that is not 0, and the compacted list, the slots nb0 + rank and the pool
    lookups of the second tile all show in the pool order and the words.  (One frame: the reference takes 3 s for it.)"""
    md, n = _tile_edge_frames(hip)[2]
    assert ACROSS <= n < ACROSS + SCAN_TILE // 4, n
    T, _, rgba, K = frames[0]
    cfg = dict(dr.BASE, max_depth_m=md)
    lo, dims = _box(hip, 0.05, T, dr.W, dr.H, K, **cfg)
    assert int(np.prod(dims)) == n and n - SCAN_TILE > 2 * dims[0] * dims[1]   # the last slab is the widening and stays empty
    rng = np.random.default_rng(23)
    seed = np.sort(rng.choice(n, n // 3, replace=False))
    idx0 = np.stack([lo[0] + seed % dims[0], lo[1] + (seed // dims[0]) % dims[1], lo[2] + seed // (dims[0] * dims[1])], 1).astype(np.int32)
    vox0 = np.zeros((len(idx0), 4096, 3), np.uint32)
    vox0[..., 0] = rng.uniform(-0.3, 0.3, vox0.shape[:2]).astype(np.float32).view(np.uint32)
    vox0[..., 1] = (rng.uniform(0.0, 2.0, vox0.shape[:2]) * (rng.random(vox0.shape[:2]) < 0.7)).astype(np.float32).view(np.uint32)
    vox0[..., 2] = rng.integers(0, 1 << 32, vox0.shape[:2], dtype=np.uint64).astype(np.uint32)
    layer = Layer(hip, 0.05)
    layer.upload(idx0, vox0)
    di = layer.depth_integrator(**cfg)
    order0 = di.pool_order()
    pos = {tuple(b): i for i, b in enumerate(idx0)}
    vox0 = vox0[[pos[tuple(b)] for b in order0]]
    n_old = len(order0)
    assert n_old == len(idx0)
    ref = ref32.layer(0.05, order0, vox0, **cfg)
    st = fuse(di, ref, T, np.full((dr.H, dr.W), 100.0, np.float32), rgba, K)
    same_layer(di, layer, ref)
    order, vox = ref.pool()                        # == the GPU's, bit for bit
    assert st["n_candidate_blocks"] == n and len(order) == n_old + st["n_new_blocks"] and np.array_equal(order[:n_old], order0)
    cand = _candidate_index(order, lo, dims)
    old = cand[:n_old][(vox[:n_old] != vox0).any((1, 2))]   # existing blocks the frame wrote to: touched
    new = cand[n_old:]                                      # the pool's tail: touched and new
    print(f"max_depth {md:.2f}: {n} candidates; before / beyond candidate {SCAN_TILE}: touched existing blocks {(old < SCAN_TILE).sum()} / "
          f"{(old >= SCAN_TILE).sum()}, new {(new < SCAN_TILE).sum()} / {(new >= SCAN_TILE).sum()}; {st['n_touched_blocks']} touched")
    for side in (old, new):
        assert (side < SCAN_TILE).sum() >= 8 and (side >= SCAN_TILE).sum() >= 8
    assert len(old) + len(new) <= st["n_touched_blocks"]
    assert np.all(np.diff(new) > 0)                # step 9: ascending key is ascending candidate


def test_a_box_above_the_cap_is_refused(hip, ref32, frames):
    T, depth, rgba, K = frames[0]
    layer = Layer(hip, 0.01)
    ok = layer.depth_integrator(**dict(dr.BASE, max_depth_m=1.0))
    ok.integrate(T, depth, rgba, K)
    ok.sync()
    before = (ok.pool_order(),) + layer.download()
    di = layer.depth_integrator(**dict(dr.BASE, max_depth_m=200.0))
    with pytest.raises(CoxError) as e:
        di.integrate(T, depth, rgba, K)
    assert e.value.status == -1
    assert all(v == 0 for k, v in di.last_stats().items() if k != "kernel_ms")
    after = (ok.pool_order(),) + layer.download()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- 6. pool edges ----------------------------------------------------------------------------------------------------------------
def _two_views():
    K = dr.scaled_intrinsics(dr.W, dr.H)
    out = []
    for origin, target in (([0.13, -0.21, 0.17], [2.2, 0.0, 0.05]), ([0.2, 0.4, 0.3], [1.0, 2.2, 0.4])):
        _, T = dr.look_at(origin, target)
        out.append((T, dr.scene_depth(T, dr.W, dr.H, K), dr.scene_colors(dr.W, dr.H), K))
    return out


def test_pool_exactly_full_and_one_block_short(hip, ref32):
    views = _two_views()
    probe = ref32.layer(dr.VOXEL, **dr.BASE)
    n0 = probe.integrate(*views[0])[1]["n_new_blocks"]
    n1 = probe.integrate(*views[1])[1]["n_new_blocks"]
    assert n0 > 0 and n1 > 1
    # capacity exactly n_blocks + n_new: fine
    layer, di, ref = pair(hip, ref32, capacity=n0 + n1)
    layer.set_auto_grow(False)
    assert layer.capacity() == n0 + n1
    fuse(di, ref, *views[0])
    fuse(di, ref, *views[1], max_blocks=n0 + n1)
    same_layer(di, layer, ref)
    assert layer.n_blocks() == n0 + n1 == layer.capacity()
    # one block less: refused whole, the layer as it was
    layer, di, ref = pair(hip, ref32, capacity=n0 + n1 - 1)
    layer.set_auto_grow(False)
    fuse(di, ref, *views[0])
    before = (di.pool_order(),) + layer.download()
    st = fuse(di, ref, *views[1], expect=-4, max_blocks=n0 + n1 - 1)
    assert all(v == 0 for k, v in st.items() if k != "kernel_ms")
    after = (di.pool_order(),) + layer.download()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and layer.n_blocks() == n0
    same_layer(di, layer, ref)
    layer.reserve(n0 + n1 + 3)   # room: the next frame gives the reference's result
    fuse(di, ref, *views[1])
    same_layer(di, layer, ref)


def test_auto_grow_from_one_block_gives_the_same_pool(hip, ref32, frames):
    small, di_s, ref = pair(hip, ref32, capacity=1)
    large, di_l, _ = pair(hip, ref32, capacity=4096)
    for T, depth, rgba, K in frames:
        fuse(di_s, ref, T, depth, rgba, K)
        di_l.integrate(T, depth, rgba, K)
    same_layer(di_s, small, ref)
    same_layer(di_l, large, ref)
    assert small.capacity() >= small.n_blocks() > 1


# ---- 7. / 8. other writers on the layer -------------------------------------------------------------------------------------------
def _points(depth, K):
    """the frame's pixels as a point cloud in the camera frame (what a ray caster is handed)"""
    h, w = depth.shape
    K = np.asarray(K, np.float32)
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    pts = np.stack([depth * ((uu - K[2]) / K[0]), depth * ((vv - K[3]) / K[1]), depth], -1).reshape(-1, 3).astype(np.float32)
    keep = np.isfinite(depth.reshape(-1)) & (depth.reshape(-1) > 0)
    return np.ascontiguousarray(pts[keep]), np.ascontiguousarray(dr.scene_colors(w, h).reshape(-1, 4)[keep])


def _merged_frame(eng, layer, T, depth, K):
    cfg = eng.default_config(**synth.integrator_overrides(dr.VOXEL))
    integ = Integrator(eng, layer, cfg, "merged")
    integ.integrate_points(T, *_points(depth, K))
    return integ


@pytest.mark.parametrize("colour", [1, 0], ids=["rgba", "no-rgba"])
def test_prefilled_layer(hip, oracle, ref32, frames, colour):
    T0, depth0, _, K0 = frames[0]
    olayer = Layer(oracle, dr.VOXEL)
    _merged_frame(oracle, olayer, T0, depth0, K0).sync()
    idx, vox = olayer.download()
    assert len(idx) >= 8
    layer = Layer(hip, dr.VOXEL)
    layer.upload(idx, vox)
    di = layer.depth_integrator(**dr.BASE)
    order = di.pool_order()
    pos = {tuple(b): i for i, b in enumerate(idx)}
    perm = np.array([pos[tuple(b)] for b in order])
    assert sorted(perm) == list(range(len(idx)))
    ref = ref32.layer(dr.VOXEL, order, vox[perm], **dr.BASE)
    for T, depth, rgba, K in frames[1:]:
        fuse(di, ref, T, depth, rgba if colour else None, K)
    gidx, gvox = same_layer(di, layer, ref)
    if not colour:   # every colour word is as uploaded
        gpos = {tuple(b): i for i, b in enumerate(gidx)}
        assert all(np.array_equal(gvox[gpos[tuple(b)], :, 2], vox[i, :, 2]) for i, b in enumerate(idx))
        assert not gvox[[i for i, b in enumerate(gidx) if tuple(b) not in pos], :, 2].any()


def test_shared_layer_in_call_order(hip, oracle, ref32, frames):
    """depth fusion, a merged frame, depth fusion on one layer with no sync in between == Ref32 -> oracle merged -> Ref32"""
    (Ta, da, ca, Ka), (Tb, db, _, Kb), (Tc, dc, cc, Kc) = frames
    layer = Layer(hip, dr.VOXEL)
    di = layer.depth_integrator(**dr.BASE)
    di.integrate(Ta, da, ca, Ka)
    merged = _merged_frame(hip, layer, Tb, db, Kb)
    di.integrate(Tc, dc, cc, Kc)
    di.sync()
    merged.sync()
    # the composition on the CPU
    ra = ref32.layer(dr.VOXEL, **dr.BASE)
    assert ra.integrate(Ta, da, ca, Ka)[0] == 0
    olayer = Layer(oracle, dr.VOXEL)
    olayer.upload(*ra.download())
    _merged_frame(oracle, olayer, Tb, db, Kb).sync()
    rc = ref32.layer(dr.VOXEL, *olayer.download(), **dr.BASE)
    assert rc.integrate(Tc, dc, cc, Kc)[0] == 0
    rep = util.compare_layers(layer, rc)
    print(rep)
    assert rep["blocks"] >= 8
    assert rep["bitexact_d"] and rep["bitexact_w"] and rep["n_diff_color"] == 0   # both halves of the composition are exact
    # the layer is an ordinary layer for the readers
    esdf = layer.esdf_integrator(max_distance_m=1.0)
    assert esdf.update()["n_blocks"] == rep["blocks"]
    esdf.close()
    out = layer.render(Ta, dr.W, dr.H, Ka)
    assert (out["status"] & capi.R_HIT).sum() > dr.W * dr.H // 4


# ---- 9. render -> fuse on the device ----------------------------------------------------------------------------------------------
def test_render_then_fuse_without_a_host_copy(hip, ref32, frames):
    import torch
    T, depth, rgba, K = frames[0]
    first = Layer(hip, dr.VOXEL)
    d1 = first.depth_integrator(**dr.BASE)
    for f in frames:
        d1.integrate(*f)
    d1.sync()
    T2 = frames[1][0]
    image = torch.full((dr.H, dr.W), -7.0, dtype=torch.float32, device="cuda")
    first.render_dev(T2, dr.W, dr.H, K, depth=image)          # on the null stream, not waited for
    second, d2, ref = pair(hip, ref32)
    d2.integrate_dev(T2, image, None, dr.W, dr.H, K)            # ... and the frame orders behind it
    d2.sync()
    host = image.cpu().numpy()
    assert np.isfinite(host).sum() > dr.W * dr.H // 4 and not np.any(host == -7.0)
    rc, want = ref.integrate(T2, host, None, K)
    assert rc == 0
    got = d2.last_stats()
    assert {k: got[k] for k in dr.COUNTERS} == want
    idx, _ = same_layer(d2, second, ref)
    assert len(idx) >= 4


# ---- 10. saturation, determinism, range -------------------------------------------------------------------------------------------
def test_weights_saturate_at_max_weight(hip, ref32, frames):
    layer, di, ref = pair(hip, ref32, max_weight=2.0, use_const_weight=1, use_weight_dropoff=0)
    for i in range(4):
        fuse(di, ref, *frames[i % 3])
    _, vox = same_layer(di, layer, ref)
    w = vox[..., 1].copy().view(np.float32)
    assert w.max() == 2.0 and (w == 2.0).sum() > 1000


def test_weights_below_epsilon_write_nothing_and_allocate_nothing(hip, ref32, frames):
    """step 8's decision: 1 / D^2 of a surface 2 km away is below 1e-6, so such a frame writes only where a weight is stored already:
    nothing on an empty layer, and on a fused one the blocks behind the wall stay unallocated"""
    T, depth, rgba, K = frames[0]
    far = np.full((dr.H, dr.W), 2000.0, np.float32)
    layer, di, ref = pair(hip, ref32, use_const_weight=0, use_weight_dropoff=0)
    st = fuse(di, ref, T, far, rgba, K)
    assert st["n_valid_pixels"] == dr.W * dr.H and st["n_touched_blocks"] == 0 and layer.n_blocks() == 0
    st = fuse(di, ref, T, np.full((dr.H, dr.W), 1.2, np.float32), rgba, K)   # a wall at 1.2 m: nothing behind 1.5 m is observed
    n = st["n_new_blocks"]
    assert n >= 4
    st = fuse(di, ref, T, far, rgba, K)                                        # carves what is stored, and only that
    assert st["n_new_blocks"] == 0 and 0 < st["n_touched_blocks"] <= n and st["n_updated_voxels"] > 500
    idx, _ = same_layer(di, layer, ref)
    assert len(idx) == n
    # ... while weights of 1 do reach the free space behind it
    layer, di, ref = pair(hip, ref32, use_const_weight=1, use_weight_dropoff=0)
    fuse(di, ref, T, np.full((dr.H, dr.W), 1.2, np.float32), rgba, K)
    assert fuse(di, ref, T, far, rgba, K)["n_new_blocks"] > 0
    same_layer(di, layer, ref)


def test_the_same_calls_give_the_same_pool(hip, frames):
    got = []
    for _ in range(2):
        layer = Layer(hip, dr.VOXEL)
        di = layer.depth_integrator(**dr.BASE)
        for f in frames:
            di.integrate(*f)
        di.sync()
        order = di.pool_order()
        idx, vox = layer.download()
        got.append((order, idx, vox))
    assert all(np.array_equal(a, b) for a, b in zip(*got))


def test_a_pose_near_the_index_range_is_refused(hip, frames):
    T, depth, rgba, K = frames[0]
    layer = Layer(hip, dr.VOXEL)
    di = layer.depth_integrator(**dr.BASE)
    di.integrate(T, depth, rgba, K)
    di.sync()
    before = (di.pool_order(),) + layer.download()
    far = np.array(T, np.float32)
    far[4] = np.float32(16 * dr.VOXEL * (2 ** 20 - 1))
    with pytest.raises(CoxError) as e:
        di.integrate(far, depth, rgba, K)
    assert e.value.status == -5
    di.sync()
    after = (di.pool_order(),) + layer.download()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_invalid_configurations_are_refused(hip):
    layer = Layer(hip, dr.VOXEL)
    for cfg in (dict(truncation_distance=dr.VOXEL), dict(interpolation_scheme=4), dict(interpolation_scheme=-1), dict(min_depth_m=0.0), dict(max_depth_m=np.inf),
                dict(max_depth_m=np.nan), dict(truncation_distance=-0.3)):
        with pytest.raises(CoxError) as e:
            layer.depth_integrator(**{**dr.BASE, **cfg})
        assert e.value.status == -1, cfg
    di = layer.depth_integrator(**dr.BASE)
    T, depth, rgba, K = dr.scene_frames(1)[0]
    for bad_K in ([0.0, 39, 23.5, 17.5], [39, -1.0, 23.5, 17.5], [np.nan, 39, 23.5, 17.5], [39, 39, np.inf, 17.5]):
        with pytest.raises(CoxError) as e:
            di.integrate(T, depth, rgba, np.array(bad_K, np.float32))
        assert e.value.status == -1, bad_K
    assert layer.n_blocks() == 0


# ---- 11. C++ ----------------------------------------------------------------------------------------------------------------------
def test_cpp_depth_image_integrator_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "depthfuse_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "depthfuse_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
