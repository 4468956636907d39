"""The HIP layer store (cox_layer.hip: upload, voxel merge, rigid resample, growth, clone / export, relevant voxels) against
the plain numpy reference of tests/layer_ref.py, bit for bit, through the engine-agnostic helpers of
tests/test_layer_ref_cpu.py; plus the launch-shape, index-range, growth and pinned-capacity edges only this engine has."""
import numpy as np
import pytest

import layer_cases
import layer_ref
import test_layer_ref_cpu as lr
from coxgraph_amd.capi import CoxError, Layer, RegPoints
from layer_ref import PATH_NEAREST, PATH_NONE, PATH_TRILINEAR

pytestmark = pytest.mark.gpu

POOL_EXHAUSTED, INDEX_RANGE = -4, -5
EMPTY = layer_ref.empty_layer()
F = np.float32


def f2u(x):
    return np.asarray(x, F).view(np.uint32)


def cube_blocks(lo=(0, 0, 0), n=2, skip=None):
    idx = np.array([[x, y, z] for z in range(n) for y in range(n) for x in range(n) if (x, y, z) != skip], np.int32)
    return idx + np.asarray(lo, np.int32)


def general_layer(seed, idx, voxel, weights=(0.5, 1.0, 37.25), p_zero=0.0):
    """smooth-free random content: distances N(0, 3 voxels), weights from `weights` (a share p_zero of them 0), random colours"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((len(idx), 4096)) * 3 * voxel
    w = rng.choice(np.array(weights, F), size=d.shape)
    w[rng.random(d.shape) < p_zero] = 0
    return idx, layer_cases.words(d, w, rng.integers(0, 2 ** 32, d.shape, dtype=np.uint64).astype(np.uint32))


def message(seed, n):
    """n distinct blocks around zero in shuffled order, every word random bits"""
    rng = np.random.default_rng(seed)
    box = np.array([[x, y, z] for z in range(-3, 3) for y in range(-3, 4) for x in range(-3, 4)], np.int32)
    return box[rng.permutation(len(box))[:n]], rng.integers(0, 2 ** 32, (n, 4096, 3), dtype=np.uint64).astype(np.uint32)


def merged(hip, A, T, B, va, vb=None, capacity=0):
    """B after merge_from(A, T) on the engine, the reference's B and its path codes"""
    vb = va if vb is None else vb
    la, lb = lr.build(hip, A, va), lr.build(hip, B, vb, capacity=capacity)
    lb.merge_from(la, T)
    a_ref, b_ref = layer_ref.upload_ref(EMPTY, *A, 0), layer_ref.upload_ref(EMPTY, *B, 0)
    want, path = layer_ref.merge_ref(a_ref, T, b_ref, va, vb)
    return lb, want, path


# ---- the seeded cases, the plane and the metamorphic checks ------------------------------------------------------
@pytest.mark.parametrize("seed", lr.SEEDS)
def test_layer_store_matches_reference(hip, seed):
    lr.check_case(hip, layer_cases.case(seed), f"seed {seed}")


@pytest.mark.parametrize("k", range(4))
def test_resample_reproduces_a_plane(hip, k):
    lr.check_plane(hip, layer_cases.PLANE_TRANSFORMS[k], f"transform {k}")


def test_whole_block_translation_is_a_shift(hip):
    lr.check_block_shift(hip)


@pytest.mark.parametrize("axis", range(3))
def test_half_turn_is_a_mirror(hip, axis):
    lr.check_half_turn(hip, axis)


@pytest.mark.parametrize("seed", [0, 8, 16])
def test_identity_transform_equals_no_transform(hip, seed):
    lr.check_identity_is_none(hip, seed)


# ---- upload: launch shapes, index range, bit transparency ---------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_upload_launch_shapes(hip, n):
    """k_upload_insert runs 256 threads per workgroup: one short, exact, one over; host and device-resident messages"""
    import torch
    idx, vox = message(n, n)
    want = layer_ref.upload_ref(EMPTY, idx, vox, 0)
    L = Layer(hip, 0.1, capacity_blocks=64)
    L.upload(idx, vox)
    lr.assert_same_layer(L.download(), want, f"upload {n}")
    assert L.n_blocks() == n
    t_idx, t_vox = torch.from_numpy(idx).cuda(), torch.from_numpy(vox.view(np.int32)).cuda()
    D = Layer(hip, 0.1, capacity_blocks=64)
    D.upload_dev(t_idx.data_ptr(), t_vox.data_ptr(), n)
    lr.assert_same_layer(D.download(), want, f"upload_dev {n}")
    o_idx = torch.full((n, 3), 7, dtype=torch.int32, device="cuda")
    o_vox = torch.zeros((n, 4096, 3), dtype=torch.int32, device="cuda")
    assert D.export_dev(o_idx.data_ptr(), o_vox.data_ptr(), n) == n
    lr.assert_same_layer((o_idx.cpu().numpy(), o_vox.cpu().numpy().view(np.uint32)), want, f"export_dev {n}")


def test_block_index_range(hip):
    m = (1 << 20) - 2
    idx = np.array([[m, -m, m], [-m, m, -m], [-m, -m, -m], [m, m, m], [0, 0, 0]], np.int32)
    _, vox = general_layer(3, idx, 0.1)
    L = Layer(hip, 0.1, capacity_blocks=64)
    L.upload(idx, vox)
    lr.assert_same_layer(L.download(), layer_ref.upload_ref(EMPTY, idx, vox, 0), "extreme indices")
    assert lr.check_relevant(L, 0.1, 0.0, 1e9) > 0
    for bad in ([m + 1, 0, 0], [0, m + 1, 0], [0, 0, m + 1], [0, -m - 2, 0]):
        with pytest.raises(CoxError) as e:
            Layer(hip, 0.1, capacity_blocks=64).upload(np.array([bad], np.int32), vox[:1])
        assert e.value.status == INDEX_RANGE, bad
        with pytest.raises(ValueError):
            layer_ref.upload_ref(EMPTY, np.array([bad], np.int32), vox[:1], 0)


def test_upload_is_bit_transparent(hip):
    """action 0 stores words, not floats: NaNs with payloads, infinities, -0.0 and denormals come back as they went in"""
    special = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00800000], np.uint32)
    rng = np.random.default_rng(9)
    idx = np.array([[-1, 0, 2], [0, 0, 0]], np.int32)
    vox = rng.integers(0, 2 ** 32, (2, 4096, 3), dtype=np.uint64).astype(np.uint32)
    vox[..., 0] = rng.choice(special, (2, 4096))
    vox[1, :, 1] = rng.choice(special, 4096)
    L = Layer(hip, 0.1, capacity_blocks=64)
    L.upload(idx, vox)
    lr.assert_same_layer(L.download(), layer_ref.upload_ref(EMPTY, idx, vox, 0), "special words")
    L.upload(idx[::-1], vox[::-1], action=2)
    lr.assert_same_layer(L.download(), layer_ref.upload_ref(EMPTY, idx, vox, 0), "special words, reset")


# ---- mergeVoxelAIntoVoxelB -------------------------------------------------------------------------------------
def merge_table():
    """One block whose voxels run through the (aw, bw) pairs that matter, with distances and colours around them"""
    rng = np.random.default_rng(21)
    pairs = np.array([(0, 0), (0.3, 0), (0, 0.3), (1e4, 1e-6), (1e-6, 1e4), (0.7, 0), (1, 1), (37.25, 0.5)], F)
    k = layer_cases.LIN % len(pairs)
    ad, bd = (rng.standard_normal(4096) * 0.3).astype(F), (rng.standard_normal(4096) * 0.3).astype(F)
    ac = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    bc = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    half = k == 6                           # equal weights, even bytes against odd bytes: every channel blends to x.5
    ac[half], bc[half] = ac[half] & 0xFEFEFEFE, bc[half] | 0x01010101
    a = np.stack([f2u(ad), f2u(pairs[k, 0]), ac], axis=1)[None]
    b = np.stack([f2u(bd), f2u(pairs[k, 1]), bc], axis=1)[None]
    return a, b, k


def test_merge_voxel_table(hip):
    a, b, k = merge_table()
    idx = np.array([[-1, 2, 0]], np.int32)
    ad, aw = a[0, :, 0].view(F), a[0, :, 1].view(F)
    fresh = np.isin(k, (1, 5))
    assert int(((ad[fresh] * aw[fresh]) / aw[fresh] != ad[fresh]).sum()) > 50      # a first observation is NOT copied bit for bit
    want = layer_ref.merge_voxels_ref(a, b)
    assert np.array_equal(want[0, k == 0], b[0, k == 0])     # no weight on either side: B's voxel stays, bits and all
    assert int((want[0, fresh, 0] != a[0, fresh, 0]).sum()) > 50
    by_wire = lr.build(hip, (idx, b), 0.1)
    by_wire.upload(idx, a, action=1)
    by_merge, la = lr.build(hip, (idx, b), 0.1), lr.build(hip, (idx, a), 0.1)
    by_merge.merge_from(la)
    lr.assert_same_layer(by_wire.download(), (idx, want), "action 1")
    lr.assert_same_layer(by_merge.download(), (idx, want), "merge_from")
    # the same message into a fresh block: b is the zero voxel
    fresh_layer = Layer(hip, 0.1, capacity_blocks=64)
    fresh_layer.upload(idx, a, action=1)
    lr.assert_same_layer(fresh_layer.download(), (idx, layer_ref.merge_voxels_ref(a, np.zeros_like(a))), "action 1 into a fresh block")


# ---- resample edges ------------------------------------------------------------------------------------------------
SMALL_T = layer_cases.pose([1, 0, 0, 0], [0.03, 0.02, 0.01])


def test_resample_one_unobserved_neighbour(hip):
    """one weight-0 voxel inside a block: exactly the eight cells that hold it fall back to the nearest voxel"""
    idx, vox = general_layer(31, cube_blocks((-1, -1, -1)), 0.1)
    hole = vox.copy()
    hole[0, 8 + 16 * (8 + 16 * 8), 1] = 0
    lb, want, path = merged(hip, (idx, hole), SMALL_T, EMPTY, 0.1)
    lr.assert_same_layer(lb.download(), want, "hole")
    full = layer_ref.resample_ref(idx, vox, 0.1, SMALL_T, 0.1)[2]
    whole = layer_ref.resample_ref(idx, hole, 0.1, SMALL_T, 0.1)[2]
    assert int(((full == PATH_TRILINEAR) & (whole == PATH_NEAREST)).sum()) == 8 and int((full != whole).sum()) == 8


@pytest.mark.parametrize("missing", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])
def test_resample_missing_neighbour_block(hip, missing):
    """a 2x2x2 cube without one block: the cells that reach into it fall back, in each of the seven directions"""
    lo = (-1, -1, -1)
    idx, vox = general_layer(32, cube_blocks(lo), 0.1)
    keep = ~np.all(idx == np.array(lo) + np.array(missing), axis=1)
    for sign in (1.0, -1.0):
        # shifted up, a position lies below its voxel centre and the cell begins in the lower neighbour (the missing block is
        # the cell's base block); shifted down, the cell runs upward into the missing block (the neighbour lookup fails)
        T = layer_cases.pose([1, 0, 0, 0], sign * SMALL_T[4:])
        lb, want, path = merged(hip, (idx[keep], vox[keep]), T, EMPTY, 0.1)
        lr.assert_same_layer(lb.download(), want, f"missing {missing}, shift {sign}")
        fc, _, fp = layer_ref.resample_ref(idx, vox, 0.1, T, 0.1)
        pc, _, pp = layer_ref.resample_ref(idx[keep], vox[keep], 0.1, T, 0.1)
        row = {tuple(c): j for j, c in enumerate(fc.tolist())}     # fewer input blocks give fewer candidates: align them
        fp = fp[[row[tuple(c)] for c in pc.tolist()]]
        fell_back = int(((fp == PATH_TRILINEAR) & (pp == PATH_NEAREST)).sum())
        # one face of 16 x 16 cells at the least, wherever the missing block has a neighbour on the side the cells come from
        reachable = any(m == (1 if sign < 0 else 0) for m in missing)
        assert fell_back >= (15 * 15 if reachable else 0), (missing, sign, fell_back)


def test_resample_centre_on_centre(hip):
    """a shift by whole voxels puts every output centre exactly on an input centre: the cell starts AT that voxel"""
    idx, vox = general_layer(33, cube_blocks((-1, 0, -2)), 0.125, p_zero=0.01)
    T = layer_cases.pose([1, 0, 0, 0], [3 * 0.125, -5 * 0.125, 16 * 0.125])
    lb, want, path = merged(hip, (idx, vox), T, general_layer(34, cube_blocks((-1, -1, -1)), 0.125), 0.125)
    lr.assert_same_layer(lb.download(), want, "centre on centre")
    assert (path == PATH_TRILINEAR).sum() > 20000 and (path == PATH_NEAREST).sum() > 1000


@pytest.mark.parametrize("voxel_b", [0.05, 0.2])
def test_resample_between_voxel_sizes(hip, voxel_b):
    A = general_layer(35, cube_blocks((-1, -1, 0)), 0.1, p_zero=0.005)
    T = layer_cases.pose(layer_cases.quat([0.1, -0.2, 1.0], 0.4), [0.21, -0.1, 0.05])
    B = general_layer(36, cube_blocks((0, 0, 0)), voxel_b)
    lb, want, path = merged(hip, A, T, B, 0.1, voxel_b)
    lr.assert_same_layer(lb.download(), want, f"0.1 into {voxel_b}")
    assert min((path == k).sum() for k in (PATH_TRILINEAR, PATH_NEAREST, PATH_NONE)) > 100
    for mw, md in lr.RELEVANT_CFGS:
        lr.check_relevant(lb, voxel_b, mw, md)


def test_resample_into_negative_indices(hip):
    A = general_layer(37, cube_blocks((0, 0, 0)), 0.1, p_zero=0.005)
    T = layer_cases.pose(layer_cases.quat([1.0, 1.0, 0.2], 2.0), [-20.0, -31.7, -12.3])
    lb, want, path = merged(hip, A, T, EMPTY, 0.1)
    assert len(want[0]) > 8 and np.all(want[0] < 0)
    lr.assert_same_layer(lb.download(), want, "negative indices")


def test_merge_of_an_empty_layer_and_of_a_layer_into_itself(hip):
    lr.check_empty_and_self(hip)


# ---- growth, clone ----------------------------------------------------------------------------------------------------
def test_reserve_and_rebuilt_table(hip):
    idx, vox = message(41, 60)
    vox = general_layer(41, idx, 0.1)[1]
    L = Layer(hip, 0.1, capacity_blocks=64)
    L.upload(idx, vox)
    want = layer_ref.upload_ref(EMPTY, idx, vox, 0)
    assert L.capacity() == 64
    L.reserve(200)
    assert L.capacity() >= 200
    lr.assert_same_layer(L.download(), want, "after reserve")
    L.upload(idx, vox, action=1)            # every key must be found in the rebuilt table: no block is added
    assert L.n_blocks() == 60
    lr.assert_same_layer(L.download(), layer_ref.upload_ref(want, idx, vox, 1), "merge after reserve")


def test_upload_grows_the_pool(hip):
    idx, _ = message(42, 65)
    vox = general_layer(42, idx, 0.1)[1]
    L = Layer(hip, 0.1, capacity_blocks=64)
    L.upload(idx[:10], vox[:10])
    L.upload(idx, vox, action=1)
    assert L.capacity() >= 128 and L.n_blocks() == 65
    want = layer_ref.upload_ref(layer_ref.upload_ref(EMPTY, idx[:10], vox[:10], 0), idx, vox, 1)
    lr.assert_same_layer(L.download(), want, "grown by upload")
    fresh = Layer(hip, 0.1, capacity_blocks=64)
    fresh.upload(idx, vox)
    assert fresh.capacity() >= 128
    lr.assert_same_layer(fresh.download(), layer_ref.upload_ref(EMPTY, idx, vox, 0), "65 into 64")


def test_merge_grows_the_pool(hip):
    A = general_layer(43, cube_blocks((-2, -2, -2), 4)[:48], 0.1, p_zero=0.005)
    B = general_layer(44, cube_blocks((-1, -1, -1)), 0.1)
    T = layer_cases.pose(layer_cases.quat([0.3, 0.1, 1.0], 0.6), [0.4, 0.1, -0.3])
    lb, want, _ = merged(hip, A, T, B, 0.1, capacity=64)
    assert len(want[0]) > 64 and lb.capacity() >= len(want[0])
    lr.assert_same_layer(lb.download(), want, "grown by merge")
    same, want_same, _ = merged(hip, general_layer(45, message(45, 70)[0], 0.1), None, B, 0.1, capacity=64)
    assert same.capacity() >= 78
    lr.assert_same_layer(same.download(), want_same, "grown by a merge on the same grid")


def test_clone_is_a_copy(hip):
    idx, _ = message(46, 70)
    vox = general_layer(46, idx, 0.1)[1]
    src = lr.build(hip, (idx, vox), 0.1, capacity=64)
    want = layer_ref.upload_ref(EMPTY, idx, vox, 0)
    clone = src.clone_to_device(0)
    lr.assert_same_layer(clone.download(), want, "clone")
    more = general_layer(47, idx[:40] + np.array([0, 0, 1], np.int32), 0.1)
    clone.upload(*more, action=1)
    lr.assert_same_layer(clone.download(), layer_ref.upload_ref(want, *more, 1), "clone after upload")
    lr.assert_same_layer(src.download(), want, "source after the clone's upload")


# ---- pinned capacity ----------------------------------------------------------------------------------------------------
def pinned_layer(hip):
    idx, _ = message(51, 60)
    B = general_layer(51, idx, 0.1)
    L = lr.build(hip, B, 0.1, capacity=64)
    L.set_auto_grow(0)
    assert L.capacity() == 64
    return L, layer_ref.upload_ref(EMPTY, *B, 0)


def outside_blocks(seed, n):
    """blocks that no message() holds"""
    return general_layer(seed, cube_blocks((10, 10, 10), 3)[:n], 0.1)


def test_pinned_upload_that_does_not_fit_leaves_the_layer(hip):
    L, want = pinned_layer(hip)
    for action in (0, 1):
        with pytest.raises(CoxError) as e:
            L.upload(*outside_blocks(52, 5), action=action)
        assert e.value.status == POOL_EXHAUSTED
        assert L.n_blocks() == 60           # raises on a sticky error word
        lr.assert_same_layer(L.download(), want, "refused upload")
    L.upload(*outside_blocks(52, 4), action=1)
    lr.assert_same_layer(L.download(), layer_ref.upload_ref(want, *outside_blocks(52, 4), 1), "upload that fits")


@pytest.mark.parametrize("with_transform", [False, True])
def test_pinned_merge_that_does_not_fit_leaves_the_layer(hip, with_transform):
    """the contract of the uploads holds for merges: COX_ERR_POOL_EXHAUSTED before anything is inserted, no partial merge,
    no key without storage, no error word left behind"""
    L, want = pinned_layer(hip)
    T = layer_cases.pose([1, 0, 0, 0], [0.03, 0.02, 0.01]) if with_transform else None
    big = lr.build(hip, outside_blocks(53, 5), 0.1)      # the small shift keeps every block where it is: 60 + 5 > 64
    with pytest.raises(CoxError) as e:
        L.merge_from(big, T)
    assert e.value.status == POOL_EXHAUSTED
    assert L.n_blocks() == 60 and L.capacity() == 64
    lr.assert_same_layer(L.download(), want, "refused merge")
    small = outside_blocks(54, 4)
    L.merge_from(lr.build(hip, small, 0.1))
    now = layer_ref.upload_ref(want, *small, 1)
    lr.assert_same_layer(L.download(), now, "merge that fits")
    assert L.n_blocks() == 64
    with pytest.raises(CoxError) as e:      # the bound is blocks held + blocks brought, as for the uploads: 64 + 2 > 64
        L.merge_from(lr.build(hip, (small[0][:2], small[1][:2]), 0.1), T)
    assert e.value.status == POOL_EXHAUSTED and L.n_blocks() == 64
    lr.assert_same_layer(L.download(), now, "refused merge into a full pool")


# ---- relevant voxels ----------------------------------------------------------------------------------------------------
def relevant_edge_layer():
    """min_w = 1, max_d = 0.3: a block with all 4096 voxels relevant, one with none (every voxel on or beyond a threshold: w == min_w,
    |d| == max_d on both sides, NaN distance, NaN weight), one whose relevant voxels sit on the round and wave boundaries of the
    compaction, one mixed"""
    rng = np.random.default_rng(61)
    idx = np.array([[-3, -1, -2], [-2, -1, -2], [-1, -5, -7], [-4, -4, -1]], np.int32)
    d = (rng.uniform(-0.29, 0.29, (4, 4096))).astype(F)
    w = np.full((4, 4096), 2.0, F)
    k = layer_cases.LIN % 6
    w[1, k == 0] = 1.0
    d[1, k == 1], d[1, k == 2] = F(0.3), F(-0.3)
    d[1, k == 3] = np.nan
    w[1, k == 4] = np.nan
    w[1, k == 5] = np.nextafter(F(1.0), F(0))
    w[2] = 1.0
    w[2, [255, 256, 511, 512, 4095]] = np.nextafter(F(1.0), F(2))
    r = rng.random(4096)
    w[3, r < 0.3], d[3, (r >= 0.3) & (r < 0.5)] = 1.0, F(0.3)
    d[3, (r >= 0.5) & (r < 0.6)] = np.nextafter(F(0.3), F(0))
    return idx, layer_cases.words(d, w, np.uint32(0))


def test_relevant_voxels_on_the_thresholds(hip):
    idx, vox = relevant_edge_layer()
    L = lr.build(hip, (idx, vox), 0.1, shuffle=1)
    want = layer_ref.relevant_points_ref(idx, vox, 0.1, 1.0, 0.3)
    per_block = [len(layer_ref.relevant_points_ref(idx[j:j + 1], vox[j:j + 1], 0.1, 1.0, 0.3)) for j in range(4)]
    assert per_block[0] == 4096 and per_block[1] == 0 and per_block[2] == 5 and 1000 < per_block[3] < 3500
    assert lr.check_relevant(L, 0.1, 1.0, 0.3) == len(want)
    got = RegPoints.from_layer(hip, L, 1.0, 0.3).download()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the five survivors of block 2, by hand: linear index -> centre
    five = got[got[:, 4] == np.nextafter(F(1.0), F(2))]
    lin = np.array([255, 256, 511, 512, 4095])
    by_hand = (np.array([-1, -5, -7]) * 16 + np.stack([lin % 16, (lin // 16) % 16, lin // 256], axis=1) + 0.5) * 0.1
    assert five.shape == (5, 5) and np.allclose(five[:, :3], by_hand, atol=2e-6)


@pytest.mark.parametrize("seed", [2, 11, 27])
def test_relevant_voxels_of_seeded_layers(hip, seed):
    c = layer_cases.case(seed)
    L = lr.build(hip, c["A"], c["voxel_a"], shuffle=seed)
    n = [lr.check_relevant(L, c["voxel_a"], mw, md) for mw, md in lr.RELEVANT_CFGS]
    want = layer_ref.relevant_points_ref(*c["A"], c["voxel_a"], 1e-6, 0.05)
    got = RegPoints.from_layer(hip, L, 1e-6, 0.05).download()
    assert n[1] > 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_relevant_voxels_of_an_empty_layer(hip):
    L = Layer(hip, 0.1, capacity_blocks=64)
    assert L.registration_points(1.0, 0.3).shape == (0, 5)
    assert RegPoints.from_layer(hip, L, 1.0, 0.3).n == 0
    L.upload(*general_layer(62, cube_blocks(), 0.1))
    assert L.registration_points(1e9, 0.3).shape == (0, 5)      # blocks, but nothing relevant
    assert RegPoints.from_layer(hip, L, 1e9, 0.3).n == 0
