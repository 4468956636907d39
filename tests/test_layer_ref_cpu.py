"""The layer store of the CPU oracle (upload, voxel merge, rigid resample, relevant voxels) held to the plain numpy
reference of tests/layer_ref.py, over the seeded cases of tests/layer_cases.py.  The check_* helpers are engine-agnostic:
tests/test_gpu_layer.py runs them on the HIP engine.

Bars: every comparison with layer_ref is bit for bit (block set, block order, distance, weight and colour words).  The
plane check rests on neither engine nor on layer_ref's arithmetic; its bound is stated at check_plane().  Per case the tests
print what they compared (run with -s)."""
import numpy as np
import pytest

import layer_cases
import layer_ref
from coxgraph_amd.capi import CoxError, Layer
from layer_ref import PATH_NEAREST, PATH_NONE, PATH_TRILINEAR

SEEDS = list(range(32))
RELEVANT_CFGS = ((1.0, 0.3), (0.0, 1e9), (1e-6, 0.05))
# check_plane(): the largest |d - plane| of layer_ref itself on its trilinear path over the four transforms (float64 plane,
# float64 positions), measured on the CPU and rounded up, and the bound the engines are held to: four times that
PLANE_REF_ERR = 1.39e-6
PLANE_BOUND = 4 * PLANE_REF_ERR
PLANE_MIN_TRILINEAR = 0.9


def build(eng, layer, voxel, capacity=0, shuffle=None):
    idx, vox = layer
    L = Layer(eng, voxel, capacity_blocks=capacity)
    if len(idx):
        p = np.arange(len(idx)) if shuffle is None else np.random.default_rng(shuffle).permutation(len(idx))
        L.upload(idx[p], vox[p])
    return L


def assert_same_layer(got, want, name=""):
    (gi, gv), (wi, wv) = got, want
    assert np.array_equal(gi, wi), (name, "block sets differ", len(gi), len(wi))
    bad = gv != wv
    assert not bad.any(), (name, "mismatching words d/w/colour", int(bad[..., 0].sum()), int(bad[..., 1].sum()), int(bad[..., 2].sum()),
                           "first at", tuple(int(v) for v in np.argwhere(bad)[0]))


def check_relevant(layer, voxel, min_w, max_d, name=""):
    idx, vox = layer.download()
    got = layer.registration_points(min_w, max_d)
    want = layer_ref.relevant_points_ref(idx, vox, voxel, min_w, max_d)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    return len(want)


def check_case(eng, c, name=""):
    """upload (actions 0, 1, 2), merge with or without resample and the relevant voxels of the result against layer_ref"""
    va, vb, A, T, B0 = c["voxel_a"], c["voxel_b"], c["A"], c["T"], c["B"]
    empty = layer_ref.empty_layer()
    la = build(eng, A, va, shuffle=c["meta"]["seed"])
    a_ref = layer_ref.upload_ref(empty, *A, 0)
    assert_same_layer(la.download(), a_ref, name + " upload")
    lb = build(eng, B0, vb, shuffle=c["meta"]["seed"] + 1)
    b_ref = layer_ref.upload_ref(empty, *B0, 0)
    assert_same_layer(lb.download(), b_ref, name + " upload B")
    if va == vb:                            # the wire merge of the same message, then a reset
        lc = build(eng, B0, vb)
        lc.upload(*A, action=1)
        assert_same_layer(lc.download(), layer_ref.upload_ref(b_ref, *A, 1), name + " action 1")
        lc.upload(*A, action=2)
        assert_same_layer(lc.download(), a_ref, name + " action 2")
    lb.merge_from(la, T)
    want, path = layer_ref.merge_ref(a_ref, T, b_ref, va, vb)
    got = lb.download()
    assert_same_layer(la.download(), a_ref, name + " A after the merge")
    n_rel = [check_relevant(lb, vb, mw, md, name) for mw, md in RELEVANT_CFGS]
    if path is None:
        print(f"[layer {name}] {c['meta']} blocks A {len(A[0])} B {len(B0[0])} -> {len(want[0])}, same grid, relevant {n_rel}")
    else:
        n = max(int((path != PATH_NONE).sum()), 1)
        print(f"[layer {name}] {c['meta']} blocks A {len(A[0])} B {len(B0[0])} -> {len(want[0])}, resampled blocks {len(path)}, written voxels "
              f"{int((path != PATH_NONE).sum())}, trilinear {(path == PATH_TRILINEAR).sum() / n:.3f}, nearest {(path == PATH_NEAREST).sum() / n:.3f}, relevant {n_rel}")
    assert_same_layer(got, want, name + " merge")
    return path


def check_plane(eng, T, name=""):
    """A is an exact plane d = n.x - off of weight 1 over the full box at 0.1 m, merged through T into an empty B.  Trilinear
    interpolation reproduces a plane, so every voxel layer_ref takes the trilinear path for must equal the plane evaluated in
    float64 at R^T (c - t), and every voxel on the nearest path lies within half a voxel diagonal (unit gradient).

    Trilinear bound: layer_ref's own largest error against float64 over the four transforms of layer_cases.PLANE_TRANSFORMS
    was measured on the CPU as 1.385e-6 (yaw 0.17: 1.064e-6, axis (1,2,3) by 1.1: 1.385e-6, 90 degrees about z: 7.12e-7,
    translation: 9.39e-7; trilinear shares 0.953, 0.954, 0.946, 0.949).  PLANE_REF_ERR = 1.39e-6 pins it and the engines get
    PLANE_BOUND = 4 x 1.39e-6 = 5.56e-6 (float32 position rounding grows with the coordinate).  At least 0.9 of the written
    voxels must be on the trilinear path, from layer_ref's path codes."""
    voxel = 0.1
    idx, vox, n = layer_cases.plane_layer([0.3, -0.5, 0.8], 0.137)
    off = 0.137
    la, lb = build(eng, (idx, vox), voxel), Layer(eng, voxel)
    lb.merge_from(la, T)
    gi, gv = lb.download()
    a_ref = layer_ref.upload_ref(layer_ref.empty_layer(), idx, vox, 0)
    (ri, rv), path = layer_ref.merge_ref(a_ref, T, layer_ref.empty_layer(), voxel)
    assert np.array_equal(gi, ri), name
    R, t = layer_cases.rotation_matrix(T[:4].astype(np.float64) / np.linalg.norm(T[:4].astype(np.float64))), T[4:].astype(np.float64)
    truth = ((layer_cases.centres64(gi, voxel) - t) @ R) @ n - off      # row (c - t) times R = R^T (c - t)
    tri, near = path == PATH_TRILINEAR, path == PATH_NEAREST
    share = tri.sum() / max(int((tri | near).sum()), 1)
    out = {}
    for who, v in (("reference", rv), ("engine", gv)):
        d, w = v[..., 0].view(np.float32).astype(np.float64), v[..., 1].view(np.float32)
        assert np.array_equal(w > 0, tri | near), (name, who)
        out[who] = (float(np.max(np.abs(d - truth)[tri])), float(np.max(np.abs(d - truth)[near])) if near.any() else 0.0)
    print(f"[plane {name}] written {int((tri | near).sum())}, trilinear share {share:.3f}; trilinear max |d - plane|: reference {out['reference'][0]:.3e}, "
          f"engine {out['engine'][0]:.3e} (bound {PLANE_BOUND:.1e}); nearest: reference {out['reference'][1]:.3e}, engine {out['engine'][1]:.3e}")
    assert share >= PLANE_MIN_TRILINEAR, (name, share)
    assert out["reference"][0] <= PLANE_REF_ERR, (name, out)
    assert out["engine"][0] <= PLANE_BOUND, (name, out)
    assert max(out["reference"][1], out["engine"][1]) <= 0.5 * np.sqrt(3.0) * voxel, (name, out)
    return out, share


def check_block_shift(eng, shift_blocks=(1, -2, 3)):
    """voxel 0.125 (block edge 2.0): a translation by whole blocks into an empty B is A with its indices shifted"""
    idx, vox = layer_cases.exact_layer(5)
    la, lb = build(eng, (idx, vox), 0.125), Layer(eng, 0.125)
    lb.merge_from(la, layer_cases.pose([1, 0, 0, 0], 2.0 * np.array(shift_blocks)))
    moved = idx + np.array(shift_blocks, np.int32)
    o = layer_ref.order_zyx(moved)
    assert_same_layer(lb.download(), (moved[o], vox[o]), "block shift")


def check_half_turn(eng, axis):
    """voxel 0.125: a half turn about an axis into an empty B is the mirrored copy, word for word"""
    idx, vox = layer_cases.exact_layer(6 + axis)
    q = np.zeros(4)
    q[1 + axis] = 1.0
    la, lb = build(eng, (idx, vox), 0.125), Layer(eng, 0.125)
    lb.merge_from(la, layer_cases.pose(q, [0, 0, 0]))
    flip = [k for k in range(3) if k != axis]
    midx = idx.copy()
    midx[:, flip] = -idx[:, flip] - 1
    loc = layer_cases.LOC.copy()
    loc[:, flip] = 15 - loc[:, flip]
    src = loc[:, 0] + 16 * (loc[:, 1] + 16 * loc[:, 2])     # output voxel l holds the input voxel mirrored within its block
    o = layer_ref.order_zyx(midx)
    assert_same_layer(lb.download(), (midx[o], vox[o][:, src]), f"half turn about axis {axis}")


def check_identity_is_none(eng, seed):
    c = layer_cases.case(seed)
    assert c["voxel_a"] == c["voxel_b"]
    out = []
    for T in (None, layer_cases.pose([1, 0, 0, 0], [0, 0, 0])):
        la, lb = build(eng, c["A"], c["voxel_a"]), build(eng, c["B"], c["voxel_b"])
        lb.merge_from(la, T)
        out.append(lb.download())
    assert len(out[0][0]) > 0
    assert_same_layer(out[1], out[0], f"identity against none, seed {seed}")


def check_empty_and_self(eng):
    """an empty A is a no-op, and a layer is not merged into itself: COX_ERR_INVALID_ARG, B untouched"""
    c = layer_cases.case(1)
    lb, la = build(eng, c["A"], c["voxel_a"]), Layer(eng, c["voxel_a"], capacity_blocks=64)
    before = lb.download()
    small = layer_cases.pose([1, 0, 0, 0], [0.03, 0.02, 0.01])
    for T in (None, small):
        lb.merge_from(la, T)
        assert_same_layer(lb.download(), before, "empty A")
        with pytest.raises(CoxError) as e:
            lb.merge_from(lb, T)
        assert e.value.status == -1
        assert_same_layer(lb.download(), before, "A is B")


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_layer_store_matches_reference(oracle, seed):
    check_case(oracle, layer_cases.case(seed), f"seed {seed}")


def test_cases_reach_every_path_and_family():
    """the fuzz is not vacuous: over the seeds, both resample paths, unwritten voxels, every transform and every B occur"""
    seen, tri, near, none = set(), 0, 0, 0
    for seed in SEEDS:
        c = layer_cases.case(seed)
        seen |= {c["meta"]["transform"], "B " + c["meta"]["b"], "scale %g" % c["meta"]["scale"], c["meta"]["mask"], c["meta"]["colour"]}
        if c["T"] is not None and seed % 4 == 2:
            path = layer_ref.resample_ref(*c["A"], c["voxel_a"], c["T"], c["voxel_b"])[2]
            tri, near, none = tri + int((path == PATH_TRILINEAR).sum()), near + int((path == PATH_NEAREST).sum()), none + int((path == PATH_NONE).sum())
    want = set(layer_cases.TRANSFORMS) | {"B " + b for b in layer_cases.B_KINDS} | {"scale 0.5", "scale 1", "scale 2"} | set(layer_cases.MASKS) | set(layer_cases.COLOURS)
    assert want <= seen, want - seen
    assert tri > 10000 and near > 10000 and none > 10000, (tri, near, none)


@pytest.mark.parametrize("k", range(4))
def test_oracle_resample_reproduces_a_plane(oracle, k):
    check_plane(oracle, layer_cases.PLANE_TRANSFORMS[k], f"transform {k}")


def test_oracle_whole_block_translation_is_a_shift(oracle):
    check_block_shift(oracle)


@pytest.mark.parametrize("axis", range(3))
def test_oracle_half_turn_is_a_mirror(oracle, axis):
    check_half_turn(oracle, axis)


@pytest.mark.parametrize("seed", [0, 8, 16])
def test_oracle_identity_transform_equals_no_transform(oracle, seed):
    check_identity_is_none(oracle, seed)


def test_oracle_merge_of_an_empty_layer_and_of_a_layer_into_itself(oracle):
    check_empty_and_self(oracle)


def test_merge_voxels_ref_rounds_half_away_from_zero():
    """the reference's own rounding, by hand: equal weights, bytes 1 and 2 blend to 1.5 -> 2, 2 and 3 to 2.5 -> 3 (half to
    even would give 2), alpha included; weight 0 on both sides leaves B alone"""
    one = np.float32(1).view(np.uint32)
    a = np.array([[0, one, 0x01020001], [7, 0, 0xFFFFFFFF]], np.uint32)
    b = np.array([[0, one, 0x02030002], [9, 0, 0x11111111]], np.uint32)
    out = layer_ref.merge_voxels_ref(a, b)
    assert out[0, 2] == 0x02030002 and out[0, 1] == np.float32(2).view(np.uint32)
    assert np.array_equal(out[1], b[1])
