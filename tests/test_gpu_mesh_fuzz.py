"""Differential fuzz of the GPU mesher (coxgraph_amd/csrc/cox_mesher.hip) over the seeded layers of tests/mesh_cases.py: noise
layers where most cubes emit triangles, scattered unobserved voxels, weights on the validity threshold, +-0.0 and sub-1e-6
distances, missing neighbour blocks, shuffled / grown / merged pools, and boxes near the origin, thousands of blocks out and
half a million blocks out.

Per case: MeshLayer.from_layer against the C++ reference (tests/cpp/mesh_reference.cpp) bit for bit -- block list, vertex
ranges, positions, normals, colours, the missing-colour count and the message arrays of all five colour modes -- and the
connected mesh against the numpy weld of tests/mesh_ref.py.  Then what no reference mesh exercises: k_mesh_transform against a
float64 transform, the wire encoding of a moved mesh (both clamps), and the weld's edges (a part twice, empty parts, one
triangle, one cell for everything, negative cells with ties, a span beyond 2^21 cells).  Nothing but the transform has a
tolerance, and that one is derived from quat_rotate's operation count.

COX_FUZZ_SEEDS=N widens the sweep (the convention of tests/test_gpu_projective_fuzz.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_cases
import mesh_ref
from coxgraph_amd.capi import CoxError, Layer, MeshLayer

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("COX_FUZZ_SEEDS", "24"))
INDEX_RANGE = -5
F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], F)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("meshref"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_mesh_equal(g, r, name):
    assert np.array_equal(g["block_index"], r["block_index"]) and np.array_equal(g["vertex_begin"], r["vertex_begin"]), name
    assert np.array_equal(_bits(g["xyz"]), _bits(r["xyz"])), (name, int((_bits(g["xyz"]) != _bits(r["xyz"])).any(axis=1).sum()))
    assert np.array_equal(_bits(g["normals"]), _bits(r["normals"])), (name, int((_bits(g["normals"]) != _bits(r["normals"])).any(axis=1).sum()))
    assert np.array_equal(g["rgb"], r["rgb"]), (name, int((g["rgb"] != r["rgb"]).any(axis=1).sum()))


def assert_weld_equal(got, want, name):
    assert np.array_equal(_bits(got["xyz"]), _bits(want["xyz"])), name
    assert np.array_equal(_bits(got["normals"]), _bits(want["normals"])), name
    assert np.array_equal(got["rgb"], want["rgb"]), name
    assert np.array_equal(got["triangles"], want["triangles"]), name


def check_weld(hip, parts, T, thr, cat, name):
    """connected(parts, T, thr) against weld_ref of the concatenation cat = (xyz, normals, rgb) the caller worked out"""
    try:
        want = mesh_ref.weld_ref(*cat, thr)
    except mesh_ref.IndexRange:
        with pytest.raises(CoxError) as e:
            MeshLayer.connected(hip, parts, T, thr)
        assert e.value.status == INDEX_RANGE, name
        return None
    got = MeshLayer.connected(hip, parts, T, thr)
    assert_weld_equal(got, want, name)
    return got


def check_case(hip, ref, c, name):
    voxel, _, _, min_w, meta = c
    layer = mesh_cases.build_layer(hip, c)
    idx, vox = layer.download()             # what the reference is fed: a merge may rewrite voxels
    r = ref.mesh(voxel, idx, vox, min_w)
    m = MeshLayer.from_layer(hip, layer, min_weight=min_w)
    g = m.download()
    print(f"[{name}] {meta['field']} {meta['blocks']} {meta['lo']} {meta['build']} voxel {voxel} min_weight {min_w}: {len(idx)} blocks, "
          f"{m.n_triangles} triangles, missing {m.stats()[0]} (reference {r['n_missing']})")
    assert_mesh_equal(g, r, name)
    assert m.stats()[0] == r["n_missing"], name
    for mode in mesh_ref.MODES:
        a = m.msg_arrays(mode)
        for k in "xyzrgb":
            assert np.array_equal(a[k], r["msg"][mode][k]), (name, mode, k)
    for thr in (0.5 * voxel, 1e-3):
        check_weld(hip, [m], None, thr, (g["xyz"], g["normals"], g["rgb"]), (name, thr))
    return m, g, r


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_seed_sweep(hip, ref, seed):
    check_case(hip, ref, mesh_cases.case(seed), f"seed {seed}")


@pytest.mark.parametrize("seed,family", mesh_cases.FAMILY_CASES, ids=[f"{s}-" + "-".join(f) for s, f in mesh_cases.FAMILY_CASES])
def test_family_case(hip, ref, seed, family):
    _, _, r = check_case(hip, ref, mesh_cases.case(seed, family), f"family {seed}")
    if family[1] in ("full", "subset70", "slab", "two_components"):
        assert len(r["xyz"]) >= 3000


def test_extreme_origin_is_bit_identical_missing_colours_included(hip, ref):
    """Half a million blocks out a float32 coordinate has 3 cm between neighbours, more than half a voxel: a vertex can round
    into a block or a voxel that is no corner of its cube.  DESIGN.md section 7d's rule decides (block by coordinates, voxel
    clamped into it, missing only when that block does not exist); the reference implements it."""
    m, _, r = check_case(hip, ref, mesh_cases.case(*mesh_cases.EXTREME_CASE), "extreme")
    assert r["n_missing"] >= 1 and m.stats()[0] == r["n_missing"]


def test_block_face_that_rounds_into_the_block_below(hip, ref):
    """the pinned face case: thousands of vertices whose voxel index within the block found by coordinates is 16, clamped to 15"""
    check_case(hip, ref, mesh_cases.case(*mesh_cases.FACE_CASE), "face")


# ---- k_mesh_transform against float64 -------------------------------------------------------------------------------------------
# quat_rotate as cox_device.hpp writes it: uv = cross(q, v) is two products and a difference per component (3 roundings; uv + uv
# is exact), c = cross(q, uv) three more per component, and (v + qw * uv) + c a product and two sums.  One output component
# reads all three components of uv (two through c, one through qw * uv): 9 + 3 + 3 = 15 roundings; the translation adds one.
ROUNDINGS_ROTATE, ROUNDINGS_TRANSLATE = 15, 1
U = 2.0 ** -24
GENERIC_Q = np.array([0.3, -0.5, 0.7, 0.4]) / np.linalg.norm([0.3, -0.5, 0.7, 0.4])
POSES = {"identity": IDENTITY,
         "quarter_turn_z": np.array([np.sqrt(0.5), 0, 0, np.sqrt(0.5), 1.5, -2.25, 0.75], F),
         "generic": np.concatenate([GENERIC_Q, [30.0, -35.0, 20.0]]).astype(F),         # |t| = 50.2 m
         "generic_negated": np.concatenate([-GENERIC_Q, [30.0, -35.0, 20.0]]).astype(F)}
NEAR_NOISE = (220, ("noise", "full", "near", "plain"))


@pytest.fixture(scope="module")
def near_noise(hip):
    c = mesh_cases.case(*NEAR_NOISE)
    return c, mesh_cases.build_layer(hip, c)


def test_transform_against_float64(hip, near_noise):
    c, layer = near_noise
    g = MeshLayer.from_layer(hip, layer, min_weight=c[3]).download()
    assert len(g["xyz"]) > 10000
    out = {}
    for name, T in POSES.items():
        m = MeshLayer.from_layer(hip, layer, min_weight=c[3])
        m.transform(T)
        t = out[name] = m.download()
        assert np.array_equal(t["rgb"], g["rgb"]) and np.array_equal(t["vertex_begin"], g["vertex_begin"]), name
        p, n = mesh_ref.transform_ref(g["xyz"], g["normals"], T)
        len_p = np.linalg.norm(g["xyz"].astype(np.float64), axis=1, keepdims=True)
        len_n = np.linalg.norm(g["normals"].astype(np.float64), axis=1, keepdims=True)
        len_t = np.linalg.norm(T[4:].astype(np.float64))
        bound_p = (ROUNDINGS_ROTATE + ROUNDINGS_TRANSLATE) * U * (len_p + len_t)
        bound_n = ROUNDINGS_ROTATE * U * len_n
        err_p, err_n = np.abs(t["xyz"] - p), np.abs(t["normals"] - n)
        grow = np.abs(np.linalg.norm(t["normals"].astype(np.float64), axis=1, keepdims=True) - len_n)
        print(f"[transform {name}] largest error / bound: positions {np.max(err_p / bound_p):.3f}, normals {np.max(err_n / np.maximum(bound_n, 1e-300)):.3f}, "
              f"normal length {np.max(grow / np.maximum(bound_n, 1e-300)):.3f}")
        assert np.all(err_p <= bound_p), (name, float(np.max(err_p / bound_p)))
        assert np.all(err_n <= bound_n), name
        assert np.all(grow <= bound_n), name
    assert np.array_equal(_bits(out["identity"]["xyz"]), _bits(g["xyz"])) and np.array_equal(_bits(out["identity"]["normals"]), _bits(g["normals"]))
    for k in ("xyz", "normals"):
        assert np.array_equal(_bits(out["generic"][k]), _bits(out["generic_negated"][k])), k
    # the quarter turn really turned: x -> y, y -> -x
    qt = out["quarter_turn_z"]["normals"]
    assert np.allclose(qt[:, 0], -g["normals"][:, 1], atol=1e-6) and np.allclose(qt[:, 1], g["normals"][:, 0], atol=1e-6)


def test_message_of_a_moved_mesh_reaches_both_clamps(hip, near_noise):
    """cox_meshlayer_msg on a transform()ed mesh: moved by (-3, +3, 0.25) block edges every x lies below its block (0), every y two
    blocks or more above (65535), and z stays between the clamps"""
    c, layer = near_noise
    m = MeshLayer.from_layer(hip, layer, min_weight=c[3])
    before = m.download()
    edge = F(m.block_edge_length)
    m.transform(np.concatenate([[1, 0, 0, 0], np.array([-3, 3, 0.25]) * float(edge)]).astype(F))
    g, a = m.download(), m.msg_arrays("color")
    want = mesh_ref.encode_ref(g["xyz"], mesh_ref.per_vertex_block(g), edge)
    for i, k in enumerate("xyz"):
        assert np.array_equal(a[k], want[:, i]), k
    assert np.all(a["x"] == 0) and np.all(a["y"] == 65535)
    assert np.all((a["z"] > 0) & (a["z"] < 65535))      # a quarter block up: still inside the two blocks the encoding spans
    assert np.array_equal(np.stack([a[k] for k in "rgb"], 1), before["rgb"])
    assert np.array_equal(g["xyz"], before["xyz"] + np.array([-3, 3, 0.25], F) * edge)    # one float32 sum per coordinate


# ---- the weld's edges ------------------------------------------------------------------------------------------------------------
SMALL, SMALL2 = (225, ("noise", "single", "near", "plain")), (223, ("noise", "corners_only", "near", "plain"))


@pytest.fixture(scope="module")
def small(hip):
    out = []
    for spec in (SMALL, SMALL2):
        c = mesh_cases.case(*spec)
        m = MeshLayer.from_layer(hip, mesh_cases.build_layer(hip, c), min_weight=c[3])
        assert m.n_vertices >= 100
        out.append((c, m, m.download()))
    return out


def _cat(*meshes):
    return tuple(np.concatenate([g[k] for g in meshes]) for k in ("xyz", "normals", "rgb"))


def _moved(g, t):
    """a downloaded mesh translated by a pure translation pose: one float32 sum per coordinate, normals and colours as they are"""
    return dict(g, xyz=g["xyz"] + np.asarray(t, F))


def test_weld_of_a_part_passed_twice(hip, small):
    (c, m, g), _ = small
    thr = 0.5 * c[0]
    one = MeshLayer.connected(hip, [m], None, thr)
    two = check_weld(hip, [m, m], None, thr, _cat(g, g), "twice")
    n = len(one["triangles"])
    assert len(two["xyz"]) == len(one["xyz"]) and len(two["triangles"]) == 2 * n
    assert np.array_equal(two["triangles"][n:], two["triangles"][:n]) and np.array_equal(two["triangles"][:n], one["triangles"])
    both = check_weld(hip, [m, m], np.stack([IDENTITY, IDENTITY]), thr, _cat(g, g), "twice, moved by the identity")
    assert np.array_equal(both["triangles"], two["triangles"])


def test_weld_with_empty_parts(hip, small):
    (c, m, g), (_, m2, g2) = small
    empty = MeshLayer.from_layer(hip, Layer(hip, c[0], capacity_blocks=64))
    assert empty.n_vertices == 0
    thr = 0.5 * c[0]
    check_weld(hip, [empty, m, empty, m2], None, thr, _cat(g, g2), "empty parts")
    check_weld(hip, [empty, m, empty, m2], np.stack([IDENTITY] * 4), thr, _cat(g, g2), "empty parts, poses")
    assert MeshLayer.connected(hip, [empty, empty], None, thr)["triangles"].shape == (0, 3)


def test_weld_of_one_triangle(hip, ref):
    """one cube with all eight corners observed, one of them inside: one triangle, a cell table of eight slots"""
    voxel = 0.125
    d, w = np.full(4096, 0.1, F), np.zeros(4096, F)
    for z in (3, 4):
        for y in (3, 4):
            for x in (3, 4):
                w[x + 16 * y + 256 * z] = 2.0
    d[3 + 16 * 3 + 256 * 3] = -0.05
    idx, vox = np.array([[-1, 0, 2]], np.int32), mesh_cases.words(d, w, np.uint32(0x10203040))[None]
    layer = Layer(hip, voxel, capacity_blocks=4)
    layer.upload(idx, vox)
    m = MeshLayer.from_layer(hip, layer, min_weight=1.0)
    g = m.download()
    assert m.n_triangles == 1
    assert_mesh_equal(g, ref.mesh(voxel, idx, vox, 1.0), "one cube")
    got = check_weld(hip, [m], None, 1e-3, _cat(g), "one triangle")
    assert got["triangles"].tolist() == [[0, 1, 2]]
    got = check_weld(hip, [m], None, 4 * voxel, _cat(g), "one triangle, one cell")
    assert got["triangles"].tolist() == [[0, 0, 0]] and len(got["xyz"]) == 1


def test_weld_with_one_cell_for_everything(hip, small):
    (_, m, g), (_, m2, g2) = small
    got = check_weld(hip, [m, m2], None, 1e6, _cat(g, g2), "threshold 1e6")
    assert len(got["xyz"]) == 1 and np.all(got["triangles"] == 0) and len(got["triangles"]) == (len(g["xyz"]) + len(g2["xyz"])) // 3
    assert np.array_equal(_bits(got["xyz"][0]), _bits(g["xyz"][0]))


def test_weld_span_beyond_the_key_range(hip, small):
    """two parts 3 000 m apart: 3e6 cells of 1 mm exceed the 2^21 the keys hold, 6 000 cells of 0.5 m do not"""
    (_, m, g), _ = small
    far = np.array([1, 0, 0, 0, 3000.0, 0, 0], F)
    T = np.stack([IDENTITY, far])
    cat = _cat(g, _moved(g, far[4:]))
    with pytest.raises(mesh_ref.IndexRange):
        mesh_ref.weld_ref(*cat, 1e-3)
    assert check_weld(hip, [m, m], T, 1e-3, cat, "3 km at 1 mm") is None
    # through the C ABI: the status, and no handle
    parts = (C.c_void_p * 2)(m.h.value, m.h.value)
    h, nv = C.c_void_p(), C.c_uint64(7)
    st = hip.fn("meshlayer_connected")(parts, T.ctypes.data_as(C.c_void_p), C.c_uint64(2), C.c_float(1e-3), C.byref(h), C.byref(nv), None)
    assert st == INDEX_RANGE and not h.value
    got = check_weld(hip, [m, m], T, 0.5, cat, "3 km at 0.5 m")
    assert got is not None and len(got["xyz"]) > 2


def test_weld_of_negative_cells_rounds_ties_away_from_zero(hip, small):
    """voxel 0.125, threshold 0.0625: a vertex on a cube edge has two coordinates at voxel centres, odd multiples of the threshold;
    moved by a whole number of cells less half a cell they are ties, all of them negative"""
    (c, m, g), _ = small
    assert c[0] == 0.125
    thr = 0.0625
    t = np.array([-100.03125, -50.03125, -20.03125], F)
    moved = _moved(g, t)
    cells = moved["xyz"].astype(np.float64) / thr
    ties = (cells - np.floor(cells)) == 0.5
    assert np.all(cells < 0) and ties.sum() > 100
    got = check_weld(hip, [m], np.concatenate([[1, 0, 0, 0], t]).astype(F)[None], thr, _cat(moved), "negative ties")
    # floor(x + 0.5) would put the ties one cell up and weld other vertices
    up = mesh_ref.weld_ref(moved["xyz"] + F(thr) * ties, moved["normals"], moved["rgb"], thr)
    assert not np.array_equal(up["triangles"], got["triangles"])


# ---- pool order ------------------------------------------------------------------------------------------------------------------
def test_pool_order_does_not_reach_the_mesh(hip, ref):
    """the same layer uploaded at once, in three shuffled uploads, into a pool that grows from four blocks, and half of it merged
    in from a second layer (weights are powers of two, so the merge gives back every observed voxel): the same bytes"""
    seed = 250
    first = None
    for build in mesh_cases.BUILDS:
        c = mesh_cases.case(seed, ("salt", "subset70", "near", build), pow2_weights=True)
        m = MeshLayer.from_layer(hip, mesh_cases.build_layer(hip, c), min_weight=c[3])
        g = m.download()
        if first is None:
            first = g
            assert len(g["xyz"]) > 3000
            assert_mesh_equal(g, ref.mesh(c[0], c[1], c[2], c[3]), "plain")
        for k in first:
            assert first[k].tobytes() == g[k].tobytes(), (build, k)
