"""The map queries' C ABI (include/coxgraph_hip_map.h) and the test-side reference's known answers -- no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return map_ref.build(tmp_path_factory.mktemp("mapref"))


def _declared_map_symbols():
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_map.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def test_map_header_symbols_are_exported(hip):
    syms = _declared_map_symbols()
    assert syms == ["cox_layer_free_points", "cox_layer_query", "cox_layer_query_dev"]
    missing = [s for s in syms if not hasattr(hip.lib, s)]
    assert not missing, missing


def test_map_entry_points_fail_cleanly(hip):
    """Without a GPU every call reports COX_ERR_NO_DEVICE; with one, a NULL layer is COX_ERR_INVALID_ARG."""
    f = hip.fn
    xyz = (C.c_float * 3)(0, 0, 0)
    d = (C.c_float * 1)()
    st = (C.c_uint8 * 1)()
    n = C.c_uint64()
    want = -2 if hip.device_count() == 0 else -1
    assert f("layer_query")(None, xyz, C.c_uint64(1), C.c_int(1), C.c_int(0), d, None, None, st) == want
    assert f("layer_query_dev")(None, xyz, C.c_uint64(1), C.c_int(1), C.c_int(0), d, None, None, st, None) == want
    assert f("layer_free_points")(None, C.c_float(0.0), None, None, C.c_uint64(0), C.byref(n)) == want


def test_reference_reproduces_an_affine_field(ref):
    """Trilinear interpolation is exact on an affine field, and so are central differences: d = a . x + c and grad = a."""
    idx, words = map_ref.affine_layer_arrays()
    L = ref.layer(map_ref.AFFINE_VS, idx, words)
    q = map_ref.affine_queries(np.random.default_rng(3))
    exact = q.astype(np.float64) @ map_ref.AFFINE_A.astype(np.float64) + float(map_ref.AFFINE_C)
    for mode in ("interpolate", "adaptive"):
        r = L.query(q, mode, gradient=True)
        assert np.all(r["status"] == 7), mode
        assert np.max(np.abs(r["distance"] - exact)) < 2e-6
        assert np.all(r["weight"] == 1.0)
        assert np.max(np.abs(r["gradient"] - map_ref.AFFINE_A)) < 2e-5
    # nearest: the value stored at the voxel containing the point; the nearest gradient is the same exact difference
    r = L.query(q, "nearest", gradient=True)
    assert np.all(r["status"] == 5)
    v = np.floor(q.astype(np.float64) / 0.1 + 1e-6).astype(np.int64)
    b, l = v // 16, v % 16
    bi = b[:, 0] + 2 * b[:, 1] + 4 * b[:, 2]
    stored = words[bi, l[:, 0] + 16 * l[:, 1] + 256 * l[:, 2], 0].view(np.float32)
    assert np.array_equal(r["distance"], stored)
    assert np.max(np.abs(r["gradient"] - map_ref.AFFINE_A)) < 2e-5
    # centres of voxels: the trilinear value is the stored one (within rounding of the offsets)
    cen = map_ref.voxel_centres(idx, map_ref.AFFINE_VS).reshape(-1, 3)
    inner = np.all(cen < np.float32(3.1), axis=1)  # the last centre on an axis has no upper neighbour
    rc = L.query(cen[inner], "interpolate")
    assert np.all(rc["status"] == 3)
    assert np.max(np.abs(rc["distance"] - words[..., 0].reshape(-1)[inner].view(np.float32))) < 2e-6


def test_reference_misses(ref):
    idx, words = map_ref.affine_layer_arrays()
    L = ref.layer(map_ref.AFFINE_VS, idx, words)
    q = np.array([[0.02, 1.0, 1.0],      # below the first voxel centre: the cell needs block -1
                  [3.18, 1.0, 1.0],      # above the last centre
                  [5.0, 1.0, 1.0],       # no block at all
                  [np.nan, 1, 1], [np.inf, 1, 1], [-np.inf, 1, 1],
                  [3e6, 0, 0],           # beyond the block-index range
                  [0.06, 1.0, 1.0]], np.float32)
    r = L.query(q, "interpolate", gradient=True)
    assert r["status"].tolist() == [0, 0, 0, 0, 0, 0, 0, 2 | 1]
    assert np.isnan(r["distance"][:7]).all() and np.isnan(r["gradient"]).all()
    a = L.query(q, "adaptive", gradient=True)
    # the first two fall back to nearest: value yes, gradient no (a sample leaves the layer); the last has the trilinear
    # value but no trilinear gradient, so it is answered by nearest too
    assert a["status"].tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    n = L.query(q, "nearest")
    assert n["status"].tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    # an invalid voxel (weight 0) breaks the cells that use it
    w2 = words.copy()
    w2[0, 0, 1] = 0
    L2 = ref.layer(map_ref.AFFINE_VS, idx, w2)
    r2 = L2.query(np.array([[0.07, 0.07, 0.07], [0.04, 0.04, 0.04]], np.float32), "interpolate")
    assert r2["status"].tolist() == [0, 0]
    assert L2.query(np.array([[0.04, 0.04, 0.04], [0.14, 0.04, 0.04]], np.float32), "nearest")["status"].tolist() == [0, 1]


def test_reference_free_point_count_of_a_hand_built_esdf(ref):
    """Two blocks: distances 0 .. 4095 cm along the linear index, every third voxel unobserved."""
    idx = np.array([[1, 0, 0], [0, 0, 0]], np.int32)
    words = np.zeros((2, 4096, 3), np.uint32)
    d = (np.arange(4096, dtype=np.float32) * np.float32(0.01))
    words[:, :, 0] = d.view(np.uint32)
    w = np.where(np.arange(4096) % 3 == 0, 0.0, 1.0).astype(np.float32)
    words[:, :, 1] = w.view(np.uint32)
    L = ref.layer(0.1, idx, words)
    observed = int((w > 0).sum())
    assert len(L.free_points(0.0)[0]) == 2 * observed
    xyz, inten = L.free_points(20.0)
    keep = (w > 0) & (d >= np.float32(20.0))
    assert len(xyz) == 2 * int(keep.sum())
    assert len(L.free_points(1e9)[0]) == 0
    # block (0,0,0) first, voxels in linear order, centre = origin + (v + 0.5) * voxel
    cen = map_ref.voxel_centres(np.array([[0, 0, 0], [1, 0, 0]]), 0.1)
    assert np.array_equal(xyz, np.concatenate([cen[0][keep], cen[1][keep]]))
    assert np.array_equal(inten, np.concatenate([d[keep], d[keep]]))
