"""The mesh clean-up rules on the numpy reference, by hand and by physics, and the library's side of them
that needs no GPU: the five entry points are exported and fail cleanly without a device."""
import ctypes as C

import numpy as np
import pytest

import meshclean_cases as K
import meshclean_ref as R

SYMBOLS = ["cox_meshconn_from_arrays", "cox_meshconn_clean", "cox_meshconn_smooth_taubin", "cox_meshconn_simplify_clustering",
           "cox_meshconn_compute_normals"]

# Noisy unit icosphere (642 vertices, radial sigma 0.02), 10 Taubin iterations, float64 reference, measured here: the radial
# standard deviation falls from 0.0201 to 0.0075 and the enclosed volume grows by 0.92 % (mu = -0.53 is a slight inflation:
# at 100 iterations it is +9.6 %).  Bounds: the deviation at least halves, the volume stays within 2 %.
SPHERE_STD_RATIO_MAX = 0.5
SPHERE_VOLUME_DRIFT_MAX = 0.02


def test_one_triangle():
    m = R.mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 2, 0]], rgb=[[10, 20, 30]] * 3)
    c, removed = R.clean(m)
    assert removed == (0, 0, 0) and np.array_equal(c["triangles"], [[1, 2, 0]]) and np.array_equal(c["xyz"], m["xyz"])
    n = R.compute_normals(m)
    assert np.array_equal(n, [[0, 0, 1]] * 3)
    p = R.smooth_taubin(m, 1, 0.5, -0.5)
    # lambda: every vertex goes half way to the midpoint of the other two; by hand for vertex 0: (0,0,0) -> (0.25, 0.25, 0)
    half = R.smooth_taubin(m, 1, 0.5, 0.0)
    assert np.allclose(half, [[0.25, 0.25, 0], [0.5, 0.25, 0], [0.25, 0.5, 0]], atol=1e-15)
    assert p.shape == (3, 3) and np.all(p[:, 2] == 0)
    s, cid = R.simplify_clustering(m, 0.25)
    assert np.array_equal(cid, [0, 1, 2]) and np.array_equal(s["triangles"], [[1, 2, 0]]) and np.array_equal(s["rgb"], m["rgb"])


def test_two_triangles_on_the_same_vertices():
    xyz = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    same, removed = R.clean(R.mesh(xyz, [[0, 1, 2], [1, 2, 0]]))  # a rotation: the same oriented triangle
    assert removed == (0, 1, 0) and np.array_equal(same["triangles"], [[0, 1, 2]])
    kept, removed = R.clean(R.mesh(xyz, [[1, 2, 0], [0, 1, 2]]))  # the survivor keeps its own rotation
    assert removed == (0, 1, 0) and np.array_equal(kept["triangles"], [[1, 2, 0]])
    both, removed = R.clean(R.mesh(xyz, [[0, 1, 2], [0, 2, 1]]))  # opposite orientation: different triangles
    assert removed == (0, 0, 0) and np.array_equal(both["triangles"], [[0, 1, 2], [0, 2, 1]])


def test_degenerate_triangles_and_unreferenced_vertices():
    xyz = np.arange(18, dtype=np.float32).reshape(6, 3)
    m = R.mesh(xyz, [[4, 4, 1], [5, 1, 3], [3, 5, 1], [2, 3, 2]], rgb=np.arange(18).reshape(6, 3))
    c, removed = R.clean(m)
    assert removed == (2, 1, 3)
    assert np.array_equal(c["xyz"], xyz[[1, 3, 5]]) and np.array_equal(c["rgb"], m["rgb"][[1, 3, 5]])
    assert np.array_equal(c["triangles"], [[2, 0, 1]])


def test_tetrahedron_in_one_cell_vanishes():
    m = R.mesh(K.TETRA_XYZ, K.TETRA_TRI)
    s, cid = R.simplify_clustering(m, 4.0)
    assert np.array_equal(cid, [0, 0, 0, 0]) and s["xyz"].shape == (0, 3) and s["triangles"].shape == (0, 3)
    # four cells: nothing merges
    s, cid = R.simplify_clustering(m, 0.5)
    assert len(np.unique(cid)) == 4 and len(s["triangles"]) == 4
    # cells in ascending (z, y, x): (0,0,0), (x), (y), (z)
    assert np.array_equal(cid, [0, 1, 2, 3])


def test_cluster_average_by_hand():
    xyz = [[0.0, 0, 0], [0.1, 0, 0], [0.2, 0.1, 0], [1.0, 0, 0], [0, 1.0, 0]]
    m = R.mesh(xyz, [[0, 3, 4], [1, 3, 4], [2, 4, 3]], normals=[[0, 0, 1], [0, 0, 1], [0, 0, 2], [1, 0, 0], [0, 0, 0]],
               rgb=[[1, 0, 255], [2, 0, 255], [2, 1, 254], [9, 9, 9], [7, 7, 7]])
    s, cid = R.simplify_clustering(m, 0.5)
    assert np.array_equal(cid, [0, 0, 0, 1, 2])
    assert np.allclose(s["xyz"][0], [0.1, 0.1 / 3, 0], atol=1e-7) and np.array_equal(s["normals"][0], [0, 0, 1])
    assert np.array_equal(s["normals"][2], [0, 0, 0])  # a zero sum stays zero
    assert np.array_equal(s["rgb"][0], [2, 0, 255])    # (2 * 5 + 3) // 6, (2 * 1 + 3) // 6, (2 * 764 + 3) // 6
    assert np.array_equal(s["triangles"], [[0, 1, 2], [0, 2, 1]])  # the first two collapse into one


def test_flat_regular_grid_interior_does_not_move():
    n, iters = 14, 2
    m = K.grid(n, spacing=0.125)  # exact in binary: the six neighbours of an interior vertex average to it exactly
    for dtype in (np.float64, np.float32):
        p = R.smooth_taubin(m, iters, dtype=dtype)
        moved = np.any(p != m["xyz"].astype(dtype), axis=1).reshape(n, n)
        # a half-step moves a vertex only if it or a neighbour is off balance: the boundary first, one ring further per half-step
        ring = 2 * iters
        assert not moved[ring:-ring, ring:-ring].any() and moved[0].all() and moved[:, -1].all()
    assert np.all(p[:, 2] == 0)


def test_noisy_sphere_gets_smoother_and_keeps_its_volume():
    s = K.icosphere(3, 1.0, noise=0.02)
    p = R.smooth_taubin(s, 10)
    r0, r1 = np.linalg.norm(s["xyz"].astype(np.float64), axis=1), np.linalg.norm(p, axis=1)
    v0, v1 = K.volume(s["xyz"], s["triangles"]), K.volume(p, s["triangles"])
    print(f"radial std {r0.std():.5f} -> {r1.std():.5f}, volume {v0:.5f} -> {v1:.5f} ({v1 / v0 - 1:+.4%})")
    assert r1.std() < SPHERE_STD_RATIO_MAX * r0.std()
    assert abs(v1 / v0 - 1) < SPHERE_VOLUME_DRIFT_MAX


def test_sphere_normals_are_radial():
    s = K.icosphere(3, 2.0, center=(1.0, -2.0, 0.5))
    n = R.compute_normals(s)
    u = s["xyz"].astype(np.float64) - [1.0, -2.0, 0.5]
    cos = np.einsum("ij,ij->i", n, u / np.linalg.norm(u, axis=1)[:, None])
    assert cos.min() > 0.9999 and np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-12)


@pytest.mark.parametrize("cell", [0.05, 0.3, 1.1])
def test_partition_does_not_depend_on_the_accumulation_dtype(cell):
    m = K.grid(24, spacing=0.1, noise=0.03, offset=(100.0, -50.0, 3.0))
    a, cid_a = R.simplify_clustering(m, cell, np.float64)
    b, cid_b = R.simplify_clustering(m, cell, np.float32)
    assert np.array_equal(cid_a, cid_b) and np.array_equal(a["triangles"], b["triangles"]) and np.array_equal(a["rgb"], b["rgb"])
    assert a["xyz"].shape == b["xyz"].shape and np.abs(a["xyz"] - b["xyz"]).max() < 1e-4
    with pytest.raises(R.IndexRange):
        R.partition(m["xyz"], 1e-6)


def test_library_exports_the_clean_up_and_fails_cleanly_without_a_gpu(hip):
    missing = [s for s in SYMBOLS if not hasattr(hip.lib, s)]
    assert not missing, missing
    h = C.c_void_p()
    xyz, tri = np.ascontiguousarray(K.TETRA_XYZ), np.ascontiguousarray(K.TETRA_TRI)
    st = hip.fn("meshconn_from_arrays")(C.c_int(0), xyz.ctypes.data_as(C.c_void_p), None, None, tri.ctypes.data_as(C.c_void_p), C.c_uint64(4), C.c_uint64(4),
                                        C.byref(h))
    if hip.device_count() > 0:
        assert st == 0 and h.value
        hip.fn("meshconn_destroy", None)(h)
    else:
        assert st == -2 and not h.value  # COX_ERR_NO_DEVICE: nothing falls back to the host
        assert hip.fn("meshconn_from_arrays")(C.c_int(0), None, None, None, None, C.c_uint64(4), C.c_uint64(0), C.byref(h)) == -1
