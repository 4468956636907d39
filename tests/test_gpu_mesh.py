"""The GPU mesher (coxgraph_amd/csrc/cox_mesher.hip) against the test-side reference (tests/cpp/mesh_reference.cpp, whose vertex
positions come from the CPU checker's marching cubes), against the oracle-pinned isosurface path, and against physics that
needs no restatement: the synthetic scene's walls and sphere, and an analytic sphere's topology, area and volume."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

import mesh_ref
from coxgraph_amd import mesh_io, synth
from coxgraph_amd.capi import Integrator, Layer, MeshConverter, MeshLayer, MeshMsg, RegPoints
from util import run_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("meshref"))


@pytest.fixture(scope="module", params=[0.10, 0.05])
def submap(request, hip):
    """The tests/test_gpu_submap.py submap: frames 0..140 step 10 of the benchmark stream, merged, subsample 2."""
    voxel = request.param
    layer, _, _ = run_frames(hip, method="merged", voxel=voxel, frames=range(0, 150, 10), subsample=2, capacity_blocks=8192)
    return voxel, layer


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("min_w", [1.0, 1e-4])
def test_mesh_is_bit_identical_to_the_reference(hip, ref, submap, min_w):
    voxel, layer = submap
    m = MeshLayer.from_layer(hip, layer, min_weight=min_w)
    g = m.download()
    idx, vox = layer.download()
    r = ref.mesh(voxel, idx, vox, min_w)
    assert m.n_triangles > 1000 and m.n_blocks > 10
    assert np.array_equal(g["block_index"], r["block_index"]) and np.array_equal(g["vertex_begin"], r["vertex_begin"])
    assert np.array_equal(_bits(g["xyz"]), _bits(r["xyz"]))
    assert np.array_equal(_bits(g["normals"]), _bits(r["normals"]))
    assert np.array_equal(g["rgb"], r["rgb"])
    missing, ms = m.stats()
    assert missing == r["n_missing"] == 0 and ms[0] > 0 and ms[1] > 0
    assert np.count_nonzero(g["rgb"].any(axis=1)) > 0.9 * len(g["rgb"])  # the fused stream is coloured
    for mode in mesh_ref.MODES:
        a = m.msg_arrays(mode)
        for k in "xyzrgb":
            assert np.array_equal(a[k], r["msg"][mode][k]), (mode, k)


@pytest.mark.parametrize("min_w", [1.0, 1e-4])
def test_mesh_agrees_with_the_isosurface_path(hip, submap, min_w):
    voxel, layer = submap
    m = MeshLayer.from_layer(hip, layer, min_weight=min_w)
    thr = 0.5 * voxel
    p = RegPoints.from_isosurface(hip, layer, min_weight=min_w, vertex_proximity_threshold=thr)
    assert 3 * m.n_triangles == p.n_mesh_vertices
    c = MeshLayer.connected(hip, [m], None, thr)
    assert len(c["xyz"]) == p.n_connected_vertices and len(c["triangles"]) == m.n_triangles
    # every registration point is a connected vertex, in the same order
    where = {tuple(v): i for i, v in enumerate(_bits(c["xyz"]).tolist())}
    pos = [where[tuple(v)] for v in _bits(p.download()[:, :3].copy()).tolist()]
    assert len(pos) == p.n and np.all(np.diff(pos) > 0)
    # the welded triangles index the welded vertices and reproduce the unwelded positions within the threshold
    g = m.download()
    assert np.all(np.abs(c["xyz"][c["triangles"].reshape(-1)] - g["xyz"]) <= thr)


def test_mesh_lies_on_the_scene_and_normals_face_free_space(hip, submap):
    voxel, layer = submap
    g = MeshLayer.from_layer(hip, layer, min_weight=1.0).download()
    p, n = g["xyz"].astype(np.float64), g["normals"].astype(np.float64)
    d_planes = np.minimum(np.abs(p - synth.ROOM_MIN), np.abs(p - synth.ROOM_MAX))
    rad = p - synth.SPHERE_C
    r = np.linalg.norm(rad, axis=1)
    d_sphere = np.abs(r - synth.SPHERE_R)
    err = np.minimum(d_planes.min(axis=1), d_sphere)
    assert np.quantile(err, 0.95) < 0.5 * voxel
    # a face normal against the radial direction at its triangle's centroid (at a vertex of a sliver triangle the two differ by
    # the triangle's own extent): triangles whose three vertices are sphere vertices
    on_sphere = ((d_sphere < 0.5 * voxel) & (d_sphere < d_planes.min(axis=1))).reshape(-1, 3).all(axis=1)
    cen = p.reshape(-1, 3, 3).mean(axis=1)[on_sphere] - synth.SPHERE_C
    cos_sphere = np.einsum("ij,ij->i", n[::3][on_sphere], cen / np.linalg.norm(cen, axis=1)[:, None])
    assert on_sphere.sum() > 100 and np.quantile(cos_sphere, 0.05) > 0.9
    # wall vertices: the nearest plane is a wall, the normal points into the room (away from that wall)
    ax = d_planes.argmin(axis=1)
    lo = np.abs(p[np.arange(len(p)), ax] - synth.ROOM_MIN[ax]) < np.abs(p[np.arange(len(p)), ax] - synth.ROOM_MAX[ax])
    on_wall = (d_planes.min(axis=1) < 0.5 * voxel) & (d_sphere > 2 * voxel)
    inward = np.where(lo, 1.0, -1.0) * n[np.arange(len(p)), ax]
    print(f"sphere cos q05 {np.quantile(cos_sphere, 0.05):.3f}, wall inward q05 {np.quantile(inward[on_wall], 0.05):.3f}, {on_wall.sum()} wall vertices")
    assert on_wall.sum() > 1000 and np.quantile(inward[on_wall], 0.05) > 0.9


# ---- an analytic sphere that straddles block boundaries on all three axes ---------------------------------------------
VS, CENTER, RADIUS = 0.05, np.array([0.8 + 0.013, 0.8 - 0.021, 0.8 + 0.007]), 0.35


def _sphere_layer(hip, drop=None):
    idx, words = [], []
    lin = np.arange(4096)
    l = np.stack([lin & 15, (lin >> 4) & 15, lin >> 8], 1)
    for bz in (0, 1):
        for by in (0, 1):
            for bx in (0, 1):
                if drop == (bx, by, bz):
                    continue
                c = (np.array([bx, by, bz]) * 16 + l + 0.5) * VS
                d = np.clip(np.linalg.norm(c - CENTER, axis=1) - RADIUS, -3 * VS, 3 * VS).astype(np.float32)
                w = np.ones(4096, np.float32)
                words.append(np.stack([d.view(np.uint32), w.view(np.uint32), np.full(4096, 0x80604020, np.uint32)], 1))
                idx.append((bx, by, bz))
    layer = Layer(hip, VS, capacity_blocks=64)
    layer.upload(np.array(idx, np.int32), np.array(words, np.uint32))
    return layer


def _weld(xyz, tol):
    """Test-side weld: vertices closer than tol become the first of them."""
    pairs = cKDTree(xyz).query_pairs(tol, output_type="ndarray")
    rep = np.arange(len(xyz))
    for a, b in sorted(map(tuple, pairs)):
        ra, rb = rep[a], rep[b]
        while rep[ra] != ra:
            ra = rep[ra]
        while rep[rb] != rb:
            rb = rep[rb]
        rep[max(ra, rb)] = min(ra, rb)
    for i in range(len(rep)):
        j = i
        while rep[j] != j:
            j = rep[j]
        rep[i] = j
    return rep


def _edges(tri):
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    u, cnt = np.unique(e, axis=0, return_counts=True)
    return u, cnt


def test_analytic_sphere_is_closed_with_the_right_area_and_volume(hip, ref):
    layer = _sphere_layer(hip)
    m = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    g = m.download()
    idx, vox = layer.download()
    r = ref.mesh(VS, idx, vox, 1e-4)
    assert np.array_equal(_bits(g["xyz"]), _bits(r["xyz"])) and np.array_equal(_bits(g["normals"]), _bits(r["normals"]))
    assert m.n_blocks == 8  # every block holds part of the sphere
    xyz = g["xyz"].astype(np.float64)
    tri = _weld(xyz, 1e-4 * VS)[np.arange(len(xyz))].reshape(-1, 3)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    assert keep.all(), "degenerate triangles on a generic sphere"
    _, cnt = _edges(tri)
    assert np.all(cnt == 2), np.bincount(cnt)
    V, E, F = len(np.unique(tri)), len(cnt), len(tri)
    assert V - E + F == 2
    a, b, c = xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]
    cr = np.cross(b - a, c - a)
    area = 0.5 * np.linalg.norm(cr, axis=1).sum()
    vol = np.einsum("ij,ij->i", a - CENTER, np.cross(b - CENTER, c - CENTER)).sum() / 6.0
    assert abs(area / (4 * np.pi * RADIUS ** 2) - 1) < 0.02, area
    assert abs(vol / (4 / 3 * np.pi * RADIUS ** 3) - 1) < 0.03, vol
    # normals: the face normal of each triangle, outward
    assert np.all(np.einsum("ij,ij->i", g["normals"][::3], (a + b + c) / 3 - CENTER) > 0)


def test_a_missing_neighbour_block_opens_the_hole_the_reference_predicts(hip, ref):
    layer = _sphere_layer(hip, drop=(1, 0, 0))
    m = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    g = m.download()
    idx, vox = layer.download()
    r = ref.mesh(VS, idx, vox, 1e-4)
    assert np.array_equal(g["block_index"], r["block_index"]) and np.array_equal(g["vertex_begin"], r["vertex_begin"])
    assert np.array_equal(_bits(g["xyz"]), _bits(r["xyz"])) and np.array_equal(g["rgb"], r["rgb"])
    xyz = g["xyz"].astype(np.float64)
    tri = _weld(xyz, 1e-4 * VS).reshape(-1, 3)
    e, cnt = _edges(tri)
    assert np.all(cnt <= 2) and np.any(cnt == 1)
    # the open edges run around the missing block (x in [0.8, 1.6), y, z in [0, 0.8)): along its -x face and along the faces it
    # shares with the blocks above and beside it, where block (0,0,0)'s max-plane cubes lost their corners
    b = xyz[e[cnt == 1].reshape(-1)]
    assert np.all(b[:, 0] > 0.8 - 1.5 * VS) and np.all(b[:, 1] < 0.8 + 1.5 * VS) and np.all(b[:, 2] < 0.8 + 1.5 * VS)
    assert not np.any((xyz[:, 0] > 0.8 + VS) & (xyz[:, 1] < 0.8 - VS) & (xyz[:, 2] < 0.8 - VS))  # nothing inside it


def test_wire_encoding_round_trips(hip, submap):
    voxel, layer = submap
    m = MeshLayer.from_layer(hip, layer, min_weight=1.0)
    g, a = m.download(), m.msg_arrays("color")
    edge = np.float32(m.block_edge_length)
    bi = np.repeat(g["block_index"], np.diff(g["vertex_begin"].astype(np.int64)), axis=0).astype(np.float32)
    conv = np.float32(2.0) / np.float32(65535)
    dec = np.stack([(a[k].astype(np.float32) * conv + bi[:, i]) * edge for i, k in enumerate("xyz")], 1)
    # one fixed-point unit from the truncation, plus the float rounding of the decoder's own three operations
    err = np.abs(dec.astype(np.float64) - g["xyz"])
    tol = float(conv) * float(edge) + 3 * np.spacing(np.abs(g["xyz"])).astype(np.float64)
    assert np.all(err <= tol), (err - tol).max()
    assert np.array_equal(np.stack([a[k] for k in "rgb"], 1), g["rgb"])


def test_mesh_message_feeds_recover_mode(hip):
    """generateSubmapMeshMsg -> TsdfRecover::processMesh: the mesh of one frame, sent with one history run per triangle and that
    frame's pose, rebuilds a TSDF whose surface lies within a voxel of the original one."""
    voxel = 0.05
    layer, _, _ = run_frames(hip, method="merged", voxel=voxel, frames=[0], subsample=2, capacity_blocks=8192)
    m = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    T, _, _, _ = synth.make_frame(0)
    d = m.to_msg("color", history=lambda idx, n: [[0, 0]] * n, trajectory=[(1600000000, 0, T)])
    assert len(d["blocks"]) == m.n_blocks
    fresh = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, fresh, hip.default_config(**synth.integrator_overrides(voxel)), "merged")
    conv = MeshConverter(hip)
    n_points, n_calls = conv.process_mesh(integ, MeshMsg(**d))
    integ.sync()
    assert n_calls == 1 and n_points >= 3 * m.n_triangles
    back = MeshLayer.from_layer(hip, fresh, min_weight=1e-4).download()["xyz"]
    dist, _ = cKDTree(m.download()["xyz"]).query(back)
    print("recovered surface distance quantiles 50/95 % [voxels]:", np.quantile(dist, [0.5, 0.95]) / voxel)
    assert len(back) > 0.5 * 3 * m.n_triangles and np.quantile(dist, 0.95) < voxel


def test_mesh_orders_behind_frames_in_flight(hip):
    voxel = 0.05
    cfg = hip.default_config(**synth.integrator_overrides(voxel))
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, cfg, "merged")
    frames = [synth.make_frame(t) for t in range(0, 60, 10)]
    keep = []
    for T, pts, rgba, _ in frames:
        pts, rgba = np.ascontiguousarray(pts[::2]), np.ascontiguousarray(rgba[::2])
        keep.append((pts, rgba))
        integ.integrate_points_async(T, pts.ctypes.data, rgba.ctypes.data, len(pts))
    a = MeshLayer.from_layer(hip, layer, min_weight=1e-4).download()
    integ.sync()
    b = MeshLayer.from_layer(hip, layer, min_weight=1e-4).download()
    assert len(b["xyz"]) > 1000
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_edge_cases(hip, submap):
    voxel, layer = submap
    empty = Layer(hip, voxel, capacity_blocks=64)
    m = MeshLayer.from_layer(hip, empty)
    assert (m.n_blocks, m.n_triangles) == (0, 0) and m.download()["xyz"].shape == (0, 3)
    assert MeshLayer.connected(hip, [m], None, 0.01)["triangles"].shape == (0, 3)
    # blocks without a valid cube: every weight zero
    idx = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
    vox = np.zeros((2, 4096, 3), np.uint32)
    vox[..., 0] = np.float32(-0.01).view(np.uint32)
    vox[:, :2048, 0] = np.float32(0.01).view(np.uint32)
    unobserved = Layer(hip, voxel, capacity_blocks=64)
    unobserved.upload(idx, vox)
    assert MeshLayer.from_layer(hip, unobserved).n_triangles == 0
    vox[..., 1] = np.float32(3.0).view(np.uint32)
    unobserved.upload(idx, vox)
    assert MeshLayer.from_layer(hip, unobserved).n_triangles > 0
    assert MeshLayer.from_layer(hip, unobserved, min_weight=3.0).n_triangles == 0
    assert MeshLayer.from_layer(hip, layer, min_weight=1e9).n_triangles == 0


def test_global_mesh_of_two_submaps_is_transform_plus_concatenation(hip, submap):
    voxel, layer = submap
    other, _, _ = run_frames(hip, method="merged", voxel=voxel, frames=range(70, 150, 10), subsample=4, capacity_blocks=8192)
    th = np.radians(3.0)
    T = [np.array([np.cos(th / 2), 0, 0, np.sin(th / 2), 0.07, -0.03, 0.01], np.float32),
         np.array([1, 0, 0, 0, 0.0, 0.0, 0.0], np.float32)]
    parts = [MeshLayer.from_layer(hip, layer, 1.0), MeshLayer.from_layer(hip, other, 1.0)]
    thr = 0.5 * voxel
    got = MeshLayer.connected(hip, parts, np.stack(T), thr)
    # Python composition: every part moved by transform(), concatenated, welded with the same cell rule in numpy
    moved = [MeshLayer.from_layer(hip, layer, 1.0), MeshLayer.from_layer(hip, other, 1.0)]
    for mm, t in zip(moved, T):
        mm.transform(t)
    cat = {k: np.concatenate([mm.download()[k] for mm in moved]) for k in ("xyz", "normals", "rgb")}
    weld = mesh_ref.weld_ref(cat["xyz"], cat["normals"], cat["rgb"], thr)
    survivors = weld["survivors"]
    assert np.array_equal(_bits(got["xyz"]), _bits(cat["xyz"][survivors]))
    assert np.array_equal(_bits(got["normals"]), _bits(cat["normals"][survivors]))
    assert np.array_equal(got["rgb"], cat["rgb"][survivors])
    assert np.array_equal(got["triangles"].reshape(-1), weld["triangles"].reshape(-1))
    # the rotation reached the normals: R n, still unit length where the triangle was not degenerate
    nn = np.linalg.norm(got["normals"], axis=1)
    assert np.all((np.abs(nn - 1) < 1e-5) | (nn == 0))


def test_cpp_mesh_flow_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "mesh_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mesh_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    g = mesh_io.read_ply(str(tmp_path / "global_mesh.ply"))
    s = mesh_io.read_ply(str(tmp_path / "submap0_mesh.ply"))
    assert len(g["triangles"]) > 1000 and g["triangles"].max() < len(g["xyz"])
    assert len(s["xyz"]) < len(g["xyz"]) and s["triangles"].max() < len(s["xyz"])
