"""The mesher's C ABI (include/coxgraph_hip_mesh.h), the PLY writer, the mesh reference's colour modes, and what the seeded cases of
tests/mesh_cases.py reach on the reference alone -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_cases
import mesh_ref
from coxgraph_amd import mesh_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_mesh_symbols():
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_mesh.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def test_mesh_header_symbols_are_exported(hip):
    syms = _declared_mesh_symbols()
    assert len(syms) >= 12 and "cox_meshlayer_from_layer" in syms and "cox_meshlayer_connected" in syms
    missing = [s for s in syms if not hasattr(hip.lib, s)]
    assert not missing, missing


def test_mesh_entry_points_fail_cleanly(hip):
    """NULL handles / outputs -> COX_ERR_INVALID_ARG; a call that needs a device gets COX_ERR_NO_DEVICE without one."""
    f = hip.fn
    u = C.c_uint64()
    h = C.c_void_p()
    T = (C.c_float * 7)(1, 0, 0, 0, 0, 0, 0)
    buf = (C.c_uint16 * 4)()
    cbuf = (C.c_uint8 * 4)()
    assert f("meshlayer_from_layer")(None, C.c_float(1.0), C.byref(h), None, None) == -1
    assert f("meshlayer_size")(None, C.byref(u), None, None) == -1
    assert f("meshlayer_stats")(None, None, None) == -1
    assert f("meshlayer_download")(None, None, None, None, None, None, C.c_uint64(0), C.c_uint64(0)) == -1
    assert f("meshlayer_data_dev")(None, None, None, None, None) == -1
    assert f("meshlayer_transform")(None, T) == -1
    assert f("meshlayer_msg")(None, C.c_int(0), buf, buf, buf, cbuf, cbuf, cbuf, C.c_uint64(4)) == -1
    assert f("meshlayer_connected")(None, None, C.c_uint64(1), C.c_float(0.01), C.byref(h), None, None) == -1
    assert f("meshlayer_connected")(None, None, C.c_uint64(0), C.c_float(0.01), None, None, None) == -1
    assert f("meshlayer_connected")(None, None, C.c_uint64(0), C.c_float(0.0), C.byref(h), None, None) == -1
    assert f("meshconn_size")(None, C.byref(u), None) == -1
    assert f("meshconn_download")(None, None, None, None, None, C.c_uint64(0), C.c_uint64(0)) == -1
    f("meshlayer_destroy", None)(None)
    f("meshconn_destroy", None)(None)
    # an empty connected mesh lives on the current device: the one call that needs nothing but a GPU
    st = f("meshlayer_connected")(None, None, C.c_uint64(0), C.c_float(0.01), C.byref(h), C.byref(u), None)
    if hip.device_count() == 0:
        assert st == -2
    else:
        assert st == 0 and u.value == 0
        f("meshconn_destroy", None)(h)


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    xyz = rng.normal(size=(50, 3)).astype(np.float32)
    nrm = rng.normal(size=(50, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    tri = rng.integers(0, 50, size=(70, 3)).astype(np.uint32)
    p = str(tmp_path / "m.ply")
    mesh_io.write_ply(p, xyz, tri, nrm, rgb)
    back = mesh_io.read_ply(p)
    assert np.array_equal(back["xyz"], xyz) and np.array_equal(back["normals"], nrm)
    assert np.array_equal(back["rgb"], rgb) and np.array_equal(back["triangles"], tri)
    head = open(p, "rb").read(40)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    # 9 header lines of properties + 27 bytes per vertex + 13 per face
    assert os.path.getsize(p) == open(p, "rb").read().index(b"end_header\n") + 11 + 50 * 27 + 70 * 13
    mesh_io.write_ply(p, np.zeros((0, 3)), np.zeros((0, 3)))
    e = mesh_io.read_ply(p)
    assert e["xyz"].shape == (0, 3) and e["triangles"].shape == (0, 3)
    with pytest.raises(ValueError):
        mesh_io.write_ply(p, xyz, [[0, 1, 50]])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("meshref"))


def _plane_layer(z0=2.0, voxel=0.5, weight=2.0, rgb=(255, 0, 0)):
    """One block whose TSDF is the plane z = z0 (positive above), every voxel coloured rgb."""
    lin = np.arange(4096)
    zc = ((lin >> 8) + 0.5) * voxel
    d = (zc - z0).astype(np.float32)
    w = np.full(4096, weight, np.float32)
    c = np.uint32(255) | (np.uint32(rgb[2]) << 8) | (np.uint32(rgb[1]) << 16) | (np.uint32(rgb[0]) << 24)
    vox = np.stack([d.view(np.uint32), w.view(np.uint32), np.full(4096, c, np.uint32)], -1)[None]
    return np.zeros((1, 3), np.int32), vox


def test_colour_modes_by_hand(ref):
    """The plane z = 2 (voxel 0.5 m, block edge 8 m): every triangle lies in it, its normal is exactly (0, 0, 1) (towards the
    positive side) and each vertex sits at z = 2 exactly.  Values below are worked out by hand from DESIGN.md section 7d."""
    idx, vox = _plane_layer()
    m = ref.mesh(0.5, idx, vox, 1.0)
    nv = len(m["xyz"])
    # the 15 x 15 inside cubes across the plane, two triangles each (the max-plane cubes need neighbour blocks: none here)
    assert nv == 3 * 2 * 15 * 15 and m["n_missing"] == 0
    assert np.all(m["xyz"][:, 2] == 2.0)
    assert np.array_equal(m["normals"], np.tile(np.float32([0, 0, 1]), (nv, 1)))
    assert np.all(m["rgb"] == [255, 0, 0])
    msg = m["msg"]
    # z: (2 / 8 - 0) / (2 / 65535) = 8191.875 -> 8191
    for mode in mesh_ref.MODES:
        assert np.all(msg[mode]["z"] == 8191)
    def rgb_of(mode):
        return np.stack([msg[mode][k] for k in "rgb"], 1)
    assert np.all(rgb_of("color") == [255, 0, 0])
    assert np.all(rgb_of("normals") == [127, 127, 255])       # (0 * .5 + .5) * 255 = 127.5 -> 127; (1 * .5 + .5) * 255 = 255
    assert np.all(rgb_of("gray") == [127, 127, 127])          # 0.5 * 255 = 127.5 -> 127
    # lights: l1 = (0.8, -0.2, 0.7) / sqrt(1.17), l2 = (-0.5, 0.2, 0.2) / sqrt(0.33); n = z: d1 = 0.647150, d2 = 0.348155
    # lambert:       (0.647150 * 0.5 + 0.348155 * 0.5) + 0.2 = 0.697653 -> 177.9 -> 177
    # lambert_color: red (0.647150 + 0.348155) + 0.2 = 1.195 -> 1 -> 255; green / blue 0.2 -> 51
    assert np.all(rgb_of("lambert") == [177, 177, 177])
    assert np.all(rgb_of("lambert_color") == [255, 51, 51])
    # colour only from voxels above min_weight: at min_weight = weight every corner is invalid, nothing is meshed
    assert len(ref.mesh(0.5, idx, vox, 2.0)["xyz"]) == 0


def test_mesh_smoke_compiles_and_reports_no_gpu(hip, tmp_path):
    exe = str(tmp_path / "mesh_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mesh_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    rc = subprocess.call([exe, str(tmp_path)])
    assert rc == (0 if hip.device_count() > 0 else 77)


# ---- the seeded cases of tests/mesh_cases.py reach what they claim, on the reference alone ----------------------------------
WITH_FACE_NEIGHBOURS = ("full", "subset70", "slab", "two_components")


@pytest.fixture(scope="module")
def family_meshes(ref):
    """the reference mesh and its coverage counts of every pinned case, computed once"""
    out = {}
    for seed, fam in mesh_cases.FAMILY_CASES + [mesh_cases.EXTREME_CASE, mesh_cases.FACE_CASE]:
        voxel, idx, vox, min_w, meta = mesh_cases.case(seed, fam)
        m = ref.mesh(voxel, idx, vox, min_w)
        out[seed] = (meta, m, mesh_ref.colour_rule_counts(m, idx, voxel))
        print(seed, fam, f"voxel {voxel} min_weight {min_w}: {len(idx)} blocks, {len(m['xyz']) // 3} triangles, {out[seed][2]}, {m['seconds'] * 1e3:.0f} ms")
    return out


def test_family_cases_cover_every_field_origin_and_build():
    fams = [f for _, f in mesh_cases.FAMILY_CASES]
    assert {f[0] for f in fams} == set(mesh_cases.FIELDS) and {f[1] for f in fams} == set(mesh_cases.BLOCK_SETS)
    assert {f[2] for f in fams} == {"near", "far"} and {f[3] for f in fams} == set(mesh_cases.BUILDS)
    assert mesh_cases.EXTREME_CASE[1][2] == "extreme"
    assert len({s for s, _ in mesh_cases.FAMILY_CASES}) == len(fams)
    drawn = [mesh_cases.case(s)[4] for s in range(24)]
    assert all(d["lo"] != "extreme" for d in drawn) and {d["lo"] for d in drawn} == {"near", "far"}
    for seed in (0, 7):     # a case is a function of its seed
        a, b = mesh_cases.case(seed), mesh_cases.case(seed)
        assert a[0] == b[0] and a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert all(len(mesh_cases.case(s)[1]) <= mesh_cases.MAX_BLOCKS for s in range(24))


def test_family_cases_yield_surface(family_meshes):
    for seed, (meta, m, _) in family_meshes.items():
        assert len(m["xyz"]) % 3 == 0 and m["seconds"] < 0.1, seed
        if meta["blocks"] in WITH_FACE_NEIGHBOURS:
            assert len(m["xyz"]) // 3 >= 1000, (seed, meta)


def test_far_case_has_degenerate_triangles(family_meshes):
    meta, _, c = family_meshes[mesh_cases.FAR_CASE[0]]
    assert meta["lo"] == "far" and c["zero_normal"] >= 20, c


def test_tiny_case_puts_vertices_on_voxel_boundaries(family_meshes):
    meta, _, c = family_meshes[mesh_cases.TINY_CASE[0]]
    assert meta["field"] == "tiny" and c["midpoint"] >= 100, c
    for a, b in mesh_cases.exact_diff_pairs():      # 1e-6f itself, the float above and the float below
        assert a > 0 > b
    diffs = [np.float32(a - b) for a, b in mesh_cases.exact_diff_pairs()]
    t = np.float32(1e-6)
    assert diffs == [t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))]


def test_face_cases_reach_both_voxel_clamps(family_meshes):
    """A vertex on a block face, thousands of blocks out: the block found by coordinates and the block whose voxel range holds
    it can differ by one, and the voxel index is clamped into the block found -- from -1 in the far tiny case, from 16 in the
    pinned face case (block indices found by search: see mesh_cases.origin)."""
    meta, _, c = family_meshes[mesh_cases.FAR_TINY_CASE[0]]
    assert (meta["field"], meta["lo"]) == ("tiny", "far") and c["clamped_low"] >= 30, c
    meta, m, c = family_meshes[mesh_cases.FACE_CASE[0]]
    assert meta["voxel"] == 0.08 and c["clamped_high"] >= 1000 and m["n_missing"] == 0, c


def test_noise_cases_put_vertices_outside_their_block(family_meshes):
    """A vertex outside its own block comes from a cube across the block's +x / +y / +z face, so the block sets without face
    neighbours (edges_only, corners_only, single) cannot have one: the bar is for the other four."""
    seen = 0
    for seed, (meta, _, c) in family_meshes.items():
        if meta["field"] == "noise" and meta["blocks"] in WITH_FACE_NEIGHBOURS:
            assert c["outside"] >= 1000, (seed, meta, c)
            seen += 1
        elif meta["field"] == "noise":
            assert c["outside"] == 0, (seed, meta, c)
    assert seen >= 4


def test_missing_colour_only_in_the_extreme_case(family_meshes):
    for seed, (meta, m, c) in family_meshes.items():
        assert c["missing"] == m["n_missing"], (seed, c, m["n_missing"])      # the numpy restatement of the rule and the reference
        if meta["lo"] == "extreme":
            assert m["n_missing"] >= 1
        else:
            assert m["n_missing"] == 0, (seed, meta)


def test_threshold_case_straddles_both_min_weights(ref):
    voxel, idx, vox, _, meta = mesh_cases.case(*mesh_cases.THRESHOLD_CASE)
    assert meta["field"] == "threshold"
    w = vox[..., 1].view(np.float32)
    for v in mesh_cases.threshold_values():
        assert np.count_nonzero(w == v) > 100, v
    strict, loose = (len(ref.mesh(voxel, idx, vox, mw)["xyz"]) for mw in (1.0, 1e-4))
    assert 0 < strict < loose
    # a weight equal to min_weight is invalid: raising those voxels by one ulp adds cubes
    for mw in mesh_cases.MIN_WEIGHTS:
        up = vox.copy()
        wu = up[..., 1].view(np.float32)
        wu[wu == np.float32(mw)] = np.nextafter(np.float32(mw), np.float32(2))
        up[..., 1] = wu.view(np.uint32)
        assert len(ref.mesh(voxel, idx, up, mw)["xyz"]) > len(ref.mesh(voxel, idx, vox, mw)["xyz"]), mw


def test_weld_ref_by_hand():
    """Nine vertices, threshold 0.5 (cells = round(2 p), halves away from zero):
         0 (-0.25, -1.0,  0.3 ) -> (-1, -2, 1)   -0.5 is a tie: away from zero, not floor(x + 0.5) = 0
         1 (-0.3,  -1.1,  0.26) -> (-1, -2, 1)   welded into 0
         2 ( 0.25,  0.0,  0.0 ) -> ( 1,  0, 0)   +0.5 ties up
         3 ( 0.0,   0.0,  0.0 ) -> ( 0,  0, 0)
         4 ( 0.26,  0.1, -0.1 ) -> ( 1,  0, 0)   welded into 2 (-0.2 rounds to -0)
         5 (-0.2,  -0.2, -0.2 ) -> ( 0,  0, 0)   welded into 3
         6 (-0.75,  0.0,  0.0 ) -> (-2,  0, 0)   -1.5 is a tie: -2
         7 (-0.74,  0.0,  0.0 ) -> (-1,  0, 0)
         8 (-0.25, -1.0,  0.3 ) -> cell of 0
       survivors in mesh order 0 2 3 6 7; triangles (0 0 1) (2 1 2) (3 4 0)."""
    xyz = np.float32([[-0.25, -1.0, 0.3], [-0.3, -1.1, 0.26], [0.25, 0, 0], [0, 0, 0], [0.26, 0.1, -0.1], [-0.2, -0.2, -0.2], [-0.75, 0, 0],
                      [-0.74, 0, 0], [-0.25, -1.0, 0.3]])
    nrm = np.arange(27, dtype=np.float32).reshape(9, 3)
    rgb = np.arange(27, dtype=np.uint8).reshape(9, 3)
    w = mesh_ref.weld_ref(xyz, nrm, rgb, 0.5)
    assert w["survivors"].tolist() == [0, 2, 3, 6, 7]
    assert w["triangles"].tolist() == [[0, 0, 1], [2, 1, 2], [3, 4, 0]] and w["triangles"].dtype == np.uint32
    assert np.array_equal(w["xyz"], xyz[[0, 2, 3, 6, 7]]) and np.array_equal(w["normals"], nrm[[0, 2, 3, 6, 7]]) and np.array_equal(w["rgb"], rgb[[0, 2, 3, 6, 7]])
    assert mesh_ref.c_round(np.array([-0.5, 0.5, -1.5, 2.5, -0.49999999999999994, 0.49999999999999994, -0.0])).tolist() == [-1, 1, -2, 3, -0.0, 0, -0.0]
    # one cell for everything; a span of 2^21 cells is refused, one less is not
    assert mesh_ref.weld_ref(xyz, nrm, rgb, 1e6)["triangles"].tolist() == [[0, 0, 0]] * 3
    two = np.float32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [2097152.0, 0, 0], [0, 0, 0], [0, 0, 0]])
    with pytest.raises(mesh_ref.IndexRange):
        mesh_ref.weld_ref(two, two, np.zeros((6, 3), np.uint8), 1.0)
    two[3, 0] = 2097151.0
    assert len(mesh_ref.weld_ref(two, two, np.zeros((6, 3), np.uint8), 1.0)["xyz"]) == 2
    assert mesh_ref.weld_ref(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.uint8), 0.1)["triangles"].shape == (0, 3)


def test_encode_ref_by_hand(ref):
    """test_colour_modes_by_hand's z: (2 / 8 - 0) / (2 / 65535) = 8191.875 -> 8191; one block below the block's origin q is
    negative -> 0; two blocks above it q = 65535 -> the upper clamp; just below, (2 - 1.25e-5) * 32767.5 = 65534.6 -> 65534 and
    (2 - 1.25e-4) * 32767.5 = 65530.9 -> 65530"""
    edge = np.float32(8.0)
    got = mesh_ref.encode_ref(np.float32([[2.0, -8.0, 16.0], [0.0, 15.9999, 24.0 - 1e-3], [8.0, 8.0, 8.0]]), np.int32([[0, 0, 0], [0, 0, 1], [1, 1, 1]]), edge)
    assert got.tolist() == [[8191, 0, 65535], [0, 65534, 65530], [0, 0, 0]] and got.dtype == np.uint16
    idx, vox = _plane_layer()
    m = ref.mesh(0.5, idx, vox, 1.0)
    enc = mesh_ref.encode_ref(m["xyz"], mesh_ref.per_vertex_block(m), edge)
    assert np.all(enc[:, 2] == 8191)
    for i, k in enumerate("xyz"):
        assert np.array_equal(enc[:, i], m["msg"]["color"][k])


def test_transform_ref_by_hand():
    q = np.float32([np.sqrt(0.5), 0, 0, np.sqrt(0.5)])     # 90 degrees about z: x -> y, y -> -x
    p, n = mesh_ref.transform_ref([[1, 2, 3]], [[0, 1, 0]], np.concatenate([q, [10, 20, 30]]))
    assert np.allclose(p, [[8, 21, 33]], atol=1e-6) and np.allclose(n, [[-1, 0, 0]], atol=1e-6)
