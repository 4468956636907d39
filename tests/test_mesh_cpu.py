"""The mesher's C ABI (include/coxgraph_hip_mesh.h), the PLY writer and the mesh reference's colour modes -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

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
