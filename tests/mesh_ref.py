"""Loader of the test-side mesh reference (tests/cpp/mesh_reference.cpp), built with the checker's float flags, and the pieces
the C++ reference does not cover, restated in numpy from DESIGN.md section 7d: the weld, the wire encoding of any position, a
rigid transform in float64, and counts of what a reference mesh holds (which rules of the colour lookup its vertices reach)."""
import ctypes as C
import os
import subprocess

import numpy as np

from layer_cases import rotation_matrix

F = np.float32
K_EPS = F(1e-6)


class IndexRange(ValueError):
    """The weld's cells span 2^21 or more on an axis (COX_ERR_INDEX_RANGE)."""


def c_round(x):
    """C's round(): to nearest, halves away from zero (|x| - floor|x| is exact in float64)"""
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(f + (a - f >= 0.5), x)


def weld_ref(xyz, nrm, rgb, threshold):
    """createConnectedMesh: cell = round(double(p) * (1 / double(float(threshold)))) per axis; the first vertex in mesh order
    owns its cell and keeps position, normal and colour; survivors stay in mesh order; every input vertex is replaced by its
    survivor.  -> dict(xyz, normals, rgb, triangles uint32[nt, 3], survivors: input index of each output vertex)."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    if len(xyz) == 0:
        return dict(xyz=xyz, normals=np.zeros((0, 3), F), rgb=np.zeros((0, 3), np.uint8), triangles=np.zeros((0, 3), np.uint32),
                    survivors=np.zeros(0, np.int64))
    cells = c_round(xyz.astype(np.float64) * (1.0 / np.float64(F(threshold)))).astype(np.int64)
    if np.any(cells.max(axis=0) - cells.min(axis=0) >= 1 << 21):
        raise IndexRange(cells.max(axis=0) - cells.min(axis=0))
    rel = cells - cells.min(axis=0)             # 21 bits per axis: one integer per cell
    _, first, inv = np.unique(rel[:, 0] | (rel[:, 1] << 21) | (rel[:, 2] << 42), return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    survivors = first[order]
    return dict(xyz=xyz[survivors], normals=np.asarray(nrm)[survivors], rgb=np.asarray(rgb)[survivors],
                triangles=rank[inv.reshape(-1)].astype(np.uint32).reshape(-1, 3), survivors=survivors)


def encode_ref(xyz, block_index_per_vertex, edge):
    """generateVoxbloxMeshMsg's coordinates in float32: q = (p / edge - float(index)) / (2.0f / 65535), 0 for !(q > 0), 65535
    for q >= 65535, else truncated -> uint16[n, 3]"""
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    q = (p / F(edge) - np.asarray(block_index_per_vertex).astype(F)) / (F(2.0) / F(65535.0))
    out = np.zeros(q.shape, np.uint16)
    mid = (q > 0) & (q < F(65535.0))
    out[mid] = q[mid].astype(np.uint16)     # truncation: q is positive here
    out[q >= F(65535.0)] = 65535
    return out


def transform_ref(xyz, nrm, T):
    """T p and R n in float64, T = qw qx qy qz tx ty tz as the float32 values the engine is given"""
    T = np.asarray(T, F).astype(np.float64)
    R = rotation_matrix(T[:4])
    return np.asarray(xyz, np.float64) @ R.T + T[4:], np.asarray(nrm, np.float64) @ R.T


def per_vertex_block(mesh):
    return np.repeat(mesh["block_index"], np.diff(mesh["vertex_begin"].astype(np.int64)), axis=0)


def colour_rule_counts(mesh, idx, voxel):
    """What the vertices of a reference mesh reach, in the float32 arithmetic of section 7d's colour rule: dict(outside: not in
    a voxel of their own block; midpoint: a coordinate equal to the midpoint 0.5f * (c + (c + voxel)) of two neighbouring corner
    samples, i.e. on a voxel boundary; zero_normal; missing: outside and the block found by coordinates not in idx; clamped_low /
    clamped_high: outside, not missing, and the voxel index within the block found by coordinates below 0 / above 15 on an axis)."""
    v, b = mesh["xyz"], per_vertex_block(mesh)
    vs = F(voxel)
    vs_inv, bs = F(1.0 / np.float64(vs)), vs * F(16)
    bs_inv = F(1.0 / np.float64(bs))
    o = b.astype(F) * bs
    s = np.floor((v - o) * vs_inv + K_EPS)
    outside = np.any((s < 0) | (s >= 16), axis=1)
    c = o[:, :, None] + (np.arange(16, dtype=F) + F(0.5))[None, None, :] * vs      # lower corner sample of cube 0..15 per axis
    mid = F(0.5) * (c + (c + vs))
    midpoint = np.any(v[:, :, None] == mid, axis=(1, 2))
    bb = np.floor(v * bs_inv + K_EPS).astype(np.int64)

    def key(a):
        a = np.asarray(a, np.int64) + (1 << 20)
        return a[:, 0] | (a[:, 1] << 21) | (a[:, 2] << 42)
    missing = outside & ~np.isin(key(bb), key(np.asarray(idx).reshape(-1, 3)))
    rel = np.floor((v - bb.astype(F) * bs) * vs_inv + K_EPS)
    low, high = outside & ~missing & np.any(rel < 0, axis=1), outside & ~missing & np.any(rel >= 16, axis=1)
    return dict(clamped_low=int(low.sum()), clamped_high=int(high.sum()), outside=int(outside.sum()), midpoint=int(midpoint.sum()), zero_normal=int(np.all(mesh["normals"] == 0, axis=1).sum()),
                missing=int(missing.sum()))


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mesh_reference.cpp")
MODES = ("color", "normals", "gray", "lambert", "lambert_color")


def build(out_dir):
    lib = os.path.join(str(out_dir), "libmeshref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-o", lib, SRC])
    return MeshRef(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class MeshRef:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.mesh_ref_build.restype = C.c_void_p

    def mesh(self, voxel_size, idx, vox, min_weight):
        """Mesh of the wire arrays (Layer.download()) -> dict as MeshLayer.download() plus n_missing, seconds, and msg(mode)."""
        idx = np.ascontiguousarray(idx, np.int32)
        vox = np.ascontiguousarray(vox, np.uint32)
        h = C.c_void_p(self.lib.mesh_ref_build(C.c_float(voxel_size), C.c_uint64(len(idx)), _p(idx), _p(vox), C.c_float(min_weight)))
        try:
            nb, nv, nm, sec = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
            self.lib.mesh_ref_size(h, C.byref(nb), C.byref(nv), C.byref(nm), C.byref(sec))
            nb, nv = int(nb.value), int(nv.value)
            out = dict(block_index=np.zeros((nb, 3), np.int32), vertex_begin=np.zeros(nb + 1, np.uint64), xyz=np.zeros((nv, 3), np.float32),
                       normals=np.zeros((nv, 3), np.float32), rgb=np.zeros((nv, 3), np.uint8))
            self.lib.mesh_ref_get(h, *[_p(out[k]) for k in ("block_index", "vertex_begin", "xyz", "normals", "rgb")])
            out["n_missing"], out["seconds"] = int(nm.value), float(sec.value)
            edge = np.float32(voxel_size) * np.float32(16)
            out["msg"] = {}
            for m, name in enumerate(MODES):
                a = {k: np.zeros(nv, np.uint16) for k in "xyz"}
                a.update({k: np.zeros(nv, np.uint8) for k in "rgb"})
                self.lib.mesh_ref_msg(h, C.c_float(edge), C.c_int(m), *[_p(a[k]) for k in "xyzrgb"])
                out["msg"][name] = a
            return out
        finally:
            self.lib.mesh_ref_free(h)
