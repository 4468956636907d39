"""Loader of the test-side map-query reference (tests/cpp/map_reference.cpp), built with the checker's float flags."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_reference.cpp")
MODES = {"nearest": 0, "interpolate": 1, "adaptive": 2}


def build(out_dir):
    lib = os.path.join(str(out_dir), "libmapref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-o", lib, SRC])
    return MapRef(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class RefLayer:
    """An oracle Layer rebuilt from wire arrays (Layer.download())."""

    def __init__(self, ref, voxel_size, idx, vox):
        self.ref = ref
        idx = np.ascontiguousarray(idx, np.int32)
        vox = np.ascontiguousarray(vox, np.uint32)
        self.h = C.c_void_p(ref.lib.map_ref_build(C.c_float(voxel_size), C.c_uint64(len(idx)), _p(idx), _p(vox)))

    def __del__(self):
        if getattr(self, "h", None):
            self.ref.lib.map_ref_free(self.h)
            self.h = None

    def query(self, xyz, mode="interpolate", gradient=False):
        """cox_layer_query's semantics -> dict(distance, weight, [gradient,] status, seconds); NaN where a status bit is clear."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        out = dict(distance=np.full(n, np.nan, np.float32), weight=np.full(n, np.nan, np.float32), status=np.zeros(n, np.uint8))
        g = np.full((n, 3), np.nan, np.float32) if gradient else None
        sec = self.ref.lib.map_ref_query(self.h, _p(xyz), C.c_uint64(n), C.c_int(MODES[mode]), C.c_int(int(gradient)), _p(out["distance"]),
                                         _p(out["weight"]), _p(g) if gradient else None, _p(out["status"]))
        if gradient:
            out["gradient"] = g
        out["seconds"] = float(sec)
        return out

    def free_points(self, min_distance):
        """createFreePointcloudFromEsdfLayer -> (xyz float32[n,3], intensity float32[n]) in cox_layer_free_points' order."""
        n = int(self.ref.lib.map_ref_free_points(self.h, C.c_float(min_distance), None, None))
        xyz, inten = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        if n:
            self.ref.lib.map_ref_free_points(self.h, C.c_float(min_distance), _p(xyz), _p(inten))
        return xyz, inten


class MapRef:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.map_ref_build.restype = C.c_void_p
        self.lib.map_ref_query.restype = C.c_double
        self.lib.map_ref_free_points.restype = C.c_uint64

    def layer(self, voxel_size, idx, vox):
        return RefLayer(self, voxel_size, idx, vox)


# ---- hand-built layers shared by the CPU and GPU tests -------------------------------------------------------------------
AFFINE_A, AFFINE_C, AFFINE_VS = np.array([0.3, -0.7, 0.5], np.float32), np.float32(0.1), np.float32(0.1)


def voxel_centres(idx, voxel_size):
    """Centres of every voxel of the blocks idx [n,3], float32 [n,4096,3]: block_index * block_size + (v + 0.5) * voxel_size."""
    vs = np.float32(voxel_size)
    bs = vs * np.float32(16)
    lin = np.arange(4096)
    v = np.stack([lin & 15, (lin >> 4) & 15, lin >> 8], 1).astype(np.float32)
    origin = np.asarray(idx, np.float32)[:, None, :] * bs
    return origin + (v[None] + np.float32(0.5)) * vs


def affine_layer_arrays():
    """2 x 2 x 2 blocks at 0.1 m holding d = a . x + c at every voxel centre, weight 1: wire arrays (idx, words)."""
    idx = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.int32)
    c = voxel_centres(idx, AFFINE_VS).astype(np.float64)
    d = (c @ AFFINE_A.astype(np.float64) + np.float64(AFFINE_C)).astype(np.float32)
    words = np.zeros((len(idx), 4096, 3), np.uint32)
    words[..., 0] = d.view(np.uint32)
    words[..., 1] = np.float32(1.0).view(np.uint32)
    return idx, words


def affine_queries(rng, n=4000):
    """Points of the affine layer whose gradient samples all lie inside it: uniform, exactly on the block faces (1.6 m) and
    on voxel centres."""
    lo, hi = 0.16, 3.04
    u = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    face = rng.uniform(lo, hi, size=(n // 4, 3)).astype(np.float32)
    face[np.arange(len(face)), rng.integers(0, 3, len(face))] = np.float32(16) * AFFINE_VS
    cen = ((rng.integers(2, 30, size=(n // 4, 3)).astype(np.float32) + np.float32(0.5)) * AFFINE_VS).astype(np.float32)
    return np.concatenate([u, face, cen])
