"""Loader of the test-side mesh reference (tests/cpp/mesh_reference.cpp), built with the checker's float flags."""
import ctypes as C
import os
import subprocess

import numpy as np

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
