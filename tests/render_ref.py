"""Loader of the test-side render reference (tests/cpp/render_reference.cpp), built with the checker's float flags, and the
hand-built layers and poses the CPU and GPU render tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

from coxgraph_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "render_reference.cpp")
R_HIT, R_NORMAL, R_COLOR, R_BUDGET = 1, 2, 4, 8
DEFAULTS = dict(min_depth=0.1, max_depth=10.0, step_scale=0.75, min_step_voxels=0.25, max_samples=4096)


class Config(C.Structure):
    _fields_ = [("min_depth", C.c_float), ("max_depth", C.c_float), ("step_scale", C.c_float), ("min_step_voxels", C.c_float),
                ("max_samples", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("n_samples", C.c_uint64), ("n_block_skips", C.c_uint64), ("n_budget", C.c_uint64), ("seconds", C.c_double)]


def build(out_dir):
    lib = os.path.join(str(out_dir), "librenderref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-o", lib, SRC])
    return RenderRef(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class RefLayer:
    """An oracle Layer rebuilt from wire arrays (Layer.download())."""

    def __init__(self, ref, voxel_size, idx, vox):
        self.ref = ref
        idx = np.ascontiguousarray(idx, np.int32)
        vox = np.ascontiguousarray(vox, np.uint32)
        self.h = C.c_void_p(ref.lib.render_ref_build(C.c_float(voxel_size), C.c_uint64(len(idx)), _p(idx), _p(vox)))

    def __del__(self):
        if getattr(self, "h", None):
            self.ref.lib.render_ref_free(self.h)
            self.h = None

    def render(self, T_G_C, w, h, K=None, **cfg):
        """cox_layer_render's semantics -> dict(depth[h,w], normal[h,w,3], rgba[h,w,4], status[h,w], samples[h,w], stats)."""
        T = np.ascontiguousarray(T_G_C, np.float32)
        K = np.ascontiguousarray(synth.INTRINSICS[(w, h)] if K is None else K, np.float32)
        c = Config(**{**DEFAULTS, **cfg})
        out = dict(depth=np.empty((h, w), np.float32), normal=np.empty((h, w, 3), np.float32), rgba=np.empty((h, w, 4), np.uint8),
                   status=np.empty((h, w), np.uint8), samples=np.empty((h, w), np.uint32))
        s = Stats()
        self.ref.lib.render_ref_render(self.h, _p(T), C.c_int(w), C.c_int(h), _p(K), C.byref(c), _p(out["depth"]), _p(out["normal"]), _p(out["rgba"]),
                                       _p(out["status"]), _p(out["samples"]), C.byref(s))
        out["stats"] = dict(n_hits=int(s.n_hits), n_samples=int(s.n_samples), n_block_skips=int(s.n_block_skips), n_budget=int(s.n_budget),
                            seconds=float(s.seconds))
        return out


class RenderRef:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.render_ref_build.restype = C.c_void_p
        self.lib.render_ref_render.restype = None

    def layer(self, voxel_size, idx, vox):
        return RefLayer(self, voxel_size, idx, vox)


# ---- poses ---------------------------------------------------------------------------------------------------------------------
def look_at_pose(origin, target):
    """(R_G_C float64, origin float64, T_G_C float32[7]) of a camera at origin whose optical axis (z) points at target, image
    x horizontal."""
    origin, target = np.asarray(origin, np.float64), np.asarray(target, np.float64)
    z = target - origin
    z /= np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)
    return R, origin, np.concatenate([synth.quat_from_matrix(R), origin]).astype(np.float32)


def scaled_intrinsics(w, h):
    """K of a w x h image that covers the field of view of the 640 x 480 one."""
    fx, fy, cx, cy = synth.INTRINSICS[(640, 480)]
    sx, sy = w / 640.0, h / 480.0
    return np.array([fx * sx, fy * sy, cx * sx, cy * sy], np.float32)


def analytic_depth(R, origin, w, h, K):
    """synth.render_depth for any intrinsics: the analytic z-depth of the room and the sphere."""
    key = (w, h)
    saved = synth.INTRINSICS.get(key)
    synth.INTRINSICS[key] = tuple(float(k) for k in K)
    try:
        return synth.render_depth(R, origin, w, h)
    finally:
        if saved is None:
            del synth.INTRINSICS[key]
        else:
            synth.INTRINSICS[key] = saved


# ---- hand-built layers -----------------------------------------------------------------------------------------------------------
def voxel_centres(idx, voxel_size):
    """Centres of every voxel of the blocks idx [n,3], float32 [n,4096,3]: block_index * block_size + (v + 0.5) * voxel_size."""
    vs = np.float32(voxel_size)
    bs = vs * np.float32(16)
    lin = np.arange(4096)
    v = np.stack([lin & 15, (lin >> 4) & 15, lin >> 8], 1).astype(np.float32)
    origin = np.asarray(idx, np.float32)[:, None, :] * bs
    return origin + (v[None] + np.float32(0.5)) * vs


def field_layer_arrays(voxel_size, idx, field, trunc=None, color=None):
    """Wire arrays (idx, words) of the blocks idx holding d = field(centres) (float64 in, rounded once), weight 1."""
    idx = np.asarray(idx, np.int32)
    c = voxel_centres(idx, voxel_size).astype(np.float64)
    d = field(c.reshape(-1, 3)).reshape(c.shape[:2])
    if trunc is not None:
        d = np.clip(d, -trunc, trunc)
    words = np.zeros((len(idx), 4096, 3), np.uint32)
    words[..., 0] = d.astype(np.float32).view(np.uint32)
    words[..., 1] = np.float32(1.0).view(np.uint32)
    if color is not None:
        words[..., 2] = color
    return idx, words


# The plane z = 1.5 seen from below in one block of 0.125 m voxels (block edge 2 m): d = 1.5 - z at every centre, untruncated.
# Every number of the central ray is a short binary fraction, so float32 carries the march without rounding.
PLANE_VS, PLANE_Z = 0.125, 1.5
PLANE_K = np.array([64.0, 64.0, 4.0, 4.0], np.float32)   # 9 x 9 image, central pixel (4, 4)
PLANE_T = np.array([1, 0, 0, 0, 1.0625, 1.0625, 0.0], np.float32)  # camera axes = world axes, on a voxel centre line, looking along +z


def plane_layer_arrays():
    color = np.uint32(255 | (30 << 8) | (20 << 16) | (10 << 24))  # wire word a | b << 8 | g << 16 | r << 24: r, g, b, a = 10, 20, 30, 255
    return field_layer_arrays(PLANE_VS, [(0, 0, 0)], lambda c: PLANE_Z - c[:, 2], color=color)


def sphere_layer_arrays(voxel_size, centre, radius, blocks=2, trunc=None):
    idx = [(x, y, z) for z in range(blocks) for y in range(blocks) for x in range(blocks)]
    return field_layer_arrays(voxel_size, idx, lambda c: np.linalg.norm(c - centre, axis=1) - radius, trunc=trunc)


def error_in_voxels(depth, truth, voxel):
    """(share of pixels hit among those with a finite analytic depth, median and 95th percentile of |depth - truth| / voxel)."""
    want = np.isfinite(truth)
    hit = np.isfinite(depth) & want
    err = np.abs(depth[hit].astype(np.float64) - truth[hit].astype(np.float64)) / voxel
    return float(hit.sum() / max(1, want.sum())), float(np.median(err)), float(np.quantile(err, 0.95))
