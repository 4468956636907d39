"""Loader of the test-side collision reference (tests/cpp/collide_reference.cpp), built with the checker's float flags, and the
hand-built layers the CPU and GPU tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

import map_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "collide_reference.cpp")

C_TRAVERSABLE, C_OBSERVED, C_DISTANCE, C_CLEARED, C_INVALID = 1, 2, 4, 8, 16
SEG_FEASIBLE, SEG_GOAL, SEG_CLAMPED, SEG_TOO_LONG, SEG_INVALID = 1, 2, 4, 8, 16
TREE_KEEP, TREE_INVALID = 1, 2

RECORD_DTYPE = np.dtype([("n_samples", np.uint32), ("first_blocked", np.uint32), ("flags", np.uint32), ("free_length", np.float32),
                         ("goal", np.float32, 3), ("pad", np.uint32)])
assert RECORD_DTYPE.itemsize == 32


class Config(C.Structure):
    """cox_collide_config with the yaml's defaults (cox_collide_config_default)."""
    _fields_ = [("collision_radius", C.c_float), ("collision_optimistic", C.c_int32), ("clearing_radius", C.c_float), ("clearing_centre", C.c_float * 3),
                ("sample_spacing", C.c_float), ("max_samples", C.c_uint32), ("max_extension_range", C.c_float), ("crop", C.c_int32),
                ("crop_margin", C.c_float), ("crop_min_length", C.c_float)]


DEFAULTS = dict(collision_radius=2.0, collision_optimistic=0, clearing_radius=0.0, clearing_centre=(0.0, 0.0, 0.0), sample_spacing=0.05, max_samples=4096,
                max_extension_range=1.5, crop=1, crop_margin=0.3, crop_min_length=0.5)


def config(**cfg):
    c = Config()
    for k, v in {**DEFAULTS, **cfg}.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        if k == "clearing_centre":
            v = (C.c_float * 3)(*[float(x) for x in v])
        setattr(c, k, v)
    return c


def build(out_dir):
    lib = os.path.join(str(out_dir), "libcollideref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-o", lib, SRC])
    return CollideRef(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class RefLayer:
    """An oracle Layer rebuilt from wire arrays (Layer.download()), answering the rules of DESIGN.md section 7k."""

    def __init__(self, ref, voxel_size, idx, vox):
        self.ref = ref
        idx = np.ascontiguousarray(idx, np.int32)
        vox = np.ascontiguousarray(vox, np.uint32)
        self.h = C.c_void_p(ref.lib.collide_ref_build(C.c_float(voxel_size), C.c_uint64(len(idx)), _p(idx), _p(vox)))

    def __del__(self):
        if getattr(self, "h", None):
            self.ref.lib.collide_ref_free(self.h)
            self.h = None

    def points(self, xyz, **cfg):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        out = dict(state=np.zeros(len(xyz), np.uint8), distance=np.full(len(xyz), np.nan, np.float32))
        c = config(**cfg)
        self.ref.lib.collide_ref_points(self.h, C.byref(c), _p(xyz), C.c_uint64(len(xyz)), _p(out["state"]), _p(out["distance"]))
        return out

    def segments(self, a, b, **cfg):
        """records (RECORD_DTYPE) plus min_margin (the smallest |distance - collision_radius| over every sample), n_samples and seconds."""
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
        rec = np.zeros(len(a), RECORD_DTYPE)
        c = config(**cfg)
        margin, looked = C.c_float(), C.c_uint64()
        sec = self.ref.lib.collide_ref_segments(self.h, C.byref(c), _p(a), _p(b), C.c_uint64(len(a)), _p(rec), C.byref(margin), C.byref(looked))
        return dict(records=rec, min_margin=float(margin.value), n_samples=int(looked.value), seconds=float(sec))

    def trajectories(self, offsets, xyz, **cfg):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        rec = np.zeros(len(offsets) - 1, RECORD_DTYPE)
        c = config(**cfg)
        self.ref.lib.collide_ref_trajectories(self.h, C.byref(c), _p(offsets), C.c_uint64(len(offsets) - 1), _p(xyz), _p(rec))
        return rec


class CollideRef:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.collide_ref_build.restype = C.c_void_p
        self.lib.collide_ref_segments.restype = C.c_double
        self.lib.collide_ref_points.restype = None
        self.lib.collide_ref_trajectories.restype = None
        self.lib.collide_ref_prune.restype = None
        self.lib.collide_ref_free.restype = None

    def layer(self, voxel_size, idx, vox):
        return RefLayer(self, voxel_size, idx, vox)

    def prune(self, parent, feasible):
        parent = np.ascontiguousarray(parent, np.int32)
        feasible = np.ascontiguousarray(feasible, np.uint8)
        keep = np.zeros(len(parent), np.uint8)
        self.lib.collide_ref_prune(_p(parent), _p(feasible), C.c_uint64(1), C.c_uint64(len(parent)), _p(keep))
        return keep


def records_equal(got, exp):
    """Every field bit for bit (NaN goals included); returns the name of the first field that differs, or None."""
    for name in RECORD_DTYPE.names:
        g, e = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        if not np.array_equal(g.view(np.uint32), e.view(np.uint32)):
            return name
    return None


# ---- hand-built layers ---------------------------------------------------------------------------------------------------
VS = np.float32(0.1)


def field_layer_arrays(idx, field):
    """Blocks idx [n,3] at 0.1 m holding field(centres float64 [m,3]) at every voxel centre, weight 1: wire arrays (idx, words)."""
    idx = np.asarray(idx, np.int32)
    c = map_ref.voxel_centres(idx, VS).astype(np.float64)
    d = field(c.reshape(-1, 3)).reshape(c.shape[:2]).astype(np.float32)
    words = np.zeros((len(idx), 4096, 3), np.uint32)
    words[..., 0] = d.view(np.uint32)
    words[..., 1] = np.float32(1.0).view(np.uint32)
    return idx, words


def wall_layer_arrays(blocks_x=3):
    """The wall field d = 4.0 - x over blocks_x x 1 x 1 blocks (x in [0, 1.6 * blocks_x)): affine, so its trilinear value is the
    field wherever the cell is complete (0.05 <= coordinate < 1.6 * blocks - 0.05)."""
    return field_layer_arrays([(x, 0, 0) for x in range(blocks_x)], lambda c: 4.0 - c[:, 0])


ROOM_C, ROOM_R = np.array([3.2, 3.2, 1.6]), 0.5
ROOM_REMOVED = [(1, 2, 0), (3, 0, 1), (2, 2, 1)]
ROOM_UNOBSERVED = [(0, 5, 5, 5), (5, 100, 7, 3), (10, 8, 8, 8), (20, 15, 0, 15), (27, 3, 12, 9)]  # (block ordinal, vx, vy, vz)


def room_layer_arrays():
    """4 x 4 x 2 blocks at 0.1 m: d = min(x, 6.4 - x, y, 6.4 - y, |p - c| - 0.5) at voxel centres, weight 1; three blocks removed
    and a few single voxels set to weight 0."""
    idx = [(x, y, z) for z in range(2) for y in range(4) for x in range(4) if (x, y, z) not in ROOM_REMOVED]

    def field(c):
        walls = np.minimum(np.minimum(c[:, 0], 6.4 - c[:, 0]), np.minimum(c[:, 1], 6.4 - c[:, 1]))
        return np.minimum(walls, np.linalg.norm(c - ROOM_C, axis=1) - ROOM_R)
    idx, words = field_layer_arrays(idx, field)
    for bi, vx, vy, vz in ROOM_UNOBSERVED:
        words[bi, (vx % 16) + 16 * (vy % 16 + 16 * (vz % 16)), 1] = 0
    return idx, words


def ball_segments(rng, a, lo, hi, max_len=1.5):
    """For every start a[n,3] an end point uniform in the ball of max_len about it, redrawn until it lies in the box [lo, hi]."""
    a = np.asarray(a, np.float64)
    b = np.empty_like(a)
    todo = np.arange(len(a))
    while len(todo):
        d = rng.normal(size=(len(todo), 3))
        d *= (max_len * rng.uniform(0.0, 1.0, len(todo)) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
        c = a[todo] + d
        ok = np.all((c >= lo) & (c <= hi), axis=1)
        b[todo[ok]] = c[ok]
        todo = todo[~ok]
    return b


ROOM_LO, ROOM_HI = np.zeros(3), np.array([6.4, 6.4, 3.2])


def room_segments(rng, n=2000, max_len=1.5):
    """Segments with end points uniform in the room's box, at most max_len apart."""
    a = rng.uniform(ROOM_LO, ROOM_HI, size=(n, 3))
    return a.astype(np.float32), ball_segments(rng, a, ROOM_LO, ROOM_HI, max_len).astype(np.float32)


# ---- trees: name -> (parent, feasible, keep) -------------------------------------------------------------------------------
_K, _I = TREE_KEEP, TREE_INVALID
TREES = {
    "one node": ([-1], [1], [_K]),
    "one blocked node": ([-1], [0], [0]),
    "chain": ([-1, 0, 1, 2, 3], [1, 1, 0, 1, 1], [_K, _K, 0, 0, 0]),
    "star": ([-1, 0, 0, 0, 0], [1, 0, 1, 1, 0], [_K, 0, _K, _K, 0]),
    "parent with the higher index": ([1, 2, -1, 0], [1, 1, 1, 1], [_K, _K, _K, _K]),
    "parent with the higher index, blocked": ([1, 2, -1, 0], [1, 0, 1, 1], [0, 0, _K, 0]),
    "self parent": ([-1, 1, 1], [1, 1, 1], [_K, _I, _I]),
    "2-cycle with a tail": ([1, 0, 1, 2, -1], [1, 1, 1, 1, 1], [_I, _I, _I, _I, _K]),
    "out-of-range parent": ([-1, 7, 1, -2, 0], [1, 1, 1, 1, 1], [_K, _I, _I, _I, _K]),
    "blocked root": ([-1, 0, 1, -1, 3], [0, 1, 1, 1, 1], [0, 0, 0, _K, _K]),
    "feasible is bit 0": ([-1, 0, 0], [3, 2, 255], [_K, 0, _K]),
}
