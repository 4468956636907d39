"""Seeded cases for the layer store (tests/test_layer_ref_cpu.py, tests/test_gpu_layer.py): a layer A, a transform or
none, an output voxel size and a layer B to merge into.  Built on the 3x4x4 box, the block sets and the masks of
tests/submap_cases.py; the values are chosen to reach what fused maps never hold: weight 0 among the eight neighbours,
missing neighbour blocks, negative indices, unequal voxel sizes, blended colours on x.5 and interpolated ones at 0 / 255."""
import numpy as np

import submap_cases
from submap_cases import LIN, LOC  # noqa: F401

VOXELS = (0.05, 0.1, 0.125, 0.2)
TRANSFORMS = ("none", "identity", "yaw_tilt", "full", "blocks", "flip_x", "flip_y", "flip_z")
B_KINDS = ("empty", "independent", "self")
MASKS = ("all", "blobs", "salt", "zeros")
DISTANCES = ("smooth", "raw")
COLOURS = ("random", "half", "checker")
WEIGHTS = np.array([0.0, 1e-6, 0.5, 1.0, 37.25, 1e4], np.float32)


def quat(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis])


def pose(q, t):
    q = np.asarray(q, np.float64)
    return np.concatenate([q / np.linalg.norm(q), t]).astype(np.float32)


def rotation_matrix(q):
    w, x, y, z = np.asarray(q, np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def centres64(idx, voxel):
    """voxel centres in float64 on the grid the engines use (the float32 voxel size)"""
    return ((np.asarray(idx)[:, None, :].astype(np.int64) * 16 + LOC[None]).astype(np.float64) + 0.5) * float(np.float32(voxel))


def words(d, w, colour):
    vox = np.zeros(d.shape + (3,), np.uint32)
    vox[..., 0], vox[..., 1], vox[..., 2] = np.asarray(d, np.float32).view(np.uint32), np.asarray(w, np.float32).view(np.uint32), colour
    return vox


def make_layer(rng, voxel, blocks, mask, dist, colour, lo, parity=0, weight=None, max_blocks=None):
    idx = submap_cases.block_set(blocks, rng, lo)
    if max_blocks is not None and len(idx) > max_blocks:
        idx = idx[np.sort(rng.choice(len(idx), max_blocks, replace=False))]
    c = centres64(idx, voxel)
    trunc = np.float32(3 * voxel)
    if dist == "smooth":
        d = np.clip(submap_cases.field_values("noise", rng, c, voxel, None), -trunc, trunc).astype(np.float32)
    else:                                   # raw floats, a fifth of them exactly on +-trunc
        d = (rng.standard_normal(c.shape[:-1]) * float(trunc)).astype(np.float32)
        r = rng.random(d.shape)
        d[r < 0.1], d[(r >= 0.1) & (r < 0.2)] = trunc, -trunc
    if weight is None:
        w = rng.choice(WEIGHTS[1:], size=d.shape, p=[0.05, 0.15, 0.5, 0.2, 0.1]).astype(np.float32)
    else:
        w = np.full(d.shape, weight, np.float32)
    if mask == "blobs":
        for _ in range(int(rng.integers(3, 9))):
            p = c[rng.integers(len(idx)), rng.integers(4096)]
            w[np.linalg.norm(c - p, axis=-1) < rng.uniform(2, 7) * voxel] = 0.0
    elif mask == "salt":                    # isolated weight-0 voxels: one of the eight neighbours fails
        w[rng.random(d.shape) < 0.02] = 0.0
    elif mask == "zeros":
        r = rng.random(d.shape)
        d[r < 0.01] = 0.0
        d[(r >= 0.01) & (r < 0.02)] = -0.0
    if colour == "random":
        col = rng.integers(0, 2 ** 32, d.shape, dtype=np.uint64).astype(np.uint32)
    elif colour == "half":                  # even bytes here, odd bytes in the other layer, equal weights: every blend is x.5
        b = (2 * rng.integers(0, 128, d.shape + (4,)) + parity).astype(np.uint32)
        col = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24)
    else:                                   # 0 and 255 at alternating voxels: the interpolation works at the ends of the byte
        g = idx[:, None, :].astype(np.int64) * 16 + LOC[None]
        col = np.where((g.sum(axis=-1) + parity) % 2 == 1, 0xFFFFFFFF, 0).astype(np.uint32)
    return idx, words(d, w, col)


def case(seed):
    """-> dict(voxel_a, voxel_b, A=(idx, vox), T (float32[7] or None), B=(idx, vox), meta)"""
    rng = np.random.default_rng(7907 * seed + 5)
    voxel = float(rng.choice(VOXELS))
    tkind, bkind = TRANSFORMS[seed % len(TRANSFORMS)], B_KINDS[seed % len(B_KINDS)]
    blocks = str(rng.choice(submap_cases.BLOCK_SETS))
    mask, dist, colour = (str(rng.choice(x)) for x in (MASKS, DISTANCES, COLOURS))
    scale = {3: 0.5, 4: 2.0}.get(seed % 5, 1.0) if tkind != "none" else 1.0
    voxel_b = voxel * scale
    lo = rng.integers(-3, 2, 3)             # the box straddles zero
    weight = float(rng.choice([0.5, 1.0, 37.25])) if colour == "half" else None
    A = make_layer(rng, voxel, blocks, mask, dist, colour, lo, 0, weight, max_blocks=8 if scale < 1 else None)
    t = rng.uniform(-2.0, 2.0, 3) * (rng.random() < 0.7)
    if tkind == "none":
        T = None
    elif tkind == "identity":
        T = pose([1, 0, 0, 0], [0, 0, 0])
    elif tkind == "yaw_tilt":
        T = pose(quat([rng.normal() * 0.05, rng.normal() * 0.05, 1.0], rng.uniform(-np.pi, np.pi)), t)
    elif tkind == "full":
        T = pose(rng.normal(size=4), t)
    elif tkind == "blocks":
        T = pose([1, 0, 0, 0], rng.integers(-2, 3, 3) * float(np.float32(voxel) * np.float32(16)))
    else:
        T = pose(quat(np.eye(3)["xyz".index(tkind[-1])], np.pi).round(), t)   # exactly (0, 1, 0, 0) and its kin
    if bkind == "empty":
        B = (np.zeros((0, 3), np.int32), np.zeros((0, 4096, 3), np.uint32))
    elif bkind == "self" and scale == 1.0:
        B = A
    else:
        bkind = "independent"
        rb = np.random.default_rng(104729 * seed + 11)
        lo_b = lo + rb.integers(-1, 2, 3)
        if T is not None:                   # an overlapping box where A lands
            R = rotation_matrix(T[:4].astype(np.float64))
            mid = (lo + 0.5 * np.array(submap_cases.BOX)) * 16 * voxel
            lo_b = np.floor((R @ mid + T[4:]) / (16 * voxel_b) - 0.5 * np.array(submap_cases.BOX)).astype(np.int64) + rb.integers(-1, 2, 3)
        B = make_layer(rb, voxel_b, str(rb.choice(submap_cases.BLOCK_SETS)), str(rb.choice(MASKS)), dist, colour, lo_b, 1, weight)
    meta = dict(seed=seed, voxel=voxel, scale=scale, transform=tkind, b=bkind, blocks=blocks, mask=mask, dist=dist, colour=colour)
    return dict(voxel_a=voxel, voxel_b=voxel_b, A=A, T=T, B=B, meta=meta)


def plane_layer(normal, off, lo=(-2, -1, -2), voxel=0.1):
    """d = n.x - off at every voxel centre of the full box, weight 1 -> (idx, vox, unit normal)"""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    idx = submap_cases.block_set("full", None, lo)
    d = centres64(idx, voxel) @ n - off
    return idx, words(d, np.ones(d.shape), np.uint32(0x80808080)), n


PLANE_TRANSFORMS = (pose(quat([0, 0, 1], 0.17), [0.13, -0.07, 0.02]), pose(quat([1, 2, 3], 1.1), [0.5, -0.8, 0.3]),
                    pose(quat([0, 0, 1], 0.5 * np.pi), [0, 0, 0]), pose([1, 0, 0, 0], [0.05, 0.05, 0.05]))


def exact_layer(seed, lo=(-2, -1, -2), blocks="full", voxel=0.125):
    """A layer on which whole-block shifts and half turns are exact at voxel size 0.125: weights are powers of two (so
    (d*w)/w == d), every voxel is observed, no distance is -0.0"""
    rng = np.random.default_rng(seed)
    idx = submap_cases.block_set(blocks, rng, lo)
    d = (rng.standard_normal((len(idx), 4096)) * 0.3).astype(np.float32)
    d[d == 0] = np.float32(0.25)
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=d.shape)
    return idx, words(d, w, rng.integers(0, 2 ** 32, d.shape, dtype=np.uint64).astype(np.uint32))
