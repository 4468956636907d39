"""Plain numpy references for the input side of a frame (coxgraph_amd/csrc/cox_frontend.hpp): the depth front end, the visiting
order the device-side point count feeds, and the segments of the kernel that reads pinned host inputs.  No GPU, no engine.

The depth rule is the kernel's and coxgraph_amd.synth's: a pixel is valid when its depth is finite and > 0 (denormals are, zeros of
either sign are not); valid pixels become points in row-major pixel order; in float32, one rounding per operation,
xn = (f32(u) - cx) / fx, x = d * xn, the same for y, z = d; the colour is the pixel's word, or 0 without a colour image."""
import numpy as np

F32 = np.float32
U32 = np.uint32
DEPTH_TILE = 2048  # kDepthTile


def depth_tiles(n_pixels):
    """Words of tile_sums an image of n_pixels uses: one per tile of 2048 pixels, at least one."""
    return max(1, -(-int(n_pixels) // DEPTH_TILE))


def depth_valid(depth):
    d = np.asarray(depth, F32)
    return np.isfinite(d) & (d > 0)


def depth_to_points(depth, rgba, K):
    """depth f32 [h, w]; rgba u8 [h * w, 4] (or [h, w, 4]) or None; K = (fx, fy, cx, cy).
    -> (xyz f32 [n, 3], rgba u8 [n, 4], tile_sums u32 [tiles], n)"""
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    fx, fy, cx, cy = (F32(x) for x in K)
    d = depth.reshape(-1)
    keep = depth_valid(d)
    i = np.flatnonzero(keep)
    u, v = (i % w).astype(F32), (i // w).astype(F32)
    dv = d[i]
    with np.errstate(over="ignore", under="ignore"):
        xn = ((u - cx) / fx).astype(F32)
        yn = ((v - cy) / fy).astype(F32)
        xyz = np.stack([(dv * xn).astype(F32), (dv * yn).astype(F32), dv], axis=1).astype(F32)
    if rgba is None:
        colours = np.zeros((len(i), 4), np.uint8)
    else:
        colours = np.ascontiguousarray(np.asarray(rgba, np.uint8).reshape(-1, 4)[i])
    padded = np.zeros(depth_tiles(h * w) * DEPTH_TILE, U32)
    padded[:h * w] = keep
    tile_sums = padded.reshape(-1, DEPTH_TILE).sum(axis=1, dtype=np.uint64).astype(U32)
    return np.ascontiguousarray(xyz), colours, tile_sums, int(len(i))


def depth_to_points_f64(depth, K):
    """The same formula in float64 on the float32 inputs: xyz f64 [n, 3]."""
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    fx, fy, cx, cy = (np.float64(F32(x)) for x in K)
    d = depth.reshape(-1)
    i = np.flatnonzero(depth_valid(d))
    dv = d[i].astype(np.float64)
    return np.stack([dv * (((i % w).astype(np.float64) - cx) / fx), dv * (((i // w).astype(np.float64) - cy) / fy), dv], axis=1)


def mixed_sequence(idx, n):
    """cox_device.hpp mixed_sequence: the sequence number at which point idx of n is visited (idx: int or array)."""
    idx = np.asarray(idx, np.int64)
    groups = int(n) >> 10
    return np.where((groups << 10) <= idx, idx, (idx & 1023) * groups + (idx >> 10))


def pow2_above(n):
    """cox_raygen.hpp pow2_above: the power of two > n, at most 2^31 (FrameParams::np2)."""
    p = 1
    while p <= n and p < 0x80000000:
        p <<= 1
    return p


def host_segment(n_bytes):
    """(n16, tail_words) of an array of n_bytes (a multiple of 4): whole 16 bytes, then 4-byte words behind them."""
    assert n_bytes % 4 == 0
    return n_bytes // 16, (n_bytes % 16) // 4


def copy_words(a):
    """What the copy kernel must leave at its destination."""
    return np.array(a, U32, copy=True)
