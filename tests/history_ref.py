"""numpy restatement of the observation-history rule, for checking the HIP kernels bit for bit.

Marking.  A point p_C of a frame with pose T_G_C = (qw, qx, qy, qz, tx, ty, tz) marks when it is finite, min_ray <= |p_C| <=
max_ray (isPointValid; |p| = sqrt((x x + y y) + z z) in float32) and the cloud is not a freespace cloud.  It is moved to G with
Eigen's _transformVector in float32, operation by operation as the device does it (uv = 2 (q x p); p + w uv + q x uv; + t),
scaled by the float32 1 / voxel_size and indexed with floor(x * inv + 1e-6f), the sum rounded to float32 before the floor.
Block = index >> 4, cell = (local >> 2) per axis with x fastest, bit = frame id (word id >> 5).

Encoding.  A 256-bit mask as ascending inclusive [first, last] runs; adjacent bits form one run.
"""
import numpy as np

F = np.float32
EPS = F(1e-6)
CELLS, WORDS = 64, 8


def _cross(a, b):
    # (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), every product and difference rounded to float32
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def transform_points(T, p):
    T = np.asarray(T, F)
    p = np.asarray(p, F).reshape(-1, 3)
    qv = np.broadcast_to(T[1:4], p.shape)
    uv = _cross(qv, p)
    uv = (uv + uv).astype(F)
    c = _cross(qv, uv)
    return (((p + T[0] * uv).astype(F) + c).astype(F) + T[4:7]).astype(F)


def marking_points(p, min_ray, max_ray, freespace=False):
    """bool[n]: the points of a cloud that mark."""
    p = np.asarray(p, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).astype(F) + p[:, 2] * p[:, 2]).astype(F)).astype(F)
        ok = (r <= F(3.0e38)) & ~(r < F(min_ray)) & ~(r > F(max_ray))
    return ok & (not freespace)


def grid_index(p_G, voxel_size):
    inv = F(1.0) / F(voxel_size)
    return np.floor((np.asarray(p_G, F) * inv).astype(F) + EPS).astype(np.int64)


def cells_of(p_G, voxel_size):
    """-> (block int64[n,3], cell int64[n]) of points in the layer's frame."""
    g = grid_index(p_G, voxel_size)
    local = g & 15
    return g >> 4, (local[:, 0] >> 2) | ((local[:, 1] >> 2) << 2) | ((local[:, 2] >> 2) << 4)


class Record:
    """The record as a dict block index -> uint32[64, 8]."""

    def __init__(self, voxel_size):
        self.voxel_size = float(F(voxel_size))
        self.blocks = {}

    def mark(self, T, p, frame_id, min_ray, max_ray, freespace=False):
        assert 0 <= frame_id < 256
        p = np.asarray(p, F).reshape(-1, 3)
        keep = marking_points(p, min_ray, max_ray, freespace)
        if not keep.any():
            return
        blk, cell = cells_of(transform_points(T, p[keep]), self.voxel_size)
        uniq = np.unique(np.concatenate([blk, cell[:, None]], 1), axis=0)
        for bx, by, bz, c in uniq:
            m = self.blocks.setdefault((int(bx), int(by), int(bz)), np.zeros((CELLS, WORDS), np.uint32))
            m[c, frame_id >> 5] |= np.uint32(1) << np.uint32(frame_id & 31)

    def arrays(self):
        """(block_index int32[n,3], masks uint32[n,64,8]) in (z, y, x) order, as cox_obs_download gives them."""
        keys = sorted(self.blocks, key=lambda k: (k[2], k[1], k[0]))
        idx = np.array(keys, np.int32).reshape(len(keys), 3)
        masks = np.stack([self.blocks[k] for k in keys]) if keys else np.zeros((0, CELLS, WORDS), np.uint32)
        return idx, masks


def runs_of_mask(words):
    """uint32[8] -> [[first, last], ...] ascending, inclusive, adjacent bits merged."""
    bits = np.unpackbits(np.asarray(words, "<u4").view(np.uint8), bitorder="little")
    padded = np.concatenate([[0], bits, [0]]).astype(np.int8)
    d = np.diff(padded)
    return [[int(a), int(b) - 1] for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]


def triangle_masks(xyz, voxel_size, block_index, masks):
    """OR over the three vertices' cells; xyz float32[3 nt, 3] -> uint32[nt, 8].  A missing block counts as all zero."""
    table = {tuple(int(v) for v in b): k for k, b in enumerate(np.asarray(block_index))}
    blk, cell = cells_of(np.asarray(xyz, F).reshape(-1, 3), voxel_size)
    slot = np.array([table.get((int(b[0]), int(b[1]), int(b[2])), -1) for b in blk], np.int64)
    per_vertex = np.where((slot >= 0)[:, None], np.asarray(masks, np.uint32)[np.maximum(slot, 0), cell], np.uint32(0)) if len(masks) else np.zeros((len(blk), WORDS), np.uint32)
    v = per_vertex.reshape(-1, 3, WORDS)
    return v[:, 0] | v[:, 1] | v[:, 2]


def encode(tri_masks, vertex_begin):
    """-> (history_begin uint64[nt + 1], history uint32[...], block_has_history uint8[nb]) in cox_mesh_msg's layout."""
    tri_masks = np.asarray(tri_masks, np.uint32).reshape(-1, WORDS)
    uniq, inv = np.unique(tri_masks, axis=0, return_inverse=True)  # (few distinct masks: each is decoded once)
    flat = [[v for run in runs_of_mask(m) for v in run] for m in uniq]
    hb, hist = [0], []
    for k in np.asarray(inv).reshape(-1):
        hist += flat[k]
        hb.append(len(hist))
    hb = np.array(hb, np.uint64)
    vb = np.asarray(vertex_begin, np.int64) // 3
    has = np.array([1 if hb[vb[k + 1]] > hb[vb[k]] else 0 for k in range(len(vb) - 1)], np.uint8)
    return hb, np.array(hist, np.uint32), has
