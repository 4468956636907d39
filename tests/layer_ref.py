"""Plain numpy reference of the TSDF layer store: wire upload (deserializeMsgToLayer), the voxel merge
(mergeVoxelAIntoVoxelB), the rigid resample (transformLayer + Interpolator::getVoxel) and the relevant-voxel extraction
(findRelevantVoxelIndices).  Written from the definitions in include/coxgraph_hip.h and DESIGN.md; shares no code with the
oracle or the kernels.

Both engines are built without contraction and with IEEE division, so a reference that keeps every intermediate in
np.float32 and follows the stated operation order is exact: the bar of every comparison is bit for bit.

A layer is (idx int32[n,3], vox uint32[n,4096,3]) with blocks in (z,y,x) order, as Layer.download() returns it; a voxel is
three words: distance bits, weight bits, colour a | b<<8 | g<<16 | r<<24."""
import numpy as np

F = np.float32
K_EPS = F(1e-6)          # the engine's kEps (voxblox kCoordinateEpsilon)
VPS = 16
NVOX = VPS ** 3
IDX_LIMIT = (1 << 20) - 1  # block indices live in [-(2^20 - 1), 2^20 - 1)
PATH_NONE, PATH_TRILINEAR, PATH_NEAREST = 0, 1, 2
LIN = np.arange(NVOX)
LOC = np.stack([LIN % VPS, (LIN // VPS) % VPS, LIN // (VPS * VPS)], axis=1)
# Interpolator's 8x8 table; neighbour order (0,0,0),(0,0,1),(0,1,0),(0,1,1),(1,0,0),(1,0,1),(1,1,0),(1,1,1)
TABLE = np.array([[1, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 1, 0, 0, 0], [-1, 0, 1, 0, 0, 0, 0, 0], [-1, 1, 0, 0, 0, 0, 0, 0],
                  [1, 0, -1, 0, -1, 0, 1, 0], [1, -1, -1, 1, 0, 0, 0, 0], [1, -1, 0, 0, -1, 1, 0, 0], [-1, 1, 1, -1, 1, -1, -1, 1]], F)


class Grid:
    """The four float32 constants of a layer's grid"""

    def __init__(self, voxel):
        self.vs = F(voxel)
        self.vs_inv = F(1.0 / np.float64(self.vs))
        self.bs = F(self.vs * F(VPS))
        self.bs_inv = F(1.0 / np.float64(self.bs))


def empty_layer():
    return np.zeros((0, 3), np.int32), np.zeros((0, NVOX, 3), np.uint32)


def order_zyx(idx):
    idx = np.asarray(idx).reshape(-1, 3)
    return np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))


def _f(words):
    return np.ascontiguousarray(words, np.uint32).view(F)


def _centre(i, size):
    """getCenterPointFromGridIndex: (float(i) + 0.5) * size"""
    return (np.asarray(i).astype(F) + F(0.5)) * size


def _key(b):
    b = np.asarray(b, np.int64)
    return ((b[..., 2] + (1 << 20)) << 42) | ((b[..., 1] + (1 << 20)) << 21) | (b[..., 0] + (1 << 20))


# ---- mergeVoxelAIntoVoxelB ----------------------------------------------------------------------------------------
def _round_half_away(v):
    r = np.trunc(v)
    return r + np.where(np.abs(v - r) >= F(0.5), np.copysign(F(1), v), F(0)).astype(F)


def merge_voxels_ref(a_words, b_words):
    """A's voxels [...,3] merged into B's -> B's new words.  cw = aw + bw; nothing happens unless cw > 0"""
    a, b = np.ascontiguousarray(a_words, np.uint32), np.ascontiguousarray(b_words, np.uint32)
    ad, aw, bd, bw = _f(a[..., 0]), _f(a[..., 1]), _f(b[..., 0]), _f(b[..., 1])
    out = b.copy()
    with np.errstate(all="ignore"):
        cw = aw + bw
        hit = cw > 0
        d = (ad * aw + bd * bw) / cw
        w1, w2 = aw / cw, bw / cw
        col = np.zeros(cw.shape, np.uint32)
        for sh in (0, 8, 16, 24):
            ca, cb = ((a[..., 2] >> sh) & 255).astype(F), ((b[..., 2] >> sh) & 255).astype(F)
            v = _round_half_away(ca * w1 + cb * w2)
            col |= ((np.where(hit, v, 0).astype(np.int64) & 255) << sh).astype(np.uint32)
    out[..., 0] = np.where(hit, d.view(np.uint32), b[..., 0])
    out[..., 1] = np.where(hit, cw.view(np.uint32), b[..., 1])
    out[..., 2] = np.where(hit, col, b[..., 2])
    return out


# ---- deserializeMsgToLayer ---------------------------------------------------------------------------------------
def upload_ref(layer, idx, vox, action):
    """action 0 overwrites the message's blocks, 1 merges them voxel by voxel, 2 clears the layer first -> new layer"""
    lidx, lvox = empty_layer() if action == 2 else layer
    idx, vox = np.asarray(idx, np.int32).reshape(-1, 3), np.asarray(vox, np.uint32).reshape(-1, NVOX, 3)
    if np.any(idx < -IDX_LIMIT) or np.any(idx >= IDX_LIMIT):
        raise ValueError("block index out of range")
    blocks = {tuple(int(v) for v in i): w for i, w in zip(lidx, lvox)}
    for i, w in zip(idx, vox):
        k = tuple(int(v) for v in i)
        if action == 1:
            blocks[k] = merge_voxels_ref(w, blocks.get(k, np.zeros((NVOX, 3), np.uint32)))
        else:
            blocks[k] = w.copy()
    if not blocks:
        return empty_layer()
    keys = np.array(list(blocks), np.int32)
    o = order_zyx(keys)
    return keys[o], np.stack([blocks[tuple(int(v) for v in keys[j])] for j in o])


# ---- transformLayer ------------------------------------------------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _rotate(q, v):
    """Eigen's quaternion * vector: uv = 2 (q.vec x v); (v + w uv) + q.vec x uv"""
    qv = (q[1], q[2], q[3])
    uv = _cross(qv, v)
    uv = tuple(u + u for u in uv)
    c = _cross(qv, uv)
    return tuple((v[k] + q[0] * uv[k]) + c[k] for k in range(3))


def _pose(T):
    T = np.asarray(T, F)
    return [F(x) for x in T[:4]], [F(x) for x in T[4:]]


def inverse_ref(T):
    """minkindr inverse: the conjugate rotation and -R^T t"""
    q, t = _pose(T)
    qi = [q[0], -q[1], -q[2], -q[3]]
    rt = _rotate(qi, t)
    return qi, [-rt[0], -rt[1], -rt[2]]


def candidate_blocks_ref(idx, grid_in, T_B_A, grid_out):
    """Output blocks that may receive data: around each transformed input block centre a float-stepped box of half
    diagonal sqrt(3)/2 * block_in -> int32 [m,3] in (z,y,x) order"""
    q, t = _pose(T_B_A)
    offset = F(F(F(np.sqrt(3.0)) * grid_in.bs) * F(0.5))
    inv = F(1) / grid_out.bs
    found = set()
    idx = np.asarray(idx).reshape(-1, 3)
    for b in idx[order_zyx(idx)]:
        r = _rotate(q, tuple(_centre(int(b[k]), grid_in.bs) for k in range(3)))
        axes = []
        for k in range(3):
            c = F(r[k] + t[k])
            x, hi, ids = F(c - offset), F(c + offset), []
            while x < hi:
                ids.append(int(np.floor(F(F(x * inv) + K_EPS))))
                x = F(x + grid_out.bs)
            axes.append(ids)
        found.update((ix, iy, iz) for ix in axes[0] for iy in axes[1] for iz in axes[2])
    cand = np.array(sorted(found, key=lambda c: (c[2], c[1], c[0])), np.int32).reshape(-1, 3)
    if np.any(cand < -IDX_LIMIT) or np.any(cand >= IDX_LIMIT):
        raise ValueError("candidate block index out of range")
    return cand


def _interp(q, data):
    """q . (table . data), every sum sequential from 0"""
    md = []
    for r in range(8):
        s = np.zeros_like(data[0])
        for c in range(8):
            s = s + TABLE[r, c] * data[c]
        md.append(s)
    v = np.zeros_like(data[0])
    for i in range(8):
        v = v + q[i] * md[i]
    return v


def _resample_points(keys, rows, vox, g, pos):
    """Interpolator::getVoxel(pos, interpolate) or, failing that, the nearest voxel -> words [n,3], path [n]"""
    n = len(pos[0])

    def find(b):
        k = _key(np.stack(b, axis=-1))
        j = np.clip(np.searchsorted(keys, k), 0, max(len(keys) - 1, 0))
        hit = (keys[j] == k) if len(keys) else np.zeros(n, bool)
        return np.where(hit, rows[j] if len(keys) else 0, -1)

    lim = F(1048575.0)
    sc = [p * g.bs_inv for p in pos]
    inside = np.ones(n, bool)
    for s in sc:
        inside &= (s > -lim) & (s < lim)
    b0 = [np.where(inside, np.floor(s + K_EPS), 0).astype(np.int64) for s in sc]
    row0 = find(b0)
    exists = inside & (row0 >= 0)
    b, vi, v0 = [], [], []
    for k in range(3):
        origin = b0[k].astype(F) * g.bs
        v = np.clip(np.floor((pos[k] - origin) * g.vs_inv + K_EPS).astype(np.int64), 0, VPS - 1)
        v0.append(v)
        low = (pos[k] - (origin + _centre(v, g.vs))) < F(0)     # below the voxel centre: the lower neighbour starts the cell
        v = v - low
        wrap = v < 0
        b.append(b0[k] - wrap)
        vi.append(v + VPS * wrap)
    ok = exists.copy()
    d, w, ch = [], [], [[], [], [], []]
    for i in range(8):
        step = ((i >> 2) & 1, (i >> 1) & 1, i & 1)
        nv, nb = [], []
        for k in range(3):
            v = vi[k] + step[k]
            over = v >= VPS
            nv.append(v - VPS * over)
            nb.append(b[k] + over)
        row = find(nb)
        ok &= row >= 0
        words = vox[np.maximum(row, 0), nv[0] + VPS * (nv[1] + VPS * nv[2])]
        wi = _f(words[:, 1])
        ok &= wi > 0
        d.append(_f(words[:, 0]))
        w.append(wi)
        for c, sh in enumerate((24, 16, 8, 0)):
            ch[c].append(((words[:, 2] >> sh) & 255).astype(F))
    off = [(pos[k] - (b[k].astype(F) * g.bs + _centre(vi[k], g.vs))) * g.vs_inv for k in range(3)]
    dx, dy, dz = off
    q = [np.ones(n, F), dx, dy, dz, dx * dy, dy * dz, dz * dx, dx * dy * dz]
    out = np.zeros((n, 3), np.uint32)
    tri = np.zeros((n, 3), np.uint32)
    tri[:, 0], tri[:, 1] = _interp(q, d).view(np.uint32), _interp(q, w).view(np.uint32)
    for c, sh in enumerate((24, 16, 8, 0)):     # colour channels: interpolated as floats, truncated toward zero, & 255
        val = np.where(ok, _interp(q, ch[c]), 0)
        tri[:, 2] |= ((np.trunc(val).astype(np.int64) & 255) << sh).astype(np.uint32)
    near = vox[np.maximum(row0, 0), v0[0] + VPS * (v0[1] + VPS * v0[2])]
    out[ok] = tri[ok]
    out[exists & ~ok] = near[exists & ~ok]
    path = np.where(ok, PATH_TRILINEAR, np.where(exists, PATH_NEAREST, PATH_NONE)).astype(np.uint8)
    return out, path


def resample_ref(idx, vox, voxel_in, T_B_A, voxel_out, chunk=32):
    """transformLayer(A, T_B_A) onto a grid of voxel_out -> (candidate blocks int32 [m,3] in (z,y,x) order, words
    uint32 [m,4096,3], path uint8 [m,4096]).  A block where every path is PATH_NONE is one that transformLayer drops."""
    gi, go = Grid(voxel_in), Grid(voxel_out)
    idx, vox = np.asarray(idx, np.int32).reshape(-1, 3), np.asarray(vox, np.uint32).reshape(-1, NVOX, 3)
    if len(idx) == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, NVOX, 3), np.uint32), np.zeros((0, NVOX), np.uint8)
    cand = candidate_blocks_ref(idx, gi, T_B_A, go)
    qi, ti = inverse_ref(T_B_A)
    keys = _key(idx)
    o = np.argsort(keys)
    keys, rows = keys[o], o
    words, path = np.zeros((len(cand), NVOX, 3), np.uint32), np.zeros((len(cand), NVOX), np.uint8)
    with np.errstate(all="ignore"):
        for s in range(0, len(cand), chunk):
            c = cand[s:s + chunk]
            centre = tuple((c[:, None, k].astype(F) * go.bs + _centre(LOC[None, :, k], go.vs)).ravel() for k in range(3))
            r = _rotate(qi, centre)
            pos = [r[k] + ti[k] for k in range(3)]
            wd, pt = _resample_points(keys, rows, vox, gi, pos)
            words[s:s + chunk], path[s:s + chunk] = wd.reshape(len(c), NVOX, 3), pt.reshape(len(c), NVOX)
    return cand, words, path


def merge_ref(A, T_B_A, B, voxel_a, voxel_b=None):
    """mergeLayerAintoLayerB(A, [T_B_A,] B) -> (new B, path codes of the resampled blocks that were merged or None)"""
    if T_B_A is None:
        return upload_ref(B, A[0], A[1], 1), None
    cand, words, path = resample_ref(A[0], A[1], voxel_a, T_B_A, voxel_a if voxel_b is None else voxel_b)
    keep = (path != PATH_NONE).any(axis=1)
    return upload_ref(B, cand[keep], words[keep], 1), path[keep]


# ---- findRelevantVoxelIndices ------------------------------------------------------------------------------------
def relevant_points_ref(idx, vox, voxel, min_w, max_d):
    """Voxels with w > min_w and |d| < max_d -> float32 [n,5] = centre x, y, z, distance, weight; blocks in (z,y,x)
    order, voxels in linear order; centre = float(b) * block_size + (float(l) + 0.5) * voxel"""
    g = Grid(voxel)
    idx, vox = np.asarray(idx, np.int32).reshape(-1, 3), np.asarray(vox, np.uint32).reshape(-1, NVOX, 3)
    out = [np.zeros((0, 5), F)]
    for j in order_zyx(idx):
        d, w = _f(vox[j, :, 0]), _f(vox[j, :, 1])
        with np.errstate(invalid="ignore"):
            m = (w > F(min_w)) & (np.abs(d) < F(max_d))
        c = [F(idx[j, k]) * g.bs + _centre(LOC[m, k], g.vs) for k in range(3)]
        out.append(np.stack(c + [d[m], w[m]], axis=1).astype(F))
    return np.concatenate(out, axis=0)
