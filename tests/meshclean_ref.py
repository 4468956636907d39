"""numpy restatement of the five mesh clean-up rules of DESIGN.md section 7h (include/coxgraph_hip_mesh.h), parameterised by the
dtype of the float accumulations.

Index decisions are always taken as specified -- the float32 cell expression, the canonical triple, "the first in mesh order
stays", the orders of vertices, members, neighbours and triangles.  Only the sums (and the divide / square root behind them) run
in `dtype`: float64 is the reference the GPU is compared with, float32 restates the GPU's own arithmetic and measures how far
float32 may drift from the reference on a given input (the tolerance of tests/test_gpu_meshclean.py).
"""
import numpy as np


class IndexRange(Exception):
    """An axis spans 2^21 cells or more (COX_ERR_INDEX_RANGE)."""


def mesh(xyz, triangles, normals=None, rgb=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return dict(xyz=xyz, triangles=np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3),
                normals=np.zeros_like(xyz) if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3),
                rgb=np.zeros(xyz.shape, np.uint8) if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3))


# ---- clean ---------------------------------------------------------------------------------------------------------------------
def clean(m):
    """-> (mesh, (degenerate, duplicate, unreferenced))."""
    tri = m["triangles"].astype(np.int64)
    nv = len(m["xyz"])
    deg = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2]) if len(tri) else np.zeros(0, bool)
    live = np.flatnonzero(~deg)
    t = tri[live]
    k = np.argmin(t, axis=1) if len(t) else np.zeros(0, np.int64)
    canon = np.stack([t[np.arange(len(t)), (k + j) % 3] for j in range(3)], axis=1) if len(t) else np.zeros((0, 3), np.int64)
    seen, keep = set(), []
    for i, c in zip(live.tolist(), map(tuple, canon.tolist())):  # mesh order: the first of equal canonical forms stays
        if c not in seen:
            seen.add(c)
            keep.append(i)
    keep = np.array(keep, np.int64)
    used = np.zeros(nv, bool)
    used[tri[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    out = dict(xyz=m["xyz"][used], normals=m["normals"][used], rgb=m["rgb"][used], triangles=new[tri[keep]].astype(np.uint32).reshape(-1, 3))
    return out, (int(deg.sum()), int(len(live) - len(keep)), int(nv - used.sum()))


# ---- sequential sums over the rows of a CSR list ------------------------------------------------------------------------------
def _rows(keys, n):
    """keys ascending -> (begin, count) per row 0 .. n-1."""
    count = np.bincount(keys, minlength=n).astype(np.int64)
    return np.cumsum(count) - count, count


def _sequential_sum(values, begin, count, dtype):
    """s[r] = ((values[begin] + values[begin + 1]) + ...) in dtype, from the first member on; rows with count 0 give 0."""
    s = np.zeros((len(begin),) + values.shape[1:], dtype)
    has = count > 0
    s[has] = values[begin[has]]
    for k in range(1, int(count.max()) if len(count) else 0):
        more = count > k
        s[more] = s[more] + values[begin[more] + k]
    return s


def adjacency(triangles, nv):
    """N(i) as CSR with ascending neighbour index: no self-loop, every neighbour once."""
    t = triangles.astype(np.int64)
    u = np.concatenate([t[:, 0], t[:, 1], t[:, 1], t[:, 2], t[:, 2], t[:, 0]])
    v = np.concatenate([t[:, 1], t[:, 0], t[:, 2], t[:, 1], t[:, 0], t[:, 2]])
    e = np.unique(np.stack([u, v], 1)[u != v], axis=0) if len(t) else np.zeros((0, 2), np.int64)
    begin, count = _rows(e[:, 0], nv)
    return begin, count, e[:, 1]


# ---- Taubin --------------------------------------------------------------------------------------------------------------------
def smooth_taubin(m, iterations=100, lam=0.5, mu=-0.53, dtype=np.float64):
    """-> positions in dtype (the factors are the float32 values the C ABI receives)."""
    p = m["xyz"].astype(dtype)
    begin, count, col = adjacency(m["triangles"], len(p))
    has = count > 0
    n = count[has].astype(dtype)[:, None]
    for _ in range(iterations):
        for f in (dtype(np.float32(lam)), dtype(np.float32(mu))):
            s = _sequential_sum(p[col], begin, count, dtype)
            q = p.copy()
            q[has] = p[has] + f * (s[has] / n - p[has])
            p = q
    return p


# ---- vertex normals ------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _normalized(a):
    z = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    out = a.copy()
    ok = z > 0
    out[ok] = a[ok] / np.sqrt(z[ok])[:, None]
    return out


def compute_normals(m, dtype=np.float64, xyz=None):
    p = (m["xyz"] if xyz is None else xyz).astype(dtype)
    t = m["triangles"].astype(np.int64)
    face = _cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]) if len(t) else np.zeros((0, 3), dtype)
    corner_vertex = t.reshape(-1)
    order = np.argsort(corner_vertex, kind="stable")  # (vertex, triangle) pairs emitted in triangle order
    begin, count = _rows(corner_vertex[order], len(p))
    zero = np.zeros((len(p), 3), dtype)
    return _normalized(zero + _sequential_sum(face[order // 3], begin, count, dtype))


# ---- vertex clustering ---------------------------------------------------------------------------------------------------------
def cells(xyz, cell_size):
    """The float32 cell expression: int(floorf((p - origin) / cell_size)), origin = min(p) - 0.5f * cell_size."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    c = np.float32(cell_size)
    origin = xyz.min(axis=0) - np.float32(0.5) * c
    q = np.floor((xyz - origin) / c)
    assert q.dtype == np.float32
    if not np.all(q < 2 ** 21):
        raise IndexRange()
    return q.astype(np.int64)


def partition(xyz, cell_size):
    """-> (order: vertex indices by ascending (z, y, x) cell then index, begin, count per cell, cell id per vertex)."""
    c = cells(xyz, cell_size)
    order = np.lexsort((np.arange(len(c)), c[:, 0], c[:, 1], c[:, 2]))
    cs = c[order]
    first = np.ones(len(cs), bool)
    first[1:] = np.any(cs[1:] != cs[:-1], axis=1)
    begin = np.flatnonzero(first)
    count = np.diff(np.append(begin, len(cs)))
    cid = np.empty(len(c), np.int64)
    cid[order] = np.cumsum(first) - 1
    return order, begin, count, cid


def simplify_clustering(m, cell_size, dtype=np.float64):
    """-> (mesh with xyz / normals in dtype, cell id of every input vertex)."""
    if len(m["xyz"]) == 0:
        return clean(m)[0], np.zeros(0, np.int64)
    order, begin, count, cid = partition(m["xyz"], cell_size)
    n = count.astype(dtype)[:, None]
    xyz = _sequential_sum(m["xyz"].astype(dtype)[order], begin, count, dtype) / n
    nrm = _normalized(_sequential_sum(m["normals"].astype(dtype)[order], begin, count, dtype))
    col = np.add.reduceat(m["rgb"].astype(np.int64)[order], begin, axis=0)
    rgb = ((2 * col + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    out, _ = clean(dict(xyz=xyz, normals=nrm, rgb=rgb, triangles=cid[m["triangles"].astype(np.int64)].astype(np.uint32).reshape(-1, 3)))
    return out, cid
