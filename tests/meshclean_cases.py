"""Hand-made meshes for the mesh clean-up tests (tests/test_meshclean_cpu.py, tests/test_gpu_meshclean.py)."""
import numpy as np

import meshclean_ref as R

TETRA_XYZ = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TETRA_TRI = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)


def _attributes(rng, n):
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    return nrm, rng.integers(0, 256, size=(n, 3)).astype(np.uint8)


def grid(n, spacing=0.1, noise=0.0, seed=0, offset=(0.0, 0.0, 0.0)):
    """An n x n height field over x, y: n^2 vertices, 2 (n - 1)^2 triangles, random normals and colours."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xyz = np.stack([i * spacing, j * spacing, noise * rng.normal(size=(n, n))], -1).reshape(-1, 3) + np.asarray(offset)
    v = (j * n + i)[:-1, :-1].reshape(-1)
    tri = np.concatenate([np.stack([v, v + 1, v + n + 1], 1), np.stack([v, v + n + 1, v + n], 1)])
    nrm, rgb = _attributes(rng, n * n)
    return R.mesh(xyz, tri, nrm, rgb)


def fan(n_tri=70, seed=1):
    """n_tri triangles around vertex 0: its row of the neighbour list has n_tri + 1 entries."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 1.5 * np.pi, n_tri + 1)
    rim = np.stack([np.cos(a), np.sin(a), 0.05 * rng.normal(size=n_tri + 1)], 1)
    xyz = np.concatenate([[[0.0, 0.0, 0.3]], rim])
    k = np.arange(n_tri)
    tri = np.stack([np.zeros(n_tri, np.int64), 1 + k, 2 + k], 1)
    nrm, rgb = _attributes(rng, len(xyz))
    return R.mesh(xyz, tri, nrm, rgb)


def icosphere(subdivisions=3, radius=1.0, center=(0.0, 0.0, 0.0), noise=0.0, seed=2):
    """A closed, outward-oriented sphere: 10 * 4^s + 2 vertices, 20 * 4^s triangles; radial noise of the given sigma."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, g = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    rng = np.random.default_rng(seed)
    unit = np.array(v)
    r = radius + noise * rng.normal(size=len(unit))
    nrm, rgb = _attributes(rng, len(unit))
    return R.mesh(unit * r[:, None] + np.asarray(center), np.array(f), nrm, rgb)


def volume(xyz, tri, center=(0.0, 0.0, 0.0)):
    p = np.asarray(xyz, np.float64) - np.asarray(center)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
