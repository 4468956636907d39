"""Plain numpy references of finishSubmap() (ESDF, surface box, weighted sampler, isosurface points), written from the rules of
DESIGN.md section 3 / 7b.  Nothing here imports or shares code with oracle/ or the kernels: every function works on the wire
arrays of Layer.download() (block_idx int32[n,3], words uint32[n,4096,3]) scattered into one dense padded array.

Block coordinates are compacted per axis before the scatter (runs of consecutive indices stay consecutive, any larger gap
becomes one empty block), so adjacency is preserved and a layer with blocks at -2^20 and 2^20-1 still fits in memory.
"""
import itertools
from typing import NamedTuple

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24   # unit round-off of float32
VPS = 16

# Worst-case overestimate of the {1, sqrt 2, sqrt 3} 26-neighbour chamfer metric.  A shortest lattice path for a displacement
# (a >= b >= c >= 0, in voxels) takes c space diagonals, b - c face diagonals and a - b axis steps, so its length is
#   a + (sqrt 2 - 1) b + (sqrt 3 - sqrt 2) c = v . (a, b, c),   v = (1, sqrt 2 - 1, sqrt 3 - sqrt 2).
# v itself is ordered (1 > 0.414 > 0.318), so the maximum of v . u over unit vectors u of the cone a >= b >= c is |v|:
#   1 + q = sqrt(1 + (sqrt 2 - 1)^2 + (sqrt 3 - sqrt 2)^2) = 1.12809...,   q = 12.81 %.
CHAMFER_Q = float(np.sqrt(1.0 + (np.sqrt(2.0) - 1.0) ** 2 + (np.sqrt(3.0) - np.sqrt(2.0)) ** 2) - 1.0)


class Dense:
    """Scatter / gather between wire arrays and one dense [z, y, x] array with a one-voxel pad."""

    def __init__(self, idx):
        idx = np.asarray(idx, np.int64).reshape(-1, 3)
        self.idx = idx
        self.coords, self.ranks = [], []
        for k in range(3):
            u = np.unique(idx[:, k]) if len(idx) else np.zeros(0, np.int64)
            r = np.zeros(len(u), np.int64)
            if len(u) > 1:
                r[1:] = np.cumsum(np.minimum(np.diff(u), 2))
            self.coords.append(u)
            self.ranks.append(r)
        nb = [int(r[-1]) + 1 if len(r) else 0 for r in self.ranks]
        self.shape = tuple(VPS * nb[k] + 2 for k in (2, 1, 0))
        self.rank = np.stack([self.block_rank(idx[:, k], k) for k in range(3)], axis=1) if len(idx) else np.zeros((0, 3), np.int64)
        self.present = self.scatter(np.ones((len(idx), VPS ** 3), bool), False)

    def block_rank(self, b, k):
        """dense block rank of block coordinate b on axis k, -1 where no block of the layer has that coordinate"""
        b = np.asarray(b, np.int64)
        u = self.coords[k]
        if len(u) == 0:
            return np.full(b.shape, -1, np.int64)
        p = np.clip(np.searchsorted(u, b), 0, len(u) - 1)
        return np.where(u[p] == b, self.ranks[k][p], -1)

    def _blocks(self, a):
        nz, ny, nx = [(s - 2) // VPS for s in self.shape]
        return a[1:-1, 1:-1, 1:-1].reshape(nz, VPS, ny, VPS, nx, VPS)

    def scatter(self, per_block, fill):
        per_block = np.asarray(per_block)
        a = np.full(self.shape, fill, per_block.dtype)
        v = self._blocks(a)
        for i, (rx, ry, rz) in enumerate(self.rank):
            v[rz, :, ry, :, rx, :] = per_block[i].reshape(VPS, VPS, VPS)
        return a

    def gather(self, a):
        v = self._blocks(a)
        out = np.zeros((len(self.rank), VPS ** 3), a.dtype)
        for i, (rx, ry, rz) in enumerate(self.rank):
            out[i] = v[rz, :, ry, :, rx, :].reshape(-1)
        return out

    def lookup(self, g):
        """global voxel indices int64[n,3] (x, y, z) -> dense (z, y, x) indices and a mask of those inside a present block"""
        g = np.asarray(g, np.int64)
        r = [self.block_rank(g[:, k] >> 4, k) for k in range(3)]
        ok = (r[0] >= 0) & (r[1] >= 0) & (r[2] >= 0)
        d = [np.where(ok, VPS * r[k] + (g[:, k] & 15) + 1, 0) for k in range(3)]
        ok &= self.present[d[2], d[1], d[0]]
        return (d[2], d[1], d[0]), ok

    def centres(self, voxel_size):
        """float64 voxel centres [n,4096,3] on the ideal grid (g + 0.5) * voxel_size"""
        lin = np.arange(VPS ** 3)
        loc = np.stack([lin % VPS, (lin // VPS) % VPS, lin // (VPS * VPS)], axis=1)
        return ((self.idx[:, None, :] * VPS + loc[None]).astype(np.float64) + 0.5) * float(F32(voxel_size))


def fields(vox):
    vox = np.ascontiguousarray(vox, np.uint32)
    return vox[..., 0].copy().view(F32), vox[..., 1].copy().view(F32)


# ---- ESDF ------------------------------------------------------------------------------------------------------------------
class EsdfRef(NamedTuple):
    distance: np.ndarray   # float32 [n,4096]
    observed: np.ndarray   # bool
    fixed: np.ndarray      # bool
    sweeps: int
    initial: np.ndarray    # float32 [n,4096], the field before any propagation

    def words(self):
        w = np.zeros(self.distance.shape + (3,), np.uint32)
        w[..., 0] = self.distance.view(np.uint32)
        w[..., 1] = np.where(self.observed, F32(1.0), F32(0.0)).astype(F32).view(np.uint32)
        w[..., 2] = self.fixed.astype(np.uint32)
        return w


OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]   # (dz, dy, dx)


def _shift(a, o):
    """view of a's interior displaced by o: element [i] is a[i + 1 + o]"""
    return a[tuple(slice(1 + k, a.shape[j] - 1 + k) for j, k in enumerate(o))]


def esdf_ref(idx, vox, voxel_size, max_d, min_d, default_d, min_weight, max_sweeps=100000):
    """Observed iff not w < min_weight; fixed iff |d| < min_d; other observed voxels start at +-default_d by d > 0; a source
    with |d| < max_d offers d + step (d > 0) to larger voxels or d - step (any other d) to smaller ones, step = voxel_size *
    {1, sqrt 2, sqrt 3} formed and added in float32; fixed and unobserved voxels never change.  Whole-array relaxation (one
    neighbour direction at a time, in place) until no bit changes: values only move towards zero, so the order of the updates
    cannot change the fixed point."""
    G = Dense(idx)
    d, w = fields(vox)
    vs, max_d, min_d, default_d, min_weight = F32(voxel_size), F32(max_d), F32(min_d), F32(default_d), F32(min_weight)
    with np.errstate(invalid="ignore"):
        obs_b = ~(w < min_weight)
        fixed_b = obs_b & (np.abs(d) < min_d)
        e_b = np.where(fixed_b, d, np.where(d > 0, default_d, -default_d)).astype(F32)
    e_b[~obs_b] = 0.0
    e = G.scatter(e_b, F32(0))
    obs = G.scatter(obs_b, False)
    movable = G.scatter(obs_b & ~fixed_b, False)[1:-1, 1:-1, 1:-1]
    steps = {1: F32(1.0) * vs, 2: np.sqrt(F32(2.0)) * vs, 3: np.sqrt(F32(3.0)) * vs}
    inner = e[1:-1, 1:-1, 1:-1]
    sweeps = 0
    full_movable = np.zeros(G.shape, bool)
    full_movable[1:-1, 1:-1, 1:-1] = movable
    mi = np.flatnonzero(full_movable)
    if inner.size and 4 * len(mi) < inner.size:
        # few movable voxels (a corridor through unobserved space): the same relaxation on their index list only
        flat, obs_flat = e.reshape(-1), obs.reshape(-1)
        while len(mi):
            before = flat[mi].copy()
            for o in OFFSETS:
                step = steps[abs(o[0]) + abs(o[1]) + abs(o[2])]
                ni = mi + (o[0] * G.shape[1] + o[1]) * G.shape[2] + o[2]
                src = flat[ni]
                ok = obs_flat[ni] & (np.abs(src) < max_d)
                pos = ok & (src > 0)
                lo = np.where(pos, src + step, F32(np.inf)).astype(F32)
                hi = np.where(ok & ~pos, src - step, F32(-np.inf)).astype(F32)
                cur = flat[mi]
                cur = np.where(cur > lo, lo, cur)
                flat[mi] = np.where(cur < hi, hi, cur)
            sweeps += 1
            if np.array_equal(before.view(np.uint32), flat[mi].view(np.uint32)):
                break
            assert sweeps < max_sweeps, "esdf_ref does not converge"
    elif inner.size:
        while True:
            before = inner.copy()
            for o in OFFSETS:
                step = steps[abs(o[0]) + abs(o[1]) + abs(o[2])]
                src = _shift(e, o)
                ok = _shift(obs, o) & (np.abs(src) < max_d) & movable
                pos = ok & (src > 0)
                lo = np.where(pos, src + step, F32(np.inf)).astype(F32)
                hi = np.where(ok & ~pos, src - step, F32(-np.inf)).astype(F32)
                np.copyto(inner, lo, where=inner > lo)
                np.copyto(inner, hi, where=inner < hi)
            sweeps += 1
            if np.array_equal(before.view(np.uint32), inner.view(np.uint32)):
                break
            assert sweeps < max_sweeps, "esdf_ref does not converge"
    return EsdfRef(G.gather(e), obs_b, fixed_b, sweeps, e_b)


# ---- analytic fields and the bound that rests on no propagation rule ---------------------------------------------------------
def analytic_sdf(prims, c):
    """min over disjoint solids of their exact signed distance at float64 points c[...,3] -> (sdf, nearest surface point).
    prims: ("plane", normal, offset) is the half space n.x < offset, ("sphere", centre, radius) the ball.  For DISJOINT solids
    the minimum is the exact signed distance to the union's surface on both sides."""
    best, near = None, None
    for kind, a, b in prims:
        a = np.asarray(a, np.float64)
        if kind == "plane":
            n = a / np.linalg.norm(a)
            s = c @ n - b
            p = c - s[..., None] * n
        else:
            v = c - a
            r = np.linalg.norm(v, axis=-1)
            s = r - b
            u = np.where(r[..., None] > 1e-12, v / np.maximum(r[..., None], 1e-12), np.array([1.0, 0.0, 0.0]))
            p = a + b * u
        if best is None:
            best, near = s, p
        else:
            m = s < best
            best, near = np.where(m, s, best), np.where(m[..., None], p, near)
    return best, near


def _dilate(a, n):
    for _ in range(n):
        b = a.copy()
        for ax in range(3):
            for sh in (-1, 1):
                r = np.roll(a, sh, axis=ax)
                sl = [slice(None)] * 3
                sl[ax] = 0 if sh == 1 else -1
                r[tuple(sl)] = False
                b |= r
            a = b.copy()
    return a


def esdf_true_bounds(idx, ref_distance, observed, fixed, initial, prims, voxel_size, max_d, min_d, name=""):
    """For an analytic field (exact signed distance of disjoint planes / spheres, stored unclamped inside the fixed band) and the
    ESDF `ref_distance` of any engine: for every reached (moved off its initial value), non-fixed voxel x with true distance t

        |esdf(x)| >= t - E_lo                       (always)
        |esdf(x)| <= (1 + q) t + E_up               (if the straight way to the nearest surface point lies in observed space)

    Lower bound: |esdf(x)| = |d_s| + (path length from a fixed seed s) >= t(s) + |x - s| >= t(x), the true distance being
    1-Lipschitz; only float32 rounding is lost: at most N = max_d / voxel_size + 2 additions of values below max_d and N
    rounded steps, E_lo = 2 N 2^-24 max_d.
    Upper bound: needs min_d > sqrt 3 voxel (asserted).  Let p be x's nearest surface point, r = sqrt 3 / 2 voxel (half a voxel
    diagonal) and y the point of the segment x-p at true distance rho = r (+ epsilon).  The voxel centre s nearest to y has
    |s - y| <= r, so 0 < t(s) <= 2 r < min_d: s is a fixed seed of x's sign holding t(s) exactly.  A lattice path s -> x is at
    most (1 + q) |x - s| long, so |esdf(x)| <= t(s) + (1 + q) |x - s| <= (rho + r) + (1 + q)(t - rho + r)
    <= (1 + q) t + (2 + q) r: E_up = (2 + q) sqrt 3 / 2 voxel = 1.843 voxel (the fixed band's discretisation).
    A shortest lattice path is monotone along every axis, so it stays inside the box spanned by s and x, hence inside the
    layer's bounding box as long as the segment does.  Its steps can be ordered to follow the line s - x: the moves of the
    middle axis within half a voxel, those of the minor axis (which must ride on a middle-axis move) within one and a half;
    the line is within half a voxel per axis of the segment and a sample of the segment within half a voxel of the centre of
    the voxel it falls in: less than 2.5 voxels (Chebyshev) in all.  x is excluded when the segment leaves the bounding box,
    when a voxel within two voxels of the voxels it crosses is unobserved or missing (share of the reached voxels printed and
    capped at 20 %).  Where (1 + q) t + E_up reaches max_d the bound says nothing (values at or beyond the maximum do not
    propagate): those voxels get the lower bound only, and their share of the reached voxels is printed too."""
    h = float(F32(voxel_size))
    assert float(min_d) > np.sqrt(3.0) * h, "the upper bound needs a fixed band thicker than one voxel diagonal"
    G = Dense(idx)
    c = G.centres(voxel_size)
    true, near = analytic_sdf(prims, c)
    d = ref_distance.astype(np.float64)
    reached = observed & ~fixed & (ref_distance.view(np.uint32) != initial.view(np.uint32))
    n_reached = int(reached.sum())
    t = np.abs(true)
    e_lo = 2.0 * (float(max_d) / h + 2.0) * U24 * float(max_d)
    e_up = (2.0 + CHAMFER_Q) * np.sqrt(3.0) / 2.0 * h
    assert np.all(np.sign(d[reached]) == np.sign(true[reached])), "a reached voxel has the wrong sign"
    low = (t - np.abs(d))[reached]
    assert low.max(initial=-np.inf) <= e_lo, (name, "esdf below the true distance by", low.max())
    # upper bound: the segment stays in the bounding box and every voxel within two voxels of it is observed
    blocked = np.ones(G.shape, bool)
    blocked[1:-1, 1:-1, 1:-1] = _dilate(~G.scatter(observed, False)[1:-1, 1:-1, 1:-1], 2)
    room = (1.0 + CHAMFER_Q) * t + e_up < float(max_d)
    n_beyond = int((reached & ~room).sum())      # the upper bound itself reaches max_d there: it says nothing
    sel = np.argwhere(reached & room)
    x, p = c[sel[:, 0], sel[:, 1]], near[sel[:, 0], sel[:, 1]]
    bad = np.zeros(len(sel), bool)
    n_samp = int(np.ceil(float(max_d) / (0.5 * h))) + 1
    for f in np.linspace(0.0, 1.0, n_samp):
        g = np.floor((x + f * (p - x)) / h).astype(np.int64)
        (dz, dy, dx), ok = G.lookup(g)
        bad |= ~ok | blocked[dz, dy, dx]
    n_sel, n_bad = len(sel), int(bad.sum())
    keep = sel[~bad]
    dd, tt = np.abs(d[keep[:, 0], keep[:, 1]]), t[keep[:, 0], keep[:, 1]]
    ratio_raw = float(np.max(dd / tt)) if len(keep) else 0.0
    ratio_net = float(np.max((dd - e_up) / tt)) if len(keep) else 0.0
    # one denominator for the print and the cap: the reached voxels
    share, share_beyond = n_bad / max(n_reached, 1), n_beyond / max(n_reached, 1)
    print(f"[true bounds {name}] reached {n_reached}: upper bound on {n_sel - n_bad}, {share:.1%} excluded (way to the surface blocked), {share_beyond:.1%} "
          f"beyond the reach of the bound ((1 + q) t + E_up >= max); worst true - |esdf| = {low.max(initial=0.0):.2e} (E_lo {e_lo:.2e}); "
          f"worst |esdf| / true = {ratio_raw:.4f}, worst (|esdf| - E_up) / true = {ratio_net:.4f} (1 + q = {1 + CHAMFER_Q:.4f})")
    assert share <= 0.2, (name, "excluded share", n_bad, n_reached)
    assert ratio_net <= 1.0 + CHAMFER_Q, (name, ratio_net)
    return dict(reached=n_reached, checked=n_sel - n_bad, excluded_share=share, beyond_share=share_beyond, worst_low=float(low.max(initial=0.0)), ratio_raw=ratio_raw, ratio_net=ratio_net)


# ---- surface box -------------------------------------------------------------------------------------------------------------
def center_coord(i, size):
    """(float(idx) + 0.5) * size: evaluated in double, narrowed to float"""
    return ((np.asarray(i).astype(F32).astype(np.float64) + 0.5) * np.float64(F32(size))).astype(F32)


def surface_obb_ref(idx, vox, voxel_size):
    """min / max over observed voxels (weight > 1e-6) with |d| <= voxel_size of centre -/+ half a voxel; the centre is
    float(block) * block_size + centre coordinate, all float32 -> (min[3], max[3], count); +-inf when there is none."""
    d, w = fields(vox)
    vs = F32(voxel_size)
    with np.errstate(invalid="ignore"):
        m = (w > F32(1e-6)) & (np.abs(d) <= vs)
    block_size = vs * F32(VPS)
    half = F32(0.5) * vs
    lin = np.arange(VPS ** 3)
    loc = np.stack([lin % VPS, (lin // VPS) % VPS, lin // (VPS * VPS)], axis=1)
    mn, mx = np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
    bi, vi = np.nonzero(m)
    for k in range(3):
        if len(bi):
            c = (np.asarray(idx)[bi, k].astype(F32) * block_size + center_coord(loc[vi, k], vs)).astype(F32)
            mn[k], mx[k] = (c - half).min(), (c + half).max()
    return mn, mx, int(m.sum())


# ---- weighted sampler --------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sampler_ref(weights, n, seed):
    """Python integers only: floor(w 2^20) fixed-point weights (0 unless w > 0), exact cumulative sums, draw i =
    splitmix64(seed * 0x9E3779B97F4A7C15 + i), scaled to [0, total) by a 128-bit multiply-high, index = first cumulative sum
    strictly above it (upper bound).  All indices are 0 when the total is 0."""
    import bisect
    cum, run = [], 0
    for w in np.asarray(weights, F32).tolist():
        run += int(w * 1048576.0) if w > 0.0 else 0   # float32 -> double product is exact below 2^53
        cum.append(run)
    out = np.zeros(n, np.uint32)
    if run == 0:
        return out
    for i in range(n):
        r = splitmix64(((seed * 0x9E3779B97F4A7C15) + i) & M64)
        out[i] = bisect.bisect_right(cum, (r * run) >> 64)
    return out


# ---- isosurface points -------------------------------------------------------------------------------------------------------
def round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


class IsoRef(NamedTuple):
    n_mesh_vertices: int
    n_connected: int
    points: np.ndarray       # float64 [n,5]: survivor xyz (exactly the soup's float32 values), distance, weight
    xyz32: np.ndarray        # float32 [n,3]
    near_boundary: int       # soup vertices within one float32 ulp of a proximity-cell boundary
    tol_scale: float         # multiply by the field magnitude: bound on the engines' float32 interpolation error


def isosurface_ref(ref_mesh, idx, vox, voxel_size, min_weight, threshold):
    """Vertex soup of the independent mesher reference in mesh order; merged "first in mesh order wins" on the proximity grid
    (cell = round-half-away(double(v) / threshold), in float64); (distance, weight) trilinear in float64 at the survivors that
    have all 8 neighbours present with weight > 0.  The cell an engine interpolates in is decided by float32 comparisons that
    DESIGN.md states (block = floor(p / block_size + 1e-6), voxel = floor((p - origin) / voxel_size + 1e-6) clamped to the
    block, one down where p - centre < 0); they are restated here with numpy float32, because marching-cubes vertices lie ON
    voxel-centre planes in two of three axes and only that rule says which of the two equally good cells is meant."""
    soup = ref_mesh.mesh(voxel_size, idx, vox, min_weight)["xyz"]
    nv = len(soup)
    thr = np.float64(F32(threshold))
    inv = 1.0 / thr
    scaled = soup.astype(np.float64) * inv
    frac = np.abs(np.abs(scaled - np.floor(scaled)) - 0.5)
    near = int(np.any(frac <= np.abs(scaled) * 2.0 * U24, axis=1).sum()) if nv else 0
    cells = round_half_away(scaled).astype(np.int64)
    if nv:
        _, first = np.unique(cells, axis=0, return_index=True)
        first = np.sort(first)
    else:
        first = np.zeros(0, np.int64)
    p = soup[first]
    G = Dense(idx)
    d, w = fields(vox)
    D, W = G.scatter(d.astype(np.float64), 0.0), G.scatter(w.astype(np.float64), 0.0)
    vs = F32(voxel_size)
    vs_inv, bs = F32(1.0 / np.float64(vs)), vs * F32(VPS)
    bs_inv, eps = F32(1.0 / np.float64(bs)), F32(1e-6)
    b = np.floor(p * bs_inv + eps).astype(np.int64)
    origin = (b.astype(F32) * bs).astype(F32)
    vi = np.clip(np.floor((p - origin).astype(F32) * vs_inv + eps).astype(np.int64), 0, VPS - 1)
    centre = (origin + center_coord(vi, vs)).astype(F32)
    own = G.lookup(VPS * b + vi)[1]                                     # the block of the point itself exists
    base = VPS * b + vi - ((p - centre).astype(F32) < 0)
    h = np.float64(vs)
    off = np.clip(p.astype(np.float64) / h - (base + 0.5), 0.0, 1.0)
    valid = own.copy()
    dv, wv = np.zeros(len(p)), np.zeros(len(p))
    for o in itertools.product((0, 1), repeat=3):
        (dz, dy, dx), ok = G.lookup(base + np.array(o))
        wt = np.prod(np.where(np.array(o) == 1, off, 1.0 - off), axis=1)
        with np.errstate(invalid="ignore"):
            valid &= ok & (W[dz, dy, dx] > 0)
        dv += wt * D[dz, dy, dx]
        wv += wt * W[dz, dy, dx]
    pts = np.concatenate([p[valid].astype(np.float64), dv[valid, None], wv[valid, None]], axis=1)
    # float32 error of the engines' value q . (M . f) against the exact trilinear value, per unit of F = max |f|:
    #  * M . f: 8 rows, each a sequential sum of 8 terms +-f_i: |row| <= 8 F, rounding <= 7 u 8 F = 56 u F per row;
    #  * q has products of up to three offsets in [0, 1]: 2 u each; the 8 products q_i md_i add u each: (2 + 1) u 8 F 8 = 192 u F,
    #    and the rows' own 56 u F enter with |q_i| <= 1: 448 u F;  the final sequential sum of 8 terms: 7 u 64 F = 448 u F;
    #  * the offset (p - c0) / voxel: c0 = float(block) block_size + centre coordinate carries 3 u |coordinate|, the subtraction
    #    and the product by the rounded 1 / voxel 3 u more: 3 u (|coordinate| / voxel + 1) per axis; a trilinear interpolant
    #    moves by at most 2 F per unit offset and axis: 18 u F (|coordinate| / voxel + 1).
    coord = float(np.max(np.abs(p))) / float(h) if len(p) else 0.0
    tol_scale = U24 * (56 * 8 + 192 + 448 + 18.0 * (coord + 1.0))
    return IsoRef(nv, len(first), pts, p[valid], near, tol_scale)
