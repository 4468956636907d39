"""numpy restatement of the scan-to-map rule (include/coxgraph_hip_track.h), from wire arrays.

Steps 1-3 (transform, considered, used, d, g) are float32, operation by operation as coxgraph_amd/csrc/cox_track.hip's
track_point does them (voxblox's getVoxelsAndQVector cell, the interpolation table, the q vectors and their derivatives), so
every per-point value and decision is comparable bit for bit.  Steps 4-9 are float64: the per-point row x = sqrt(w) [J, r],
the sums of x x^T taken in a selectable point order, the explicit Cholesky of the header comment, the pose update and the
stop rule.  Nothing here is vectorised across iterations or approximated.
"""
import math

import numpy as np

from coxgraph_amd import synth
from history_ref import transform_points

F = np.float32
D = np.float64
EPS = F(1e-6)
CONVERGED, MAX_ITERATIONS, LOST, DEGENERATE = 0, 1, 2, 3
CONSIDERED, USED = 1, 2
DEFAULTS = dict(dof=4, max_iterations=15, stride=1, max_abs_distance=0.0, huber_delta=0.0, damping=1e-6, translation_tolerance=1e-4,
                rotation_tolerance=1e-4, min_points=32, min_inlier_ratio=0.3)
TABLE = np.array([[1, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 1, 0, 0, 0], [-1, 0, 1, 0, 0, 0, 0, 0], [-1, 1, 0, 0, 0, 0, 0, 0],
                  [1, 0, -1, 0, -1, 0, 1, 0], [1, -1, -1, 1, 0, 0, 0, 0], [1, -1, 0, 0, -1, 1, 0, 0], [-1, 1, 1, -1, 1, -1, -1, 1]], F)


def config(**kw):
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def _key(b):
    b = np.asarray(b, np.int64) + (1 << 20)
    return b[..., 0] | (b[..., 1] << 21) | (b[..., 2] << 42)


class RefLayer:
    """A layer from wire arrays (Layer.download() / what Layer.upload takes)."""

    def __init__(self, voxel_size, idx, words):
        self.vs = F(voxel_size)
        self.vs_inv = F(D(1.0) / D(self.vs))
        self.bs = F(self.vs * F(16))
        self.bs_inv = F(D(1.0) / D(self.bs))
        idx = np.asarray(idx, np.int32).reshape(-1, 3)
        words = np.ascontiguousarray(words, np.uint32).reshape(len(idx), 4096, 3)
        keys = _key(idx)
        order = np.argsort(keys)
        self.keys = keys[order]
        self.dist = np.ascontiguousarray(words[order, :, 0]).view(F)
        self.weight = np.ascontiguousarray(words[order, :, 1]).view(F)

    def _find(self, b):
        """-> (found bool[m], position in the sorted block arrays)."""
        k = _key(b)
        if len(self.keys) == 0:
            return np.zeros(len(k), bool), np.zeros(len(k), np.int64)
        pos = np.clip(np.searchsorted(self.keys, k), 0, len(self.keys) - 1)
        return self.keys[pos] == k, pos

    def cell(self, p):
        """voxblox getVoxelsAndQVector at float32 positions p [m,3] in the layer's frame (shared with tests/reg_ref.py):
        -> (valid bool[m], dd [k,8] corner distances and off [k,3] offsets of the k valid points).  Not valid: a coordinate
        that is NaN, +-inf or beyond the packed keys, the block of the point missing, a block of the cell missing, a corner
        of weight <= 0."""
        p = np.ascontiguousarray(p, F).reshape(-1, 3)
        sel = np.arange(len(p))
        with np.errstate(over="ignore", invalid="ignore"):
            sc = (p * self.bs_inv).astype(F)
            ok = ((sc > F(-1048575.0)) & (sc < F(1048575.0))).all(1)  # index_in_range
        sel, p, sc = sel[ok], p[ok], sc[ok]
        b = np.floor((sc + EPS).astype(F)).astype(np.int64)
        found, _ = self._find(b)  # the block of the point must exist
        sel, p, b = sel[found], p[found], b[found]
        valid = np.zeros(len(ok), bool)
        if len(sel) == 0:
            return valid, np.zeros((0, 8), F), np.zeros((0, 3), F)
        # the voxel of the point, one down where the point lies below its centre
        origin = (b.astype(F) * self.bs).astype(F)
        rel = (p - origin).astype(F)
        v = np.clip(np.floor(((rel * self.vs_inv).astype(F) + EPS).astype(F)).astype(np.int64), 0, 15)
        c = (origin + ((v.astype(F) + F(0.5)) * self.vs).astype(F)).astype(F)
        v = v - ((p - c).astype(F) < 0)
        under = v < 0
        b = b - under
        v = v + 16 * under
        c0 = ((b.astype(F) * self.bs).astype(F) + ((v.astype(F) + F(0.5)) * self.vs).astype(F)).astype(F)
        off = ((p - c0).astype(F) * self.vs_inv).astype(F)
        m = len(sel)
        dd, ww, all_blocks = np.zeros((m, 8), F), np.zeros((m, 8), F), np.ones(m, bool)
        for i in range(8):
            vv = v + np.array([(i >> 2) & 1, (i >> 1) & 1, i & 1])
            over = vv >= 16
            f, pos = self._find(b + over)
            vv = vv - 16 * over
            lin = vv[:, 0] + 16 * (vv[:, 1] + 16 * vv[:, 2])
            all_blocks &= f
            dd[:, i] = self.dist[pos, lin] if len(self.keys) else 0
            ww[:, i] = self.weight[pos, lin] if len(self.keys) else 0
        with np.errstate(invalid="ignore"):
            good = all_blocks & (ww > 0).all(1)  # isVoxelValid on all eight
        valid[sel[good]] = True
        return valid, dd[good], off[good]

    def value_and_gradient(self, dd, off):
        """The interpolation table, the q vectors and their derivatives on cell()'s output: -> (val [k], grad [k,3] per
        metre), float32 operation by operation."""
        m = len(dd)
        # M . data, sequential float sums from 0, zero entries included
        md = np.zeros((m, 8), F)
        for r in range(8):
            s = np.zeros(m, F)
            for k in range(8):
                s = (s + (TABLE[r, k] * dd[:, k]).astype(F)).astype(F)
            md[:, r] = s
        dx, dy, dz = off[:, 0], off[:, 1], off[:, 2]
        one, zero = np.ones(m, F), np.zeros(m, F)
        dxy, dyz, dzx = (dx * dy).astype(F), (dy * dz).astype(F), (dz * dx).astype(F)
        q = [one, dx, dy, dz, dxy, dyz, dzx, (dxy * dz).astype(F)]
        qx = [zero, one, zero, zero, dy, zero, dz, dyz]
        qy = [zero, zero, one, zero, dx, dz, zero, dzx]
        qz = [zero, zero, zero, one, zero, dy, dx, dxy]

        def dot(qq):
            s = np.zeros(m, F)
            for i in range(8):
                s = (s + (qq[i] * md[:, i]).astype(F)).astype(F)
            return s
        val = dot(q)
        grad = np.stack([(dot(qx) * self.vs_inv).astype(F), (dot(qy) * self.vs_inv).astype(F), (dot(qz) * self.vs_inv).astype(F)], 1)
        return val, grad

    def per_point(self, T, pts, stride=1, max_abs_distance=0.0):
        """Steps 1-3 at the float32 pose T for scan pts [n,3]: dict(status uint8[n], pG[n,3], d[n], g[n,3]); NaN where the
        matching status bit is clear."""
        T = np.asarray(T, F)
        pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
        n = len(pts)
        status = np.zeros(n, np.uint8)
        pG, d, g = np.full((n, 3), np.nan, F), np.full(n, np.nan, F), np.full((n, 3), np.nan, F)
        ci = np.nonzero((np.arange(n) % stride == 0) & np.isfinite(pts).all(1))[0]
        status[ci] = CONSIDERED
        if len(ci) == 0:
            return dict(status=status, pG=pG, d=d, g=g)
        with np.errstate(over="ignore", invalid="ignore"):
            p = transform_points(T, pts[ci])
            pG[ci] = p
        valid, dd, off = self.cell(p)
        ci = ci[valid]
        val, grad = self.value_and_gradient(dd, off)
        if max_abs_distance > 0:
            keep = np.abs(val) <= F(max_abs_distance)
            ci, val, grad = ci[keep], val[keep], grad[keep]
        status[ci] |= USED
        d[ci], g[ci] = val, grad
        return dict(status=status, pG=pG, d=d, g=g)

    def normal_eq(self, T, pts, cfg, order="forward"):
        """Steps 1-5 at the float32 pose T.  order: "forward", "reverse" or a permutation of the used points' positions.
        -> dict(H[dof,dof], b[dof], cost, n_used, n_considered, abs=(H, b, cost) sums of |terms| for error bounds)."""
        T = np.asarray(T, F)
        dof = cfg["dof"]
        pp = self.per_point(T, pts, cfg["stride"], cfg["max_abs_distance"])
        ui = np.nonzero(pp["status"] & USED)[0]
        if isinstance(order, str):
            ui = ui[::-1] if order == "reverse" else ui
        else:
            ui = ui[np.asarray(order)]
        a = pp["pG"][ui].astype(D) - T[4:7].astype(D)
        g = pp["g"][ui].astype(D)
        r = pp["d"][ui].astype(D)
        axg = np.stack([a[:, 1] * g[:, 2] - a[:, 2] * g[:, 1], a[:, 2] * g[:, 0] - a[:, 0] * g[:, 2], a[:, 0] * g[:, 1] - a[:, 1] * g[:, 0]], 1)
        J = np.concatenate([g, axg], 1) if dof == 6 else np.concatenate([g, axg[:, 2:3]], 1)
        w = np.ones(len(ui), D)
        hd = D(cfg["huber_delta"])
        if hd > 0:
            big = np.abs(r) > hd
            w[big] = hd / np.abs(r[big])
        x = np.sqrt(w)[:, None] * np.concatenate([J, r[:, None]], 1)
        S, A = np.zeros((dof + 1, dof + 1), D), np.zeros((dof + 1, dof + 1), D)
        chunk = 4096  # points are added one after the other in the chosen order
        for s0 in range(0, len(ui), chunk):
            terms = x[s0:s0 + chunk, :, None] * x[s0:s0 + chunk, None, :]
            for t in terms:
                S += t
            A += np.abs(terms).sum(0)
        return dict(H=S[:dof, :dof].copy(), b=S[:dof, dof].copy(), cost=float(S[dof, dof]), n_used=int(len(ui)),
                    n_considered=int((pp["status"] & CONSIDERED).astype(bool).sum()), abs=(A[:dof, :dof].copy(), A[:dof, dof].copy(), float(A[dof, dof])))

    def refine(self, T_prior, pts, cfg, order="forward"):
        """Steps 1-9 from the float32 prior: dict(status, iterations, T float64[7], first_*/last_* of n_used, n_considered, cost,
        last_step_translation, last_step_rotation, steps=[(|dt|, |omega|) per step taken])."""
        T = np.asarray(T_prior, F).astype(D)
        out = dict(status=MAX_ITERATIONS, iterations=0, last_step_translation=0.0, last_step_rotation=0.0, steps=[])
        for k in ("n_used", "n_considered", "cost"):
            out["first_" + k] = out["last_" + k] = 0
        for it in range(cfg["max_iterations"]):
            ne = self.normal_eq(T.astype(F), pts, cfg, order)
            for k in ("n_used", "n_considered", "cost"):
                if it == 0:
                    out["first_" + k] = ne[k]
                out["last_" + k] = ne[k]
            out["iterations"] = it + 1
            if ne["n_used"] < cfg["min_points"] or D(ne["n_used"]) < D(cfg["min_inlier_ratio"]) * D(ne["n_considered"]):
                out["status"] = LOST
                break
            delta = solve(ne["H"], ne["b"], cfg["damping"])
            if delta is None:
                out["status"] = DEGENERATE
                break
            T, st, sr = update(T, delta)
            out["steps"].append((st, sr))
            out["last_step_translation"], out["last_step_rotation"] = st, sr
            if st <= cfg["translation_tolerance"] and sr <= cfg["rotation_tolerance"]:
                out["status"] = CONVERGED
                break
        out["T"] = T
        return out


def solve(H, b, damping):
    """(H + damping diag(H)) delta = -b by the lower Cholesky of include/coxgraph_hip_track.h, loop for loop; None: degenerate."""
    n = len(b)
    H = [[float(H[i][j]) for j in range(n)] for i in range(n)]
    L = [[0.0] * n for _ in range(n)]
    damping = float(damping)
    for j in range(n):
        s = H[j][j] + damping * H[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > 0.0) or not math.isfinite(s):
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, n):
            a = H[i][j]
            for k in range(j):
                a = a - L[i][k] * L[j][k]
            L[i][j] = a / L[j][j]
    y, delta = [0.0] * n, [0.0] * n
    for i in range(n):
        s = -float(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * delta[k]
        delta[i] = s / L[i][i]
    return delta


def update(T, delta):
    """Step 8: t + delta_t, normalize(exp(omega) (x) q); -> (T float64[7], |delta_t|, |omega|)."""
    wx, wy, wz = (delta[3], delta[4], delta[5]) if len(delta) == 6 else (0.0, 0.0, delta[3])
    theta = math.sqrt((wx * wx + wy * wy) + wz * wz)
    half = 0.5 * theta
    sc = math.sin(half) / theta if theta > 0.0 else 0.5
    ew, ex, ey, ez = math.cos(half), sc * wx, sc * wy, sc * wz
    qw, qx, qy, qz = (float(v) for v in T[:4])
    nw = ((ew * qw - ex * qx) - ey * qy) - ez * qz
    nx = ((ew * qx + ex * qw) + ey * qz) - ez * qy
    ny = ((ew * qy - ex * qz) + ey * qw) + ez * qx
    nz = ((ew * qz + ex * qy) - ey * qx) + ez * qw
    nn = math.sqrt(((nw * nw + nx * nx) + ny * ny) + nz * nz)
    out = np.array([nw / nn, nx / nn, ny / nn, nz / nn, float(T[4]) + delta[0], float(T[5]) + delta[1], float(T[6]) + delta[2]], D)
    return out, math.sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]), theta


# ---- poses ----------------------------------------------------------------------------------------------------------------------
def perturbed(T, dt, rotvec):
    """float32 pose: T moved by dt and turned by rotvec (world frame, about the sensor origin)."""
    out, _, _ = update(np.asarray(T, D), list(np.asarray(dt, D)) + list(np.asarray(rotvec, D)))
    return out.astype(F)


def pose_error(T, T_true):
    """(|t - t_true| in metres, rotation between the two in degrees)."""
    T, T_true = np.asarray(T, D), np.asarray(T_true, D)
    qa, qb = T[:4] / np.linalg.norm(T[:4]), T_true[:4] / np.linalg.norm(T_true[:4])
    # vector part of qa (x) conj(qb)
    v = np.array([-qa[0] * qb[1] + qa[1] * qb[0] - qa[2] * qb[3] + qa[3] * qb[2], -qa[0] * qb[2] + qa[1] * qb[3] + qa[2] * qb[0] - qa[3] * qb[1],
                  -qa[0] * qb[3] - qa[1] * qb[2] + qa[2] * qb[1] + qa[3] * qb[0]])
    return float(np.linalg.norm(T[4:] - T_true[4:])), math.degrees(2.0 * math.asin(min(1.0, float(np.linalg.norm(v)))))


# ---- the analytic scene as a layer ------------------------------------------------------------------------------------------------
def analytic_distance(c):
    """Signed distance of synth.py's room and sphere at points c [...,3] (float64): positive in free space."""
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    room = np.minimum.reduce([synth.ROOM_MAX[0] - x, x - synth.ROOM_MIN[0], synth.ROOM_MAX[1] - y, y - synth.ROOM_MIN[1], z - synth.ROOM_MIN[2],
                              synth.ROOM_MAX[2] - z])
    return np.minimum(room, np.linalg.norm(c - synth.SPHERE_C, axis=-1) - synth.SPHERE_R)


def analytic_layer_arrays(voxel_size, truncation=None):
    """Wire arrays (idx, words) of the scene: every voxel centre within truncation + voxel of a surface holds the distance
    clipped to +-truncation with weight 1; all other voxels are unobserved; blocks without an observed voxel are left out."""
    if truncation is None:
        truncation = synth.integrator_overrides(voxel_size)["default_truncation_distance"]
    vs = F(voxel_size)
    bs = float(vs) * 16
    band = truncation + float(vs)
    lo = np.floor((synth.ROOM_MIN - band) / bs).astype(int)
    hi = np.floor((synth.ROOM_MAX + band) / bs).astype(int)
    lin = np.arange(4096)
    vloc = np.stack([lin & 15, (lin >> 4) & 15, lin >> 8], 1).astype(F)
    idx, words = [], []
    for bz in range(lo[2], hi[2] + 1):
        for by in range(lo[1], hi[1] + 1):
            for bx in range(lo[0], hi[0] + 1):
                b = np.array([bx, by, bz], F)
                cen = ((b * (vs * F(16))).astype(F) + ((vloc + F(0.5)) * vs).astype(F)).astype(F)
                dist = analytic_distance(cen.astype(D))
                obs = np.abs(dist) <= band
                if not obs.any():
                    continue
                w = np.zeros((4096, 3), np.uint32)
                w[:, 0] = np.clip(dist, -truncation, truncation).astype(F).view(np.uint32)
                w[:, 1] = obs.astype(F).view(np.uint32)
                idx.append((bx, by, bz))
                words.append(w)
    return np.array(idx, np.int32), np.stack(words)


# ---- start poses of the convergence tests -------------------------------------------------------------------------------------------
def start_pose(T, voxel_size, dof, voxels, degrees, sign=1):
    """T moved by `voxels` voxels along (0.6, -0.6, 0.5) and turned by `degrees` about z (4 DoF: yaw is all that can be recovered)
    or about (0.3, -0.5, 0.8) (6 DoF); sign -1 reverses both."""
    dt = np.array([0.6, -0.6, 0.5])
    axis = np.array([0.0, 0.0, 1.0]) if dof == 4 else np.array([0.3, -0.5, 0.8])
    return perturbed(T, sign * dt / np.linalg.norm(dt) * voxels * voxel_size, sign * axis / np.linalg.norm(axis) * math.radians(degrees))


def decision_margin(steps, cfg):
    """How far the stop decision of every step taken is from flipping: the smallest of max(v, 1 / v) over the steps, v =
    max(|dt| / translation_tolerance, |omega| / rotation_tolerance).  Above 2, iteration counts can be compared."""
    m = float("inf")
    for st, sr in steps:
        v = max(st / cfg["translation_tolerance"], sr / cfg["rotation_tolerance"])
        m = min(m, max(v, 1.0 / v) if v > 0 else float("inf"))
    return m
