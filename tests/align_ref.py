"""numpy statement of the pose-candidate sweep and the coarse-to-fine search (DESIGN.md section 7o,
include/coxgraph_hip_align.h), from wire arrays.

Per candidate and point: reg_ref.rel_pose (libm cos / sin in double, narrowed to float32 as make_rel_pose does), the float32
transform in reg_point's expression order, track_ref.RefLayer.cell and value_and_gradient for has and val, e = |d - val| and the
quantised contribution in float32, r in float64.  The three integers of a record are exact; cost is a float64 sum in numpy's
order, with the sum of |terms| beside it for the bound on another order (reg_ref.sum_bounds' rule).  grid, select and search
restate the host side of the C ABI operation by operation in Python floats, so poses compare bit for bit.
"""
import itertools
import math

import numpy as np

import reg_ref
from reg_ref import D, F, U, RefLayer  # noqa: F401  (RefLayer is what callers build the reading layer with)

Q = 1024
SCORE_DTYPE = np.dtype([("score", np.uint64), ("n_corr", np.uint32), ("n_inlier", np.uint32), ("cost", np.float64)])
CHUNK_POINTS = 1 << 18   # point evaluations per call of RefLayer.cell


def point_terms(layer, pts, poses_ref, pose_read, tau, no_corr_cost=0.0):
    """Every point of pts [n,5] at every candidate of poses_ref [M,4]: (has bool[M,n], inlier bool[M,n], k int64[M,n], r float64[M,n])."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 5)
    poses_ref = np.asarray(poses_ref, D).reshape(-1, 4)
    n, M = len(pts), len(poses_ref)
    px, py, pz, pd, pw = (pts[:, k] for k in range(5))
    tau = F(tau)
    inv = F(F(1024.0) / tau)
    has, inl = np.zeros((M, n), bool), np.zeros((M, n), bool)
    kk = np.zeros((M, n), np.int64)
    r = np.broadcast_to(pw.astype(D) * D(no_corr_cost), (M, n)).copy()
    per = max(1, CHUNK_POINTS // max(n, 1))
    for c0 in range(0, M, per):
        P = [reg_ref.rel_pose(p, pose_read) for p in poses_ref[c0:c0 + per]]
        R, t = np.stack([p["R"] for p in P]), np.stack([p["t"] for p in P])
        with np.errstate(over="ignore", invalid="ignore"):
            pos = np.stack([((((R[:, 3 * k, None] * px).astype(F) + (R[:, 3 * k + 1, None] * py).astype(F)).astype(F) + (R[:, 3 * k + 2, None] * pz).astype(F)).astype(F)
                             + t[:, k, None]).astype(F) for k in range(3)], -1)
        h, dd, off = layer.cell(pos.reshape(-1, 3))
        val, _ = layer.value_and_gradient(dd, off)
        ci, pi = np.divmod(np.nonzero(h)[0], n)
        ci += c0
        with np.errstate(invalid="ignore"):
            diff = (pd[pi] - val).astype(F)
            e = np.abs(diff)
            ok = e <= tau                    # False for a NaN
            u = np.floor((e[ok] * inv).astype(F)).astype(np.int64)
        has[ci, pi] = True
        inl[ci, pi] = ok
        kk[ci[ok], pi[ok]] = np.maximum(0, Q - u)
        r[ci, pi] = (diff * pw[pi]).astype(F).astype(D)
    return has, inl, kk, r


def sweep(layer, pts, poses_ref, pose_read=(0, 0, 0, 0), tau=0.4, no_corr_cost=0.0, samples=None):
    """cox_align_sweep: (records of SCORE_DTYPE [M], sum_abs float64[M] = 0.5 sum |r^2| unscaled, scale, m).  samples: indices
    into pts with repeats, or None for all points in order."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 5)
    has, inl, kk, r = point_terms(layer, pts, poses_ref, pose_read, tau, no_corr_cost)
    idx = np.arange(len(pts)) if samples is None else np.asarray(samples, np.int64)
    assert len(idx) == 0 or (idx.min() >= 0 and idx.max() < len(pts))
    m = len(idx)
    sum_w = math.fsum(pts[idx, 4].astype(D).tolist())
    scale = m / sum_w if sum_w > 0.0 else 0.0
    mult = np.bincount(idx, minlength=len(pts)).astype(np.int64)   # how often each point is drawn
    rec = np.zeros(len(has), SCORE_DTYPE)
    rec["score"] = (kk * mult).sum(1)
    rec["n_corr"] = (has * mult).sum(1)
    rec["n_inlier"] = (inl * mult).sum(1)
    S = ((r * r) * mult.astype(D)).sum(1)      # m equal terms per drawn point: exact multiples, one rounding each
    rec["cost"] = 0.5 * S * scale * scale
    return rec, 0.5 * S, scale, m


def cost_bound(m, scale, sum_abs):
    """|difference| allowed between two summation orders of the m terms behind cost: 2 m 2^-53 scale^2 sum|terms|"""
    return 2.0 * m * U * scale ** 2 * sum_abs


def _llround(x):
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def grid(center, half_extent, step):
    """cox_align_grid: float64 [n,4], x slowest and yaw fastest."""
    axes = []
    for c, h, s in zip(center, half_extent, step):
        c, h, s = float(c), float(h), float(s)
        mk = _llround(h / s) if s > 0 else 0
        axes.append([c + s * float(j) for j in range(-mk, mk + 1)])
    return np.array(list(itertools.product(*axes)), D).reshape(-1, 4)


def select(rec, min_corr, keep):
    """cox_align_select: indices of the first `keep` eligible records by score descending, then index ascending."""
    el = [int(i) for i in np.nonzero(rec["n_corr"] >= min_corr)[0]]
    el.sort(key=lambda i: (-int(rec["score"][i]), i))
    return np.array(el[:keep], np.uint32)


def search(layer, pts, center, half_extent, step, tau=0.4, tau_min=0.1, keep=8, levels=4, min_corr=0, pose_read=(0, 0, 0, 0), no_corr_cost=0.0, samples=None):
    """cox_align_search: dict(poses [k,4], scores [k], levels=[dict(n_candidates, inlier_distance, step, kept_index, kept_pose, kept_score)])."""
    step = [float(s) for s in step]
    tau = F(tau)
    cand = grid(center, half_extent, step)
    out = []
    for level in range(levels + 1):
        rec, _, _, _ = sweep(layer, pts, cand, pose_read, tau, no_corr_cost, samples)
        idx = select(rec, min_corr, keep)
        kept = cand[idx]
        out.append(dict(n_candidates=len(cand), inlier_distance=float(tau), step=np.array(step), kept_index=idx, kept_pose=kept.copy(), kept_score=rec[idx].copy()))
        if len(idx) == 0 or level == levels:
            break
        step = [s / 2 for s in step]
        tau = max(F(tau / F(2.0)), F(tau_min))
        cand = np.concatenate([grid(p, step, step) for p in kept])
    return dict(poses=out[-1]["kept_pose"], scores=out[-1]["kept_score"], levels=out)


# ---- the analytic room as an alignment problem (tests/test_align_ref_cpu.py, tests/test_gpu_align.py) ---------------------------------
ROOM_VOXEL, ROOM_TRUNCATION = 0.2, 0.6
ROOM_HALF = (1.2, 1.2, 0.4, math.radians(170.0))
ROOM_STEP = (0.4, 0.4, 0.4, math.radians(10.0))
ROOM_SEARCH = dict(tau=0.4, tau_min=0.1, keep=8, levels=4)
ROOM_POINTS = 300
ROOM_SEED = 7
FINAL_STEP = tuple(s / 16 for s in ROOM_STEP)     # 2.5 cm, 0.625 degrees


def room_surface_points(rng, n):
    """n points on the surfaces of synth.py's room and sphere (float64 [n,3], the reading layer's frame): two thirds on the six
    faces of the room by area, a third on the sphere, which is what tells a yaw from the yaw half a turn away."""
    from coxgraph_amd import synth
    lo, hi = synth.ROOM_MIN, synth.ROOM_MAX
    n_sphere = n // 3
    ext = hi - lo
    area = np.array([ext[1] * ext[2], ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[2], ext[0] * ext[1], ext[0] * ext[1]])
    face = rng.choice(6, n - n_sphere, p=area / area.sum())
    q = rng.uniform(lo, hi, (n - n_sphere, 3))
    q[np.arange(len(q)), face // 2] = np.where(face % 2 == 0, lo[face // 2], hi[face // 2])
    v = rng.normal(size=(n_sphere, 3))
    s = synth.SPHERE_C + synth.SPHERE_R * v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([q, s])


def room_true_poses(count, seed=ROOM_SEED):
    """seeded true reference poses inside the search range (90 % of it per axis)"""
    rng = np.random.default_rng(seed)
    return [tuple(float(v) for v in rng.uniform(-0.9, 0.9, 4) * np.array(ROOM_HALF)) for _ in range(count)]


def room_problem(true_pose, seed=ROOM_SEED):
    """The reference point set [300,5] (d = 0, w = 1) that lies on the room's surfaces when the reference submap sits at true_pose
    and the reading submap at the origin."""
    import reg_cases
    q = room_surface_points(np.random.default_rng(seed + 1000), ROOM_POINTS)
    return reg_cases.points_at(q, true_pose, (0.0, 0.0, 0.0, 0.0), np.zeros(len(q)), np.ones(len(q)))


def pose_error_steps(pose, true_pose):
    """|pose - true_pose| per axis in final steps (yaw compared modulo a full turn)"""
    d = np.asarray(pose, D) - np.asarray(true_pose, D)
    d[3] = (d[3] + math.pi) % (2 * math.pi) - math.pi
    return np.abs(d) / np.array(FINAL_STEP)
