"""numpy restatement of the submap registration cost (coxgraph_amd/csrc/cox_reg.hip), from wire arrays.

The relative pose is computed in Python floats with math.cos / math.sin (the libm the library's host code calls) and narrowed
to float32 as make_rel_pose does.  The per-point transform and the interpolation are float32, operation by operation
(track_ref.RefLayer.cell / value_and_gradient: voxblox's getVoxelsAndQVector cell, the table, the q vectors); the residual and
the eight Jacobian entries are float64 in reg_point's expression order, without fused operations.  So every per-point value
and decision is comparable bit for bit; only the order of the sums (sum of weights, H, b, cost) is free.

affine_truth() is the closed form for a layer that holds an affine field: fully float64, derivatives written from the
rotation matrices, nothing shared with the restatement above.
"""
import math

import numpy as np

from track_ref import D, F, RefLayer  # noqa: F401  (RefLayer is what callers build the reading layer with)

U = 2.0 ** -53


def _cs(yaw):
    """cos, sin as C's libm gives them (NaN for a non-finite angle, where math.cos raises)"""
    yaw = float(yaw)
    return (math.cos(yaw), math.sin(yaw)) if math.isfinite(yaw) else (math.nan, math.nan)


def rel_pose(pose_ref, pose_read):
    """make_rel_pose: dict(R float32[9], t float32[3], cf, sf, cr, sr, tf, tr)"""
    ref, read = [float(v) for v in pose_ref], [float(v) for v in pose_read]
    (cf, sf), (cr, sr) = _cs(ref[3]), _cs(read[3])
    c, s = cr * cf + sr * sf, cr * sf - sr * cf
    dx, dy, dz = ref[0] - read[0], ref[1] - read[1], ref[2] - read[2]
    with np.errstate(over="ignore", invalid="ignore"):
        R = np.array([c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0], D).astype(F)
        t = np.array([cr * dx + sr * dy, -sr * dx + cr * dy, dz], D).astype(F)
    return dict(R=R, t=t, cf=cf, sf=sf, cr=cr, sr=sr, tf=ref[:3], tr=read[:3])


def per_point(layer, pts, pose_ref, pose_read, no_corr_cost=0.0):
    """reg_point for every row of pts [n,5] = x, y, z, distance, weight against the RefLayer `layer`:
    dict(r float64[n], J float64[n,8] = J_ref | J_read, has bool[n], w float32[n], pos float32[n,3]), all unscaled."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 5)
    P = rel_pose(pose_ref, pose_read)
    R, t = P["R"], P["t"]
    px, py, pz, pd, pw = (pts[:, k] for k in range(5))
    with np.errstate(over="ignore", invalid="ignore"):
        pos = np.stack([((((R[3 * k] * px).astype(F) + (R[3 * k + 1] * py).astype(F)).astype(F) + (R[3 * k + 2] * pz).astype(F)).astype(F) + t[k]).astype(F)
                        for k in range(3)], 1)
    has, dd, off = layer.cell(pos)
    val, grad = layer.value_and_gradient(dd, off)
    n = len(pts)
    r = pw.astype(D) * D(no_corr_cost)
    J = np.zeros((n, 8), D)
    hi = np.nonzero(has)[0]
    r[hi] = (((pd[hi] - val).astype(F)) * pw[hi]).astype(F).astype(D)
    w, gx, gy, gz = pw[hi].astype(D), grad[:, 0].astype(D), grad[:, 1].astype(D), grad[:, 2].astype(D)
    x, y = px[hi].astype(D), py[hi].astype(D)
    cf, sf, cr, sr, tf, tr = P["cf"], P["sf"], P["cr"], P["sr"], P["tf"], P["tr"]
    gRx, gRy, gRz = gx * cr - gy * sr, gx * sr + gy * cr, gz
    dRfp_x, dRfp_y = -sf * x - cf * y, cf * x - sf * y
    qxx, qyy = (cf * x - sf * y) + tf[0] - tr[0], (sf * x + cf * y) + tf[1] - tr[1]
    dpr_x, dpr_y = -sr * qxx + cr * qyy, -cr * qxx - sr * qyy
    J[hi, 0], J[hi, 1], J[hi, 2] = -w * gRx, -w * gRy, -w * gRz
    J[hi, 3] = -w * (gRx * dRfp_x + gRy * dRfp_y)
    J[hi, 4], J[hi, 5], J[hi, 6] = w * gRx, w * gRy, w * gRz
    J[hi, 7] = -w * (gx * dpr_x + gy * dpr_y)
    return dict(r=r, J=J, has=has, w=pw.copy(), pos=pos)


def _gather(pp, n_pts, sample_idx):
    idx = np.arange(n_pts) if sample_idx is None else np.asarray(sample_idx, np.int64)
    assert len(idx) == 0 or (idx.min() >= 0 and idx.max() < n_pts)
    w = pp["w"][idx]
    sum_w = math.fsum(w.astype(D).tolist())
    scale = len(idx) / sum_w if sum_w > 0.0 else 0.0
    return idx, w, sum_w, scale


def evaluate(layer, pts, pose_ref, pose_read, sample_idx=None, no_corr_cost=0.0, pp=None):
    """cox_reg_evaluate: dict(r[n], J_ref[n,4], J_read[n,4], has[n]) scaled by n_res / sum(w) as the C ABI does, plus the
    unscaled r0, J0 [n,8], the weights w, sum_w (math.fsum) and scale.  pp: a per_point() result to reuse."""
    pp = per_point(layer, pts, pose_ref, pose_read, no_corr_cost) if pp is None else pp
    idx, w, sum_w, scale = _gather(pp, len(pp["r"]), sample_idx)
    r0, J0 = pp["r"][idx], pp["J"][idx]
    r, J = r0 * scale, J0 * scale
    return dict(r=r, J_ref=J[:, :4].copy(), J_read=J[:, 4:].copy(), has=pp["has"][idx], r0=r0, J0=J0, w=w, sum_w=sum_w, scale=scale)


def normal_eq(layer, pts, pose_ref, pose_read, sample_idx=None, no_corr_cost=0.0, pp=None):
    """cox_reg_normal_eq: dict(H[8,8], b[8], cost, n_corr, n, scale, abs=(H, b, cost) sums of |terms|, unscaled, for the
    bound on another summation order)."""
    ev = evaluate(layer, pts, pose_ref, pose_read, sample_idx, no_corr_cost, pp)
    x = np.concatenate([ev["J0"], ev["r0"][:, None]], 1)
    S, A = np.zeros((9, 9), D), np.zeros((9, 9), D)
    for s0 in range(0, len(x), 32768):
        terms = x[s0:s0 + 32768, :, None] * x[s0:s0 + 32768, None, :]
        S += terms.sum(0)
        A += np.abs(terms).sum(0)
    sc = ev["scale"]
    return dict(H=S[:8, :8] * sc * sc, b=S[:8, 8] * sc * sc, cost=float(0.5 * S[8, 8] * sc * sc), n_corr=int(ev["has"].sum()), n=len(x), scale=sc,
                abs=(A[:8, :8].copy(), A[:8, 8].copy(), float(0.5 * A[8, 8])))


def sum_bounds(ne):
    """|difference| allowed between two summation orders of the n products behind H, b and cost: 2 n 2^-53 sum|terms| scale^2"""
    k = 2.0 * ne["n"] * U * ne["scale"] ** 2
    return k * ne["abs"][0], k * ne["abs"][1], k * ne["abs"][2]


# ---- closed form for an affine field --------------------------------------------------------------------------------------------
def _rz(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], D)


def _drz(yaw):
    """d Rz / d yaw"""
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[-s, -c, 0.0], [c, -s, 0.0], [0.0, 0.0, 0.0]], D)


def affine_truth(a, c, pts, pose_ref, pose_read, jacobians=True):
    """The cost against a layer holding d(x) = a . x + c, whose trilinear interpolation is the field itself:
    r_i = w_i (d_i - (a . (Rz(yaw_r)^T (Rz(yaw_f) p_i + t_f - t_r)) + c)) and its derivatives by the four components of
    each pose, float64, unscaled.  -> (r[n], J[n,8] or None)"""
    pts = np.asarray(pts, D).reshape(-1, 5)
    a, c = np.asarray(a, D), float(c)
    pf, pr = np.asarray(pose_ref, D), np.asarray(pose_read, D)
    p, d, w = pts[:, :3], pts[:, 3], pts[:, 4]
    Rf, Rr = _rz(float(pf[3])), _rz(float(pr[3]))
    v = p @ Rf.T + (pf[:3] - pr[:3])      # in the world frame, relative to the reading submap's origin
    r = w * (d - ((v @ Rr) @ a + c))      # (v @ Rr) = rows of Rr^T v
    if not jacobians:
        return r, None
    u = Rr @ a                            # a . (Rr^T v) = (Rr a) . v
    J = np.zeros((len(pts), 8), D)
    J[:, 0:3] = -w[:, None] * u[None, :]                  # d v / d t_f = I
    J[:, 3] = -w * ((p @ _drz(float(pf[3])).T) @ u)       # d v / d yaw_f = dRz(yaw_f) p
    J[:, 4:7] = w[:, None] * u[None, :]                   # d v / d t_r = -I
    J[:, 7] = -w * ((v @ _drz(float(pr[3]))) @ a)         # d (Rr^T v) / d yaw_r = dRz(yaw_r)^T v
    return r, J
