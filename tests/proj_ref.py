"""An independent float64 restatement of voxblox's ProjectiveTsdfIntegrator, for checking the oracle and the HIP kernels.

Written from the DESCRIPTION of the integrator, not from the oracle's or the kernel's code:
  [S]  SURVEY.md Appendix A.7b (lines 675-685): range image by spherical projection storing |p_C|; blocks along each ray;
       per voxel of every touched block: project the centre, interpolate the range (nearest / min-neighbour / bilinear /
       adaptive), sdf = range - |voxel_C|, skip sdf < -trunc, weight 1 or 1/d^2 with linear drop-off behind the surface,
       running mean with min(trunc, sdf), cap at max_weight; de-integration.
  [O]  the rule list in the header comment of oracle/cox_oracle_projective.hpp (lines 8-24): altitude = asin(z / r),
       azimuth = atan2(y, x); a pixel keeps the smallest range; points within [min_ray, max_ray] mark the blocks on the ray
       from (r + truncation) * bearing back to the sensor; a POINT's pixel truncates, a VOXEL keeps the fraction; rows
       outside [0, rows - 1] and columns outside (0, cols - 1) are rejected; adaptive = bilinear unless the 2 x 2 spans
       more than adaptive_gap (then its smallest) or holds an empty pixel (then the nearest pixel); sdf > trunc is skipped
       without carving; a new weight below 1e-6 leaves the voxel alone; de-integration adds the negated observation and
       a voxel whose weight falls below 1 goes back to unobserved.
Everything is vectorised numpy in float64: the rotation is a 3 x 3 matrix built from the quaternion, the pose inverse is that
matrix transposed, the angles are np.arcsin / np.arctan2.

AMBIGUITY.  float32 code may take a discrete decision the other way where the float64 quantity lies close to the
threshold.  Such voxels (and counters, and blocks) are reported, not compared.  The margin is RELATIVE 2^-18 of the
compared quantity: about 30 float32 ulp, i.e. the handful of rounded operations between the inputs and a decision, with
slack.  It was fixed before any run and is not tuned on anybody's output.  Image coordinates are differences / products of
quantities as large as the image (h = (H - 1) (0.5 - altitude / fov), w = W azimuth / 2 pi, + W when negative), so their
margin is 2^-18 of the image extent (H - 1 and W), in pixels.  Ambiguity is sticky across frames.
"""
import numpy as np

MARGIN = 2.0 ** -18
K_EPS = 1e-6
VPS = 16


def rotation_matrix(q):
    """3 x 3 rotation of the quaternion (w, x, y, z)."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def make_cfg(voxel_size, truncation, rows, cols, fov_deg, scheme=3, adaptive_gap=0.5, max_weight=10000.0, min_ray=0.1, max_ray=5.0,
             const_weight=True, carving=True, dropoff=True):
    f32 = lambda v: float(np.float32(v))  # the engine holds these as floats
    return dict(voxel_size=f32(voxel_size), truncation=f32(truncation), rows=int(rows), cols=int(cols), fov_rad=f32(np.float32(fov_deg)) * np.pi / 180.0,
                scheme=int(scheme), adaptive_gap=f32(adaptive_gap), max_weight=f32(max_weight), min_ray=f32(min_ray), max_ray=f32(max_ray),
                const_weight=bool(const_weight), carving=bool(carving), dropoff=bool(dropoff))


def _project(v, cfg):
    """[O] bearing -> (h, w, r, inside, near a limit of the image).  v: [n, 3] in the sensor frame."""
    H, W = cfg["rows"], cfg["cols"]
    r = np.sqrt(np.sum(v * v, axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        altitude = np.arcsin(np.clip(v[:, 2] / r, -1.0, 1.0))
    azimuth = np.arctan2(v[:, 1], v[:, 0])
    h = (H - 1) * (0.5 - altitude / cfg["fov_rad"])
    w = W * azimuth / (2.0 * np.pi)
    w = np.where(w < 0.0, w + W, w)
    mh, mw = MARGIN * (H - 1), MARGIN * W
    with np.errstate(invalid="ignore"):
        inside = (h >= 0.0) & (h <= H - 1) & (w > 0.0) & (w < W - 1)
        # the seam itself: an azimuth within the margin of zero may come out negative and wrap to the other end of the image
        near = (np.abs(h) <= mh) | (np.abs(h - (H - 1)) <= mh) | (np.abs(w) <= mw) | (np.abs(w - (W - 1)) <= mw) | (np.abs(w - W) <= mw)
    return h, w, r, inside, near


def range_image(points, cfg):
    """[S](1) + [O]: the frame's range image.  -> dict(img [H, W] with inf for 'no return', pix_amb [H, W], n_valid, n_rays,
    counts_ambiguous, casts [n], cast_amb [n])."""
    H, W = cfg["rows"], cfg["cols"]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    img = np.full((H, W), np.inf)
    pix_amb = np.zeros((H, W), bool)
    finite = np.all(np.isfinite(p), axis=1)
    h, w, r, inside, near = _project(np.where(finite[:, None], p, 1.0), cfg)
    usable = finite & (r <= 3.0e38) & ~(r < K_EPS)
    counts_amb = bool(np.any(finite & (np.abs(r - K_EPS) <= MARGIN * K_EPS)))
    valid = usable & inside
    counts_amb |= bool(np.any(usable & near))
    hi, wi = np.floor(np.where(valid, h, 0.0)).astype(np.int64), np.floor(np.where(valid, w, 0.0)).astype(np.int64)
    hi = np.minimum(hi, H - 1)
    np.minimum.at(img, (hi[valid], wi[valid]), r[valid])
    # points that float32 may put into another pixel (or reject): the pixels whose minimum that would change
    mh, mw = MARGIN * (H - 1), MARGIN * W
    fh, fw = h - np.floor(h), w - np.floor(w)
    with np.errstate(invalid="ignore"):
        bh, bw = (fh <= mh) | (fh >= 1.0 - mh), (fw <= mw) | (fw >= 1.0 - mw)
    for i in np.nonzero(usable & (inside | near) & (bh | bw | near))[0]:
        h_alt = [int(np.floor(h[i]))] + ([int(np.floor(h[i] + 2 * mh)), int(np.floor(h[i] - 2 * mh))] if bh[i] or near[i] else [])
        w_alt = [int(np.floor(w[i]))] + ([int(np.floor(w[i] + 2 * mw)), int(np.floor(w[i] - 2 * mw))] if bw[i] or near[i] else [])
        for a in set(h_alt):
            for b in set(w_alt):
                if 0 <= a < H and 0 <= b < W and r[i] <= img[a, b]:
                    pix_amb[a, b] = True  # the point is this pixel's minimum, or would become it
    with np.errstate(invalid="ignore"):
        casts = valid & (cfg["min_ray"] <= r) & (r <= cfg["max_ray"])
        cast_amb = usable & (inside | near) & (near | (np.abs(r - cfg["min_ray"]) <= MARGIN * cfg["min_ray"]) | (np.abs(r - cfg["max_ray"]) <= MARGIN * cfg["max_ray"]))
    return dict(img=img, pix_amb=pix_amb, n_valid=int(valid.sum()), n_rays=int(casts.sum()), counts_ambiguous=counts_amb or bool(np.any(cast_amb)),
                casts=casts, cast_amb=cast_amb, r=r)


def mark_blocks(T_G_C, points, ri, cfg, candidates):
    """[S](2) + [O]: geometric block marking.  For every cast ray the segment sensor -> (r + trunc) * bearing, in block units; a
    candidate block is REQUIRED when a ray that certainly casts crosses the block shrunk by the margin, ALLOWED when any ray that
    may cast comes within the margin of it (slab test)."""
    cand = np.asarray(candidates, np.float64).reshape(-1, 3)
    required, allowed = np.zeros(len(cand), bool), np.zeros(len(cand), bool)
    sel = ri["casts"] | ri["cast_amb"]
    if not sel.any() or not len(cand):
        return required, allowed
    p = np.asarray(points, np.float64).reshape(-1, 3)[sel]
    r = ri["r"][sel]
    certain = (ri["casts"] & ~ri["cast_amb"])[sel]
    R, t = rotation_matrix(T_G_C[:4]), np.asarray(T_G_C[4:7], np.float64)
    bs = cfg["voxel_size"] * VPS
    start = (t / bs)[None, :]
    end = ((p * ((r + cfg["truncation"]) / r)[:, None]) @ R.T + t) / bs
    for c0 in range(0, len(p), 256):
        e = end[c0:c0 + 256][:, None, :]
        s = np.broadcast_to(start[:, None, :], e.shape)
        eps = MARGIN * np.maximum(1.0, np.maximum(np.abs(e).max(axis=2), np.abs(s).max(axis=2)))[..., None]
        d = e - s
        for grow, out, rows in ((-1.0, required, certain[c0:c0 + 256]), (1.0, allowed, None)):
            lo, hi = cand[None, :, :] - grow * eps, cand[None, :, :] + 1.0 + grow * eps
            with np.errstate(divide="ignore", invalid="ignore"):
                t1, t2 = (lo - s) / d, (hi - s) / d
            par = d == 0.0  # parallel to the slab: inside it for every t, or for none
            t_in = np.where(par, np.where((s >= lo) & (s <= hi), -np.inf, np.inf), np.minimum(t1, t2))
            t_out = np.where(par, np.where((s >= lo) & (s <= hi), np.inf, -np.inf), np.maximum(t1, t2))
            hit = np.maximum(t_in.max(axis=2), 0.0) <= np.minimum(t_out.min(axis=2), 1.0)
            if rows is not None:
                hit = hit & rows[:, None]
            out |= hit.any(axis=0)
    return required, allowed


def _interpolate(ri, h, w, cfg):
    """[S](3) + [O]: the range at fractional pixel (h, w) -> (range with 0 for 'no return', ambiguous)."""
    H, W, scheme = cfg["rows"], cfg["cols"], cfg["scheme"]
    img = np.where(np.isinf(ri["img"]), 0.0, ri["img"])
    pa = ri["pix_amb"]
    mh, mw = MARGIN * (H - 1), MARGIN * W
    h0, w0 = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
    hr, wr = np.minimum(np.floor(h + 0.5).astype(np.int64), H - 1), np.minimum(np.floor(w + 0.5).astype(np.int64), W - 1)  # round half up: h, w >= 0
    nearest, nearest_amb = img[hr, wr], pa[hr, wr] | (np.abs(h - h0 - 0.5) <= mh) | (np.abs(w - w0 - 0.5) <= mw)
    if scheme == 0:
        return nearest, nearest_amb
    edge = (h0 + 1 >= H) | (w0 + 1 >= W)
    h1, w1 = np.minimum(h0 + 1, H - 1), np.minimum(w0 + 1, W - 1)
    a, b, c, d = img[h0, w0], img[h0, w1], img[h1, w0], img[h1, w1]
    amb4 = pa[h0, w0] | pa[h0, w1] | pa[h1, w0] | pa[h1, w1]
    mn, mx = np.minimum(np.minimum(a, b), np.minimum(c, d)), np.maximum(np.maximum(a, b), np.maximum(c, d))
    dh, dw = h - h0, w - w0
    border = (dh <= mh) | (dh >= 1.0 - mh) | (dw <= mw) | (dw >= 1.0 - mw)
    bil = (a * (1.0 - dh) + c * dh) * (1.0 - dw) + (b * (1.0 - dh) + d * dh) * dw
    if scheme == 1:
        out, amb = mn, amb4 | border
    else:
        empty = mn < K_EPS
        gap = (scheme == 3) & (mx - mn > cfg["adaptive_gap"])
        out = np.where(empty, nearest, np.where(gap, mn, bil))
        amb = amb4 | (empty & nearest_amb)
        if scheme == 3:
            amb = amb | border | (~empty & (np.abs((mx - mn) - cfg["adaptive_gap"]) <= MARGIN * np.maximum(mx, cfg["adaptive_gap"])))
        else:
            # bilinear is continuous across cells; what is not is the switch to the nearest pixel next to an empty one:
            # on a cell border, ambiguous when the neighbouring cells hold an empty pixel
            hm, hp = np.clip(np.floor(h - 2 * mh).astype(np.int64), 0, H - 1), np.clip(np.floor(h + 2 * mh).astype(np.int64) + 1, 0, H - 1)
            wm, wp = np.clip(np.floor(w - 2 * mw).astype(np.int64), 0, W - 1), np.clip(np.floor(w + 2 * mw).astype(np.int64) + 1, 0, W - 1)
            any_empty = np.zeros(len(h), bool)
            for hh in (hm, h0, hp):
                for ww in (wm, w0, wp):
                    any_empty |= img[hh, ww] < K_EPS
            amb = amb | (border & any_empty)
    return np.where(edge, a, out), np.where(edge, pa[h0, w0], amb)


def voxel_centres(blocks, voxel_size):
    """[n_blocks, 4096, 3] centres; linear voxel order x fastest."""
    lin = np.arange(VPS ** 3)
    loc = np.stack([lin % VPS, (lin // VPS) % VPS, lin // (VPS * VPS)], axis=1)
    return ((np.asarray(blocks, np.int64)[:, None, :] * VPS + loc[None, :, :]).astype(np.float64) + 0.5) * voxel_size


def run(frames, cfg, blocks, candidates=None):
    """frames: [(T_G_C [7], points [n, 3], deintegrate)]; blocks: [nb, 3] block indices to evaluate.
    -> dict(distance, weight, ambiguous, updated: [nb, 4096]; frames: per frame dict(n_valid, n_rays, counts_ambiguous, required, allowed);
            required, allowed: boolean over `candidates` (default: the blocks), over all frames)."""
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    cand = blocks if candidates is None else np.asarray(candidates, np.int64).reshape(-1, 3)
    key = lambda b: {tuple(int(v) for v in row): i for i, row in enumerate(b)}
    cand_of = key(cand)
    nb = len(blocks)
    D, Wt = np.zeros((nb, VPS ** 3)), np.zeros((nb, VPS ** 3))
    amb, updated = np.zeros((nb, VPS ** 3), bool), np.zeros((nb, VPS ** 3), bool)
    centres = voxel_centres(blocks, cfg["voxel_size"]).reshape(-1, 3)
    trunc, vs = cfg["truncation"], cfg["voxel_size"]
    per_frame = []
    req_all, alw_all = np.zeros(len(cand), bool), np.zeros(len(cand), bool)
    for T, pts, deintegrate in frames:
        T = np.asarray(T, np.float64)
        ri = range_image(pts, cfg)
        required, allowed = mark_blocks(T, pts, ri, cfg, cand)
        req_all |= required
        alw_all |= allowed
        per_frame.append(dict(n_valid=ri["n_valid"], n_rays=ri["n_rays"], counts_ambiguous=ri["counts_ambiguous"], required=required, allowed=allowed))
        blk_req = np.array([required[cand_of[tuple(int(v) for v in b)]] if tuple(int(v) for v in b) in cand_of else False for b in blocks], bool)
        blk_alw = np.array([allowed[cand_of[tuple(int(v) for v in b)]] if tuple(int(v) for v in b) in cand_of else False for b in blocks], bool)
        sel = np.repeat(blk_alw, VPS ** 3)
        if not sel.any():
            continue
        ix = np.nonzero(sel)[0]
        uncertain_block = np.repeat(blk_alw & ~blk_req, VPS ** 3)[ix]
        R, t = rotation_matrix(T[:4]), T[4:7]
        q = (centres[ix] - t) @ R  # R^T (c - t): the pose inverse by the transposed matrix
        h, w, dv, inside, near = _project(q, cfg)
        a = near.copy()
        ok = inside & (dv >= cfg["min_ray"]) & (dv <= cfg["max_ray"])
        a |= (np.abs(dv - cfg["min_ray"]) <= MARGIN * cfg["min_ray"]) | (np.abs(dv - cfg["max_ray"]) <= MARGIN * cfg["max_ray"])
        hs, ws = np.where(inside, h, 0.0), np.where(inside, w, 1.0)
        rng, ramb = _interpolate(ri, hs, ws, cfg)
        sdf = rng - dv
        m_sdf = MARGIN * np.maximum(np.maximum(rng, dv), trunc)
        ok_sdf = sdf >= -trunc
        a_sdf = np.abs(sdf + trunc) <= m_sdf
        if not cfg["carving"]:
            ok_sdf &= sdf <= trunc
            a_sdf |= np.abs(sdf - trunc) <= m_sdf

        def observation(s):
            obs = np.full(len(s), -1.0 if deintegrate else 1.0)
            if cfg["dropoff"]:
                obs = np.where(s < -vs, np.maximum(obs * ((trunc + s) / (trunc - vs)), 0.0), obs)
            return obs if cfg["const_weight"] else obs / (dv * dv)

        obs = observation(sdf)
        ow, od = Wt.reshape(-1)[ix], D.reshape(-1)[ix]
        nw = np.minimum(ow + obs, cfg["max_weight"])
        thr = 1.0 if deintegrate else K_EPS
        # the weight threshold, under the uncertainty of the sdf that the observation is made from
        a_w = np.zeros(len(ix), bool)
        for s_alt in (sdf - m_sdf, sdf + m_sdf):
            nw_alt = np.minimum(ow + observation(s_alt), cfg["max_weight"])
            a_w |= (nw_alt < thr) != (nw < thr)
        a_w |= np.abs(nw - thr) <= MARGIN * np.maximum(np.maximum(np.abs(ow), np.abs(obs)), thr)
        takes = ok & ok_sdf
        if deintegrate:
            reset = takes & (nw < 1.0)
            write = takes & ~reset & ~(nw < K_EPS)
        else:
            reset = np.zeros(len(ix), bool)
            write = takes & ~(nw < K_EPS)
        with np.errstate(invalid="ignore", divide="ignore"):
            nd = (od * ow + np.minimum(trunc, sdf) * obs) / nw
        D.reshape(-1)[ix] = np.where(reset, 0.0, np.where(write, nd, od))
        Wt.reshape(-1)[ix] = np.where(reset, 0.0, np.where(write, nw, ow))
        # ambiguous: a decision on the way to this voxel's update was close -- only where one of the two outcomes is an update
        maybe = inside | near
        close = maybe & (a | (ok & (ramb | a_sdf)) | (takes & a_w))
        close |= uncertain_block & (reset | write)
        amb.reshape(-1)[ix] |= close
        updated.reshape(-1)[ix] |= reset | write
    return dict(distance=D, weight=Wt, ambiguous=amb, updated=updated, frames=per_frame, required=req_all, allowed=alw_all)


def candidate_blocks(frames, cfg):
    """Every block index in the bounding box of the frames' ray segments (+ 1 block), for mark_blocks."""
    bs = cfg["voxel_size"] * VPS
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for T, pts, _ in frames:
        T = np.asarray(T, np.float64)
        p = np.asarray(pts, np.float64).reshape(-1, 3)
        p = p[np.all(np.isfinite(p), axis=1)]
        r = np.linalg.norm(p, axis=1)
        p, r = p[(r > K_EPS) & (r <= cfg["max_ray"] * (1 + MARGIN))], r[(r > K_EPS) & (r <= cfg["max_ray"] * (1 + MARGIN))]
        e = (p * ((r + cfg["truncation"]) / r)[:, None]) @ rotation_matrix(T[:4]).T + T[4:7]
        for v in (e, T[4:7][None, :]):
            if len(v):
                lo, hi = np.minimum(lo, v.min(axis=0)), np.maximum(hi, v.max(axis=0))
    if not np.all(np.isfinite(lo)):
        return np.zeros((0, 3), np.int64)
    lo, hi = np.floor(lo / bs).astype(np.int64) - 1, np.floor(hi / bs).astype(np.int64) + 1
    g = np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)
