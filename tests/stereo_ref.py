"""The rule of a dense-stereo frame restated in numpy, the structures of
include/coxgraph_hip_stereo.h restated in ctypes, and the scene the stereo tests share.  The GPU owes this file every bit."""
import ctypes as C
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]
NO_CENSUS_COST = 62
INVALID = 0xFFFF
RECT_LEFT, RECT_RIGHT, COST_SUM, DISPARITY = 0, 1, 2, 3

DEFAULTS = dict(n_disparities=128, n_paths=8, p1=7, p2=86, uniqueness_percent=10, lr_max_diff=1, min_depth_m=0.0, max_depth_m=float("inf"), reserved=0)


class Config(C.Structure):
    _fields_ = [("n_disparities", C.c_int32), ("n_paths", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("uniqueness_percent", C.c_int32),
                ("lr_max_diff", C.c_int32), ("min_depth_m", C.c_float), ("max_depth_m", C.c_float), ("reserved", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_valid_pixels", "n_rejected_uniqueness", "n_rejected_lr", "n_rejected_depth")] + \
               [(n, C.c_double) for n in ("remap_ms", "census_ms", "paths_ms", "winner_ms", "depth_ms", "frame_ms")]


class Camera(C.Structure):
    _fields_ = [("camera_model", C.c_int32), ("distortion_model", C.c_int32), ("intrinsics", C.c_double * 4), ("distortion_coeffs", C.c_double * 4)]


class Calibration(C.Structure):
    _fields_ = [("cam", Camera * 2), ("T_cn_cnm1", C.c_double * 16)]


def euroc_camchain():
    """the numbers of coxgraph/config/euroc/euroc_camchain.yaml"""
    with open(os.path.join(HERE, "golden", "euroc_camchain.json")) as f:
        return json.load(f)


def ideal_camchain(f=100.0, cx=40.0, cy=30.0, baseline=0.1):
    cam = dict(camera_model="pinhole", distortion_model="radtan", intrinsics=[f, f, cx, cy], distortion_coeffs=[0.0, 0.0, 0.0, 0.0])
    T = np.eye(4)
    T[0, 3] = -baseline
    return dict(cam0=dict(cam), cam1=dict(cam, T_cn_cnm1=T.tolist()))


# ---- step R ------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.sqrt(np.sum(v * v))


def rectification(chain, scale=1.0):
    """R_rect (cam0 -> rect), f, cx, cy, B, R, t of a camchain"""
    T = np.asarray(chain["cam1"]["T_cn_cnm1"], np.float64)
    R, t = T[:3, :3], T[:3, 3]
    b = -(R.T @ t)
    B = np.sqrt(np.sum(b * b))
    e1 = b / B
    zm = _unit(np.array([0.0, 0.0, 1.0]) + R.T @ np.array([0.0, 0.0, 1.0]))
    e2 = _unit(np.cross(zm, e1))
    e3 = np.cross(e1, e2)
    k0, k1 = chain["cam0"]["intrinsics"], chain["cam1"]["intrinsics"]
    f = scale * (k0[0] + k0[1] + k1[0] + k1[1]) / 4.0
    return np.stack([e1, e2, e3]), f, (k0[2] + k1[2]) / 2.0, (k0[3] + k1[3]) / 2.0, B, R, t


def distort_project(cam, x, y):
    """normalised image coordinates -> raw pixel of a pinhole + radtan camera (float64)"""
    fx, fy, cx, cy = cam["intrinsics"]
    k1, k2, p1, p2 = cam["distortion_coeffs"]
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * r2 * r2
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def map_at(chain, cam_index, u, v, scale=1.0):
    """the map of camera cam_index at rectified pixel coordinates (u, v), which need not be integers: float64, NaN behind the camera"""
    Rr, f, cx, cy, _, R, _ = rectification(chain, scale)
    M = Rr.T if cam_index == 0 else R @ Rr.T
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    rx, ry = (u - cx) / f, (v - cy) / f
    p = [M[i, 0] * rx + M[i, 1] * ry + M[i, 2] for i in range(3)]
    with np.errstate(all="ignore"):
        mx, my = distort_project(chain["cam%d" % cam_index], p[0] / p[2], p[1] / p[2])
    behind = ~(p[2] > 0.0)
    return np.where(behind, np.nan, mx), np.where(behind, np.nan, my)


def quaternion_of(M):
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    assert tr > 0.0  # the rectifying rotations of a forward-looking pair are small
    s = np.sqrt(tr + 1.0) * 2.0
    q = np.array([0.25 * s, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s])
    return q / np.sqrt(np.sum(q * q))


def rectify_maps(chain, w, h, scale=1.0):
    """step R: map0, map1 float32 [h, w, 2], K_rect float32[4], baseline float32, T_c0_rect float32[7]"""
    Rr, f, cx, cy, B, _, _ = rectification(chain, scale)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    maps = [np.stack(map_at(chain, i, u, v, scale), -1).astype(np.float32) for i in (0, 1)]
    T = np.concatenate([quaternion_of(Rr.T), [0.0, 0.0, 0.0]]).astype(np.float32)
    return maps[0], maps[1], np.array([f, f, cx, cy], np.float32), np.float32(B), T


# ---- step 1 ------------------------------------------------------------------------------------------------------------------------
def remap(img, map_xy):
    """-> (rectified u8 [h, w], masked bool [h, w]); map_xy None: the image itself, nothing masked"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    if map_xy is None:
        return img.copy(), np.zeros((h, w), bool)
    m = np.asarray(map_xy, np.float32)
    with np.errstate(all="ignore"):
        fx = np.floor(m[..., 0] * np.float32(32.0) + np.float32(0.5))
        fy = np.floor(m[..., 1] * np.float32(32.0) + np.float32(0.5))
        inside = np.isfinite(m[..., 0]) & np.isfinite(m[..., 1]) & (fx >= 0) & (fx <= 32 * (w - 1)) & (fy >= 0) & (fy <= 32 * (h - 1))
    ix, iy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
    x0, ax, y0, ay = ix >> 5, ix & 31, iy >> 5, iy & 31
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    g = img.astype(np.int64)
    out = (g[y0, x0] * (32 - ax) * (32 - ay) + g[y0, x1] * ax * (32 - ay) + g[y1, x0] * (32 - ax) * ay + g[y1, x1] * ax * ay + 512) >> 10
    return np.where(inside, out, 0).astype(np.uint8), ~inside


# ---- step 2 ------------------------------------------------------------------------------------------------------------------------
def census(img):
    """-> (62-bit words uint64 [h, w], has-a-census bool [h, w])"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    words, has = np.zeros((h, w), np.uint64), np.zeros((h, w), bool)
    if w < 9 or h < 7:
        return words, has
    has[3:h - 3, 4:w - 4] = True
    centre = img[3:h - 3, 4:w - 4]
    acc, bit = np.zeros(centre.shape, np.uint64), 0
    for dy in range(7):
        for dx in range(9):
            if (dy, dx) == (3, 4):
                continue
            acc |= (img[dy:dy + h - 6, dx:dx + w - 8] < centre).astype(np.uint64) << np.uint64(bit)
            bit += 1
    words[3:h - 3, 4:w - 4] = acc
    return words, has


# ---- step 3 ------------------------------------------------------------------------------------------------------------------------
def cost_volume(cl, hl, cr, hr, D):
    h, w = cl.shape
    Cv = np.full((h, w, D), NO_CENSUS_COST, np.int32)
    for d in range(min(D, w)):
        both = hl[:, d:] & hr[:, :w - d]
        Cv[:, d:, d] = np.where(both, np.bitwise_count(cl[:, d:] ^ cr[:, :w - d]).astype(np.int32), NO_CENSUS_COST)
    return Cv


# ---- step 4 ------------------------------------------------------------------------------------------------------------------------
def _path_step(Lq, Cp, p1, p2):
    """Lq, Cp [n, D] -> L(p, .)"""
    big = np.int32(1 << 14)
    m = Lq.min(axis=1, keepdims=True)
    below = np.concatenate([np.full_like(Lq[:, :1], big), Lq[:, :-1]], 1)
    above = np.concatenate([Lq[:, 1:], np.full_like(Lq[:, :1], big)], 1)
    return Cp + np.minimum(np.minimum(Lq, m + p2), np.minimum(below, above) + p1) - m


def aggregate(Cv, n_paths, p1, p2):
    h, w, D = Cv.shape
    S = np.zeros((h, w, D), np.int32)
    for dx, dy in DIRECTIONS[:n_paths]:
        L = np.empty_like(Cv)
        if dy == 0:
            xs = range(w) if dx > 0 else range(w - 1, -1, -1)
            for i, x in enumerate(xs):
                L[:, x] = Cv[:, x] if i == 0 else _path_step(L[:, x - dx], Cv[:, x], p1, p2)
        else:
            ys = range(h) if dy > 0 else range(h - 1, -1, -1)
            for i, y in enumerate(ys):
                L[y] = Cv[y]  # the pixels whose predecessor is outside keep this
                if i == 0:
                    continue
                # x with 0 <= x - dx < w
                lo, hi = max(0, dx), min(w, w + dx)
                if hi > lo:
                    L[y, lo:hi] = _path_step(L[y - dy, lo - dx:hi - dx], Cv[y, lo:hi], p1, p2)
        S += L
    return S


# ---- steps 5-8 ---------------------------------------------------------------------------------------------------------------------
def winner(S, uniqueness):
    """-> d0, m0, rejected-by-uniqueness"""
    D = S.shape[2]
    d0 = np.argmin(S, axis=2)
    m0 = np.take_along_axis(S, d0[..., None], 2)[..., 0]
    far = np.abs(np.arange(D)[None, None, :] - d0[..., None]) > 1
    rejected = np.any(far & (S.astype(np.int64) * (100 - uniqueness) < m0[..., None].astype(np.int64) * 100), axis=2)
    return d0, m0, rejected


def right_disparity(S):
    h, w, D = S.shape
    SR = np.full((h, w, D), np.iinfo(np.int32).max, np.int32)
    for d in range(min(D, w)):
        SR[:, :w - d, d] = S[:, d:, d]
    return np.argmin(SR, axis=2)


def subpixel(S, d0, m0):
    D = S.shape[2]
    inner = (d0 > 0) & (d0 < D - 1)
    sm = np.take_along_axis(S, np.clip(d0 - 1, 0, D - 1)[..., None], 2)[..., 0].astype(np.int64)
    sp = np.take_along_axis(S, np.clip(d0 + 1, 0, D - 1)[..., None], 2)[..., 0].astype(np.int64)
    den = np.maximum(sm + sp - 2 * m0, 1)
    num = (sm - sp) * 16 + den
    frac = np.sign(num) * (np.abs(num) // (2 * den))  # C's division truncates toward zero
    return np.where(inner, 16 * d0 + frac, 16 * d0)


def match(left, right, K_rect, baseline_m, map0=None, map1=None, **cfg):
    """One frame.  -> dict(rect_left, rect_right, cost_sum u16, disparity u16, depth f32, rgba u8, stats)"""
    c = dict(DEFAULTS, **cfg)
    D = c["n_disparities"]
    rl, masked = remap(left, map0)
    rr, _ = remap(right, map1)
    h, w = rl.shape
    cl, hl = census(rl)
    cr, hr = census(rr)
    S = aggregate(cost_volume(cl, hl, cr, hr, D), c["n_paths"], c["p1"], c["p2"])
    d0, m0, rej_u = winner(S, c["uniqueness_percent"])
    rej_lr = np.zeros((h, w), bool)
    if c["lr_max_diff"] >= 0:
        dR = right_disparity(S)
        xr = np.arange(w)[None, :] - d0
        rej_lr = (xr < 0) | (np.abs(np.take_along_axis(dR, np.clip(xr, 0, w - 1), 1) - d0) > c["lr_max_diff"])
    d16 = subpixel(S, d0, m0.astype(np.int64))
    usable = hl & ~masked
    valid = usable & ~rej_u & ~rej_lr & (d16 > 0)
    disparity = np.where(valid, d16, INVALID).astype(np.uint16)
    fB16 = np.float32(float(np.float32(K_rect[0])) * float(np.float32(baseline_m)) * 16.0)
    with np.errstate(all="ignore"):
        z = fB16 / np.where(valid, d16, 1).astype(np.float32)
    assert z.dtype == np.float32
    outside = valid & ((z < np.float32(c["min_depth_m"])) | (z > np.float32(c["max_depth_m"])))
    depth = np.where(valid & ~outside, z, np.float32(np.nan)).astype(np.float32)
    rgba = np.stack([rl, rl, rl, np.full_like(rl, 255)], -1)
    stats = dict(n_valid_pixels=int(np.sum(valid & ~outside)), n_rejected_uniqueness=int(np.sum(usable & rej_u)),
                 n_rejected_lr=int(np.sum(usable & ~rej_u & rej_lr)), n_rejected_depth=int(np.sum(outside)))
    return dict(rect_left=rl, rect_right=rr, cost_sum=S.astype(np.uint16), disparity=disparity, depth=depth, rgba=rgba, stats=stats)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
BACKGROUND, FOREGROUND = 8, 24
SCENE_K = np.array([120.0, 120.0, 80.0, 48.0], np.float32)
SCENE_BASELINE = np.float32(0.11)


def _smooth(a):
    """separable 1-2-1, borders replicated"""
    p = np.pad(a.astype(np.int64), 1, mode="edge")
    p = (p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:] + 2) >> 2
    return ((p[:-2] + 2 * p[1:-1] + p[2:] + 2) >> 2).astype(np.uint8)


def scene(w, h, seed=0):
    """-> left, right u8 [h, w], the left image's true disparity int [h, w]: a plane at 8 px, a box at 24 px in the central
    third x half; the right image is independent noise painted with right[y, x - d] = left[y, x], the plane first"""
    rng = np.random.default_rng(seed)
    left = _smooth(rng.integers(0, 256, (h, w)))
    right = _smooth(rng.integers(0, 256, (h, w)))
    truth = np.full((h, w), BACKGROUND, np.int64)
    truth[h // 4:h - h // 4, w // 3:w - w // 3] = FOREGROUND
    for d in (BACKGROUND, FOREGROUND):
        ys, xs = np.nonzero((truth == d) & (np.arange(w)[None, :] - d >= 0))
        right[ys, xs - d] = left[ys, xs]
    return left, right, truth


def constant_pair(w, h, value=100):
    a = np.full((h, w), value, np.uint8)
    return a, a.copy()


def stripes_pair(w, h, period=8):
    a = np.broadcast_to(np.where((np.arange(w) % period) < period // 2, 200, 50).astype(np.uint8), (h, w)).copy()
    return a, a.copy()
