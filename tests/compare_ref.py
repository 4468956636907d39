"""numpy statement of the layer compare (include/coxgraph_hip_compare.h), from wire arrays.

Every voxel of test layer A with weight > min_weight: its centre as map_ref.voxel_centres forms it, the float32 transform in
layer_ref._rotate's expression order, a point sample of reference layer B (the containing voxel, or the trilinear distance and
weight in layer_ref._interp's order), then the classes and the integer sums of the rule.  Every intermediate is float32 and every
sum an integer, so a record compares bit for bit.  Shares no code with the kernels.

A layer is (idx int32[n,3], vox uint32[n,4096,3]) as Layer.download() returns it; classes and error words come back per block of
A in the order A was given."""
import numpy as np

import layer_ref as LR
import map_ref
from layer_ref import F, K_EPS, VPS, Grid, _centre, _f, _interp, _key, _rotate

HIST_BINS = 22
Q_SATURATED = 1 << 20
IGNORE = {"all": 0, "behind_test": 1, "behind_gt": 2, "behind_all": 3}
SAMPLE = {"nearest": 0, "trilinear": 1}
COUNTS = ("n_a_observed", "n_overlap", "n_ignored", "n_evaluated", "sum_q", "sum_q2_lo", "sum_q2_hi", "n_near_a", "n_near_b", "n_a_surface_in_b_free",
          "n_b_surface_in_a_free", "n_agree")
STATS_DTYPE = np.dtype([(n, np.uint64) for n in COUNTS] + [("hist", np.uint64, (HIST_BINS,)), ("min_q", np.uint32), ("max_q", np.uint32)])
UNOBSERVED, NO_COUNTERPART, IGNORED, EVALUATED, A_IN_B_FREE, B_IN_A_FREE = 0, 1, 2, 3, 4, 8


def _finder(idx):
    """block indices (three int64 arrays) -> row of the block in idx, -1 when it is missing"""
    keys = _key(np.asarray(idx, np.int64).reshape(-1, 3))
    o = np.argsort(keys)
    keys = keys[o]

    def find(b):
        if len(keys) == 0:
            return np.full(len(b[0]), -1, np.int64)
        k = _key(np.stack(b, axis=-1))
        j = np.clip(np.searchsorted(keys, k), 0, len(keys) - 1)
        return np.where(keys[j] == k, o[j], -1)
    return find


def sample_ref(idx, vox, voxel, pos, trilinear):
    """B at the points pos (three float32 arrays) -> (ok bool[n], distance float32[n], weight float32[n]).  ok: the point is finite
    and inside the packed keys and the sample succeeded (nearest: the containing voxel exists and has weight > 0; trilinear: the block
    of the point and all eight voxels of the cell exist with weight > 0)."""
    g = Grid(voxel)
    n = len(pos[0])
    idx, vox = np.asarray(idx, np.int32).reshape(-1, 3), np.asarray(vox, np.uint32).reshape(-1, VPS ** 3, 3)
    zero = np.zeros(n, F)
    if len(idx) == 0:
        return np.zeros(n, bool), zero, zero.copy()
    find = _finder(idx)
    lim = F(1048575.0)
    with np.errstate(all="ignore"):
        inside = np.ones(n, bool)
        for p in pos:
            s = p * g.bs_inv
            inside &= (s > -lim) & (s < lim)           # False for a NaN
        pos = [np.where(inside, p, F(0)) for p in pos]
        b0 = [np.floor(p * g.bs_inv + K_EPS).astype(np.int64) for p in pos]
        row0 = find(b0)
        exists = inside & (row0 >= 0)
        v0, b, vi = [], [], []
        for k in range(3):
            origin = b0[k].astype(F) * g.bs
            v = np.clip(np.floor((pos[k] - origin) * g.vs_inv + K_EPS).astype(np.int64), 0, VPS - 1)
            v0.append(v)
            low = (pos[k] - (origin + _centre(v, g.vs))) < F(0)
            v = v - low
            wrap = v < 0
            b.append(b0[k] - wrap)
            vi.append(v + VPS * wrap)
        if not trilinear:
            words = vox[np.maximum(row0, 0), v0[0] + VPS * (v0[1] + VPS * v0[2])]
            d, w = _f(words[:, 0]), _f(words[:, 1])
            ok = exists & (w > 0)
            return ok, np.where(ok, d, F(0)), np.where(ok, w, F(0))
        ok = exists.copy()
        d, w = [], []
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
        off = [(pos[k] - (b[k].astype(F) * g.bs + _centre(vi[k], g.vs))) * g.vs_inv for k in range(3)]
        dx, dy, dz = off
        q = [np.ones(n, F), dx, dy, dz, dx * dy, dy * dz, dz * dx, dx * dy * dz]
        dd, ww = _interp(q, d), _interp(q, w)
    return ok, np.where(ok, dd, F(0)), np.where(ok, ww, F(0))


def config_ref(voxel_a, s=0.0, f=0.0, a=0.0, min_weight=1e-6):
    """cox_compare_create's resolution of the defaults: a distance of 0 stands for s = voxel size of A, f = 2 s, a = s"""
    s = F(voxel_a) if F(s) == 0 else F(s)
    f = F(F(2) * s) if F(f) == 0 else F(f)
    a = s if F(a) == 0 else F(a)
    return s, f, a, F(min_weight)


def quantise(e):
    """q of float32 errors e: |e| < 16 ? floor(|e| * 65536) : 2^20 (a NaN takes the second branch)"""
    with np.errstate(invalid="ignore"):
        ae = np.abs(np.asarray(e, F))
        small = ae < F(16)
        return np.where(small, np.floor(np.where(small, ae, F(0)) * F(65536.0)), Q_SATURATED).astype(np.int64)


def record(cls, dA, dB, e, s, f, a):
    """the record of per-voxel classes (without the conflict bits), distances and errors: a 0-d array of STATS_DTYPE"""
    rec = np.zeros((), STATS_DTYPE)
    ov = cls >= IGNORED
    ev = cls == EVALUATED
    rec["n_a_observed"] = int((cls != UNOBSERVED).sum())
    rec["n_overlap"] = int(ov.sum())
    rec["n_ignored"] = int((cls == IGNORED).sum())
    rec["n_evaluated"] = int(ev.sum())
    q = quantise(e[ev])
    q2 = q * q
    rec["sum_q"] = int(q.sum())
    rec["sum_q2_lo"] = int((q2 & ((1 << 20) - 1)).sum())
    rec["sum_q2_hi"] = int((q2 >> 20).sum())
    with np.errstate(invalid="ignore"):
        near_a, near_b = ov & (np.abs(dA) <= s), ov & (np.abs(dB) <= s)
        afb, bfa = near_a & (dB >= f), near_b & (dA >= f)
        rec["n_agree"] = int((ov & (np.abs(e) <= a)).sum())
    rec["n_near_a"], rec["n_near_b"] = int(near_a.sum()), int(near_b.sum())
    rec["n_a_surface_in_b_free"], rec["n_b_surface_in_a_free"] = int(afb.sum()), int(bfa.sum())
    bins = np.array([int(v).bit_length() for v in q], np.int64)      # 0 for q = 0, k for 2^(k-1) <= q < 2^k
    rec["hist"] = np.bincount(bins, minlength=HIST_BINS).astype(np.uint64)
    if len(q):
        rec["min_q"], rec["max_q"] = int(q.min()), int(q.max())
    return rec, afb, bfa


def observe(A, voxel_a, B, voxel_b, T=None, sample="nearest", min_weight=1e-6):
    """steps 1 to 4 of the rule, flat over A's voxels: (observed in A bool, overlapping bool, dA, dB, e = dA - dB float32)"""
    idx_a, vox_a = np.asarray(A[0], np.int32).reshape(-1, 3), np.asarray(A[1], np.uint32).reshape(-1, VPS ** 3, 3)
    dA, wA = _f(vox_a[..., 0]).reshape(-1), _f(vox_a[..., 1]).reshape(-1)
    with np.errstate(all="ignore"):
        obs_a = wA > F(min_weight)
        c = map_ref.voxel_centres(idx_a, voxel_a).reshape(-1, 3)
        pos = tuple(np.ascontiguousarray(c[:, k]) for k in range(3))
        if T is not None:
            q, t = LR._pose(T)
            r = _rotate(q, pos)
            pos = tuple((r[k] + t[k]).astype(F) for k in range(3))
        ok, dB, wB = sample_ref(B[0], B[1], voxel_b, pos, SAMPLE[sample] == 1)
        ov = obs_a & ok & (wB > F(min_weight))
        e = (dA - dB).astype(F)
    return obs_a, ov, dA, dB, e


def compare_ref(A, voxel_a, B, voxel_b, T=None, ignore="all", sample="nearest", s=0.0, f=0.0, a=0.0, min_weight=1e-6):
    """-> (record: 0-d array of STATS_DTYPE, classes uint32 [n,4096] with the conflict bits, error words float32 [n,4096]: e where
    the voxel is evaluated, else 0).  ignore may be a sequence of modes: then a dict mode -> that triple, from one sampling of B."""
    s, f, a, min_weight = config_ref(voxel_a, s, f, a, min_weight)
    obs_a, ov, dA, dB, e = observe(A, voxel_a, B, voxel_b, T, sample, min_weight)
    n = len(np.asarray(A[0]).reshape(-1, 3))
    out = {}
    for mode in ((ignore,) if isinstance(ignore, str) else tuple(ignore)):
        with np.errstate(invalid="ignore"):
            ign = ov & {0: np.zeros(len(dA), bool), 1: dA < 0, 2: dB < 0, 3: (dA < 0) & (dB < 0)}[IGNORE[mode]]
        cls = np.where(obs_a, NO_COUNTERPART, UNOBSERVED).astype(np.uint32)
        cls[ov] = EVALUATED
        cls[ign] = IGNORED
        rec, afb, bfa = record(cls, dA, dB, e, s, f, a)
        cls = cls | (afb * np.uint32(A_IN_B_FREE)).astype(np.uint32) | (bfa * np.uint32(B_IN_A_FREE)).astype(np.uint32)
        err = np.where((cls & 3) == EVALUATED, e, F(0)).astype(F)
        out[mode] = (rec, cls.reshape(n, -1), err.reshape(n, -1))
    return out[ignore] if isinstance(ignore, str) else out


def rmse(rec):
    """sqrt((hi * 2^20 + lo) / n_evaluated) / 65536 in Python integers and float64"""
    total = (int(rec["sum_q2_hi"]) << 20) + int(rec["sum_q2_lo"])
    return float(np.sqrt(np.float64(total) / np.float64(int(rec["n_evaluated"]))) / 65536.0)


def conflict_ratio(rec):
    den = int(rec["n_near_a"]) + int(rec["n_near_b"])
    return (int(rec["n_a_surface_in_b_free"]) + int(rec["n_b_surface_in_a_free"])) / den if den else float("nan")


def error_layer_words(cls, err):
    """the wire words of the error layer: e | 1.0f where evaluated | class"""
    words = np.zeros(cls.shape + (3,), np.uint32)
    words[..., 0] = np.ascontiguousarray(err, F).view(np.uint32)
    words[..., 1] = np.where((cls & 3) == EVALUATED, F(1.0).view(np.uint32), 0)
    words[..., 2] = cls
    return words
