"""Steps 7a and 7b of a dense-stereo frame (the 3 x 3 median over the valid values and the speckle filter on the
disparity image) restated in numpy, the structures of include/coxgraph_hip_stereo_filter.h restated in ctypes, and the frame with
the filters in it.  Builds on tests/stereo_ref.py; the GPU owes this file every bit."""
import ctypes as C

import numpy as np

import stereo_ref as sr

INVALID = sr.INVALID
NO_LABEL = 0xFFFFFFFF
DEFAULTS = dict(median_size=0, speckle_window=0, speckle_range16=16, reserved=0)
COUNTS = ("n_median_changed", "n_components", "n_speckle_components", "n_speckle_pixels")
DISPARITY_RAW, DISPARITY_MEDIAN, LABELS = 0, 1, 2


class Config(C.Structure):
    _fields_ = [("median_size", C.c_int32), ("speckle_window", C.c_int32), ("speckle_range16", C.c_int32), ("reserved", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTS] + [(n, C.c_double) for n in ("median_ms", "speckle_ms")]


# ---- step 7a -----------------------------------------------------------------------------------------------------------------------
def median3(d):
    """u16 [h, w] -> u16 [h, w]: a valid pixel off the border takes rank (n - 1) // 2 of the n valid values of its 3 x 3 window"""
    d = np.asarray(d, np.uint16)
    h, w = d.shape
    out = d.copy()
    if h < 3 or w < 3:
        return out
    win = np.stack([d[dy:dy + h - 2, dx:dx + w - 2] for dy in range(3) for dx in range(3)], -1)
    ordered = np.sort(win, -1)                       # 0xFFFF is above every valid value: the invalid ones come last
    n = np.sum(win != INVALID, -1)
    rank = np.maximum(n - 1, 0) // 2
    med = np.take_along_axis(ordered, rank[..., None], -1)[..., 0]
    centre = d[1:-1, 1:-1]
    out[1:-1, 1:-1] = np.where(centre != INVALID, med, centre)
    return out


# ---- step 7b -----------------------------------------------------------------------------------------------------------------------
def _links(d, range16):
    """the pairs (i, j) of linear indices of linked 4-neighbours"""
    h, w = d.shape
    v = d.astype(np.int64)
    ok = d != INVALID
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    across = ok[:, 1:] & ok[:, :-1] & (np.abs(v[:, 1:] - v[:, :-1]) <= range16)
    down = ok[1:] & ok[:-1] & (np.abs(v[1:] - v[:-1]) <= range16)
    return np.concatenate([idx[:, 1:][across], idx[1:][down]]), np.concatenate([idx[:, :-1][across], idx[:-1][down]])


def _components(n, a, b):
    """component number per node of the graph with edges (a[k], b[k])"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:   # a plain union-find
        parent = list(range(n))

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i
        for i, j in zip(a.tolist(), b.tolist()):
            ri, rj = find(i), find(j)
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
        return np.array([find(i) for i in range(n)], np.int64)
    graph = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    return connected_components(graph, directed=False)[1].astype(np.int64)


def labels(d, range16):
    """u16 [h, w] -> u32 [h, w]: the least linear index y * w + x of a pixel's component, 0xFFFFFFFF at invalid pixels"""
    d = np.asarray(d, np.uint16)
    h, w = d.shape
    comp = _components(h * w, *_links(d, range16))
    least = np.full(int(comp.max()) + 1, h * w, np.int64)
    np.minimum.at(least, comp, np.arange(h * w))
    lab = least[comp].reshape(h, w)
    return np.where(d != INVALID, lab, NO_LABEL).astype(np.uint32)


def sizes(lab):
    """pixels of its component, per pixel (0 at invalid pixels)"""
    ok = lab != NO_LABEL
    count = np.bincount(lab[ok].astype(np.int64), minlength=lab.size)
    return np.where(ok, count[np.where(ok, lab, 0).astype(np.int64)], 0)


def speckle(d, window, range16):
    """u16 [h, w] -> u16 [h, w]: every pixel of a component of at most `window` pixels becomes invalid"""
    d = np.asarray(d, np.uint16)
    sz = sizes(labels(d, range16))
    return np.where((d != INVALID) & (sz <= window), INVALID, d).astype(np.uint16)


def run(d, median_size=0, speckle_window=0, speckle_range16=16):
    """7a and 7b as cox_selftest_stereo_filters and a frame run them -> dict(median, labels (None with 7b off), filtered, counts)"""
    d = np.asarray(d, np.uint16)
    med = median3(d) if median_size == 3 else d.copy()
    counts = dict.fromkeys(COUNTS, 0)
    counts["n_median_changed"] = int(np.sum(med != d))
    lab, out = None, med
    if speckle_window > 0:
        lab = labels(med, speckle_range16)
        sz = sizes(lab)
        idx = np.arange(d.size, dtype=np.int64).reshape(d.shape)
        roots = lab == idx
        gone = (med != INVALID) & (sz <= speckle_window)
        out = np.where(gone, INVALID, med).astype(np.uint16)
        counts.update(n_components=int(roots.sum()), n_speckle_components=int((roots & gone).sum()), n_speckle_pixels=int(gone.sum()))
    return dict(median=med, labels=lab, filtered=out, counts=counts)


# ---- the frame ---------------------------------------------------------------------------------------------------------------------
def match_filtered(left, right, K_rect, baseline_m, map0=None, map1=None, median_size=0, speckle_window=0, speckle_range16=16, **cfg):
    """sr.match up to the disparity, 7a, 7b, then step 8 on the filtered image.  -> sr.match's dict with disparity, depth and the two
    depth counts of the filtered frame, and disparity_raw, disparity_median, labels, filter_stats"""
    out = dict(sr.match(left, right, K_rect, baseline_m, map0, map1, **cfg))
    c = dict(sr.DEFAULTS, **cfg)
    f = run(out["disparity"], median_size, speckle_window, speckle_range16)
    d = f["filtered"]
    valid = d != INVALID
    fB16 = np.float32(float(np.float32(K_rect[0])) * float(np.float32(baseline_m)) * 16.0)
    with np.errstate(all="ignore"):
        z = fB16 / np.where(valid, d, 1).astype(np.float32)
    assert z.dtype == np.float32
    outside = valid & ((z < np.float32(c["min_depth_m"])) | (z > np.float32(c["max_depth_m"])))
    stats = dict(out["stats"], n_valid_pixels=int(np.sum(valid & ~outside)), n_rejected_depth=int(np.sum(outside)))
    out.update(disparity_raw=out["disparity"], disparity_median=f["median"], labels=f["labels"], disparity=d,
               depth=np.where(valid & ~outside, z, np.float32(np.nan)).astype(np.float32), stats=stats, filter_stats=f["counts"])
    return out


def outliers(d, truth):
    """valid pixels more than 1 px from the truth"""
    valid = d != INVALID
    return int(np.sum(np.abs(d[valid].astype(np.int64) - 16 * truth[valid]) > 16))
