"""The binding of cox_selftest_stereo_filters (include/coxgraph_hip_selftest.h) and the disparity images the filter tests feed it:
shapes around the labelling tile and images that make a label travel (tests/test_gpu_stereo_filter.py)."""
import ctypes as C

import numpy as np

import stereo_filter_ref as fr
from coxgraph_amd import capi

X = fr.INVALID
TW, TH = 32, 8   # the labelling tile of coxgraph_amd/csrc/cox_stereo_filter.hpp (kTileW, kTileH)
FILL32 = 0xA5A5A5A5   # what the entry pre-fills its label output with
# (w, h)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (TW - 1, 3), (TW, TH), (TW + 1, TH + 1), (2 * TW + 1, 2 * TH + 1), (101, 37), (188, 120)]
ODD_SHAPES = [(TW - 1, 3), (TW + 1, TH + 1), (2 * TW + 1, 2 * TH + 1), (101, 37)]


def selftest(hip, d, median_size=0, speckle_window=0, speckle_range16=16, reserved=0):
    """-> status, dict(median, labels, filtered, counts, guards)"""
    d = np.ascontiguousarray(d, np.uint16)
    h, w = d.shape
    cfg = capi.StereoFilterConfig(median_size, speckle_window, speckle_range16, reserved)
    med, lab, out = np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint16)
    counts, guards = np.full(4, 99, np.uint64), np.full(3, 99, np.uint32)
    status = hip.lib.cox_selftest_stereo_filters(C.c_int(0), capi._fp(d), C.c_int(w), C.c_int(h), C.byref(cfg), capi._fp(med), capi._fp(lab), capi._fp(out),
                                                 capi._fp(counts), capi._fp(guards))
    return status, dict(median=med, labels=lab, filtered=out, counts=dict(zip(fr.COUNTS, (int(c) for c in counts))), guards=guards.tolist())


# ---- images ------------------------------------------------------------------------------------------------------------------------
def all_invalid(w, h):
    return np.full((h, w), X, np.uint16)


def constant(w, h, value=321):
    return np.full((h, w), value, np.uint16)


def checkerboard(w, h, a=100, b=117):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, a, b).astype(np.uint16)


def staircase(w, h, step, down=False):
    """every column (row when `down`) one step above the one before: crosses every tile border"""
    y, x = np.mgrid[0:h, 0:w]
    return (100 + step * (y if down else x)).astype(np.uint16)


def serpentine(w, h, down=False):
    """a path one pixel wide along every other row (column when `down`), joined at alternating ends; its values wander within a
    range of 16.  It starts at pixel 0, the least index, which is therefore the last pixel seen from its other end."""
    if down:
        return serpentine(h, w).T.copy()
    d = all_invalid(w, h)
    y, x = np.mgrid[0:h, 0:w]
    d[0::2] = (200 + 7 * ((x + y) % 3))[0::2]
    for yy in range(1, h - 1, 2):
        d[yy, w - 1 if (yy // 2) % 2 == 0 else 0] = 205
    return d


def spiral(w, h):
    """a wall one pixel wide winding inward from pixel 0, one pixel of nothing between its turns"""
    d = all_invalid(w, h)
    seen = np.zeros((h + 4, w + 4), bool)   # with a margin of two, so that looking ahead needs no bounds
    x, y, k = 0, 0, 0
    dirs = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    d[0, 0], seen[2, 2] = 300, True
    turns = 0
    while turns < 2:
        dx, dy = dirs[k]
        nx, ny = x + dx, y + dy
        free = 0 <= nx < w and 0 <= ny < h and not seen[ny + 2, nx + 2] and not seen[ny + dy + 2, nx + dx + 2]
        if free:
            x, y, turns = nx, ny, 0
            d[y, x], seen[y + 2, x + 2] = 300 + (x + y) % 5, True
        else:
            k, turns = (k + 1) % 4, turns + 1
    return d


def combs(w, h):
    """teeth on every other column that meet only in the last row"""
    d = all_invalid(w, h)
    d[:, 0::2] = 400
    d[h - 1, :] = 405
    return d


def seeded(w, h, seed, valid_share=0.6):
    """five levels 10/16 px apart: neighbours one level apart link at a range of 16, two levels apart do not"""
    rng = np.random.default_rng(seed)
    d = (200 + 10 * rng.integers(0, 5, (h, w))).astype(np.uint16)
    d[rng.random((h, w)) >= valid_share] = X
    return d


def blobs(w, h, seed):
    """seeded(), smoothed into larger patches: mid-sized components with ragged borders"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 5, ((h + 3) // 4, (w + 3) // 4))
    d = (200 + 10 * np.kron(coarse, np.ones((4, 4), np.int64))[:h, :w]).astype(np.uint16)
    flip = rng.random((h, w)) < 0.15
    d[flip] = (200 + 10 * rng.integers(0, 5, (h, w)))[flip].astype(np.uint16)
    d[rng.random((h, w)) >= 0.8] = X
    return d
