"""Bindings of the two input-side self-test entries (include/coxgraph_hip_selftest.h: cox_selftest_depth_points,
cox_selftest_copy_from_host) and the seeded images, masks and sizes of the front-end tests.  Shared by
tests/test_frontend_ref_cpu.py (no GPU) and tests/test_gpu_frontend.py."""
import ctypes as C

import numpy as np

import frontend_ref as fr

F32 = np.float32
U32 = np.uint32
SENTINEL = 0xDEADBEEF  # as a float: -6.26e18, which no point of the tests has; no seeded colour or copy word equals it
NO_DEVICE = -2

# ---- the depth front end, directly -------------------------------------------------------------------------------------------------
# (w, h): below one 8-pixel strip, around it, a column, around one tile of 2048 in one row and in three, whole tiles, an odd image
# above two tiles, and three tiles + 1
SHAPES = ((1, 1), (7, 1), (8, 1), (9, 1), (1, 9), (2047, 1), (2048, 1), (2049, 1), (683, 3), (64, 32), (67, 71), (6145, 1))
STRIDED_SHAPES = ((6145, 1), (67, 71))  # with grid 1 and 2 the tile loops of both kernels run: 4 and 3 tiles
GRIDS = (0, 1, 2)
PATTERNS = ("all", "none", "first", "last", "tile_edge", "random", "tile_hole")
INVALID = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0], F32)
DENORMAL, HUGE = F32(1e-40), F32(1e30)


def intrinsics(w, h):
    """fx != fy, and cx, cy that are no integers: no pixel has xn == 0 or yn == 0."""
    return np.array([611.16, 609.64, 0.37 * w + 0.45, 0.61 * h + 0.3], F32)


def valid_mask(pattern, n, seed=0):
    """bool [n], or None where the pattern does not exist at this size."""
    m = np.zeros(n, bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[n - 1] = True
    elif pattern == "tile_edge":  # the last pixel of tile 0 and the first of tile 1
        if n <= 2048:
            return None
        m[[2047, 2048]] = True
    elif pattern == "random":
        m = np.random.default_rng([seed, n, 50]).random(n) < 0.5
    elif pattern == "tile_hole":  # one whole tile invalid between two valid ones
        if n <= 3 * 2048:
            return None
        m[:] = True
        m[2048:4096] = False
    else:
        assert pattern == "none"
    return m


def depth_image(w, h, mask, seed=0):
    """f32 [h, w]: ordinary depths with a denormal and a huge one among them where the mask is set; elsewhere the invalid values in
    turn (NaN, +inf, -inf, 0.0, -0.0, -1.0)."""
    n = w * h
    rng = np.random.default_rng([seed, w, h, 1])
    d = rng.uniform(0.3, 5.0, n).astype(F32)
    pos = np.arange(n)
    d[pos % 7 == 3] = DENORMAL
    d[pos % 11 == 5] = HUGE
    bad = np.flatnonzero(~mask)
    d[bad] = INVALID[np.arange(len(bad)) % len(INVALID)]
    return d.reshape(h, w)


def colour_image(w, h, seed=0):
    """u8 [w * h, 4]: seeded words, none of them 0 or the sentinel."""
    words = np.random.default_rng([seed, w, h, 2]).integers(1, 0xDEADBEEF, w * h, dtype=np.uint64).astype(U32)
    return words.view(np.uint8).reshape(-1, 4)


def _p(a, t=C.c_uint32):
    return a.ctypes.data_as(C.POINTER(t))


class DepthResult:
    """xyz as words [w h, 3], rgba as words [w h], tile_sums [tiles], n, guard_touched (xyz, rgba, tile_sums): all as they came back."""


def run_depth_points(hip, depth, rgba, K, grid=0, want_rgba=True, device=0):
    """One cox_selftest_depth_points call on depth f32 [h, w] and rgba u8 [w h, 4] or None."""
    depth = np.ascontiguousarray(depth, F32)
    h, w = depth.shape
    n = w * h
    K = np.ascontiguousarray(K, F32)
    if rgba is not None:
        rgba = np.ascontiguousarray(rgba, np.uint8)
        assert rgba.shape == (n, 4)
    r = DepthResult()
    r.xyz, r.rgba, r.tile_sums = np.zeros((n, 3), U32), np.zeros(n, U32), np.zeros(fr.depth_tiles(n), U32)
    n_out, guard = C.c_uint32(0), np.zeros(3, U32)
    r.status = hip.fn("selftest_depth_points")(C.c_int(device), _p(depth, C.c_float), None if rgba is None else _p(rgba, C.c_uint8), C.c_int(w), C.c_int(h),
                                               _p(K, C.c_float), C.c_uint32(grid), C.c_int(int(want_rgba)), C.c_uint32(SENTINEL), _p(r.xyz, C.c_float),
                                               _p(r.rgba, C.c_uint8), _p(r.tile_sums), C.byref(n_out), _p(guard))
    r.n, r.guard_touched = int(n_out.value), [int(g) for g in guard]
    return r


# ---- the copy kernel, directly -----------------------------------------------------------------------------------------------------
COPY_GROUPS = (1, 8, 13)


def copy_sizes(groups):
    """words_a of the direct tests: below and around one 16-byte load, and around one and four loads per lane of the whole grid
    (S = groups * 256 lanes): n16 = S - 1, S, S + 1 and 4 S - 1, 4 S, 4 S + 1, each with every tail of 0..3 words.  At 4 S - 1 the
    last lane leaves the 4-deep loop for the remainder loop, at 4 S + 1 the first lane goes round again."""
    S = groups * 256
    sizes = [0, 1, 2, 3, 4, 5, 7]
    for centre in (4 * S, 4 * (4 * S)):
        for off in (-4, 0, 4):
            sizes += [centre + off + t for t in range(4)]
    return sizes


def second_sizes(words_a, groups):
    """words_b per words_a: absent (None), shorter than a, longer than a (and on another tail and another trip count)."""
    return (None, words_a // 3, words_a + 4 * groups * 256 + 6)


def seeded_words(n, seed):
    return np.random.default_rng([seed, n, 3]).integers(0, 0xDEADBEEF, n, dtype=np.uint64).astype(U32)


def run_copy(hip, a, b, groups, device=0):
    """(status, out_a, out_b or None, guard_touched[2]) of one cox_selftest_copy_from_host call; b None: no second segment."""
    a = np.ascontiguousarray(a, U32)
    out_a = np.zeros(len(a), U32)
    guard = np.zeros(2, U32)
    if b is None:
        pb, nb, out_b, pob = None, 0, None, None
    else:
        b = np.ascontiguousarray(b, U32)
        out_b = np.zeros(len(b), U32)
        pb, nb, pob = _p(b), len(b), _p(out_b)
    st = hip.fn("selftest_copy_from_host")(C.c_int(device), _p(a), C.c_uint64(len(a)), pb, C.c_uint64(nb), C.c_int(groups), C.c_uint32(SENTINEL),
                                           _p(out_a), pob, _p(guard))
    return st, out_a, out_b, [int(g) for g in guard]


# ---- through the integrator --------------------------------------------------------------------------------------------------------
SCENE_WH = (67, 71)  # 4757 pixels: two tiles and a part
SCENE_K = np.array([70.0, 68.0, 33.3, 35.6], F32)
# valid counts around the bundle grid (64), the mixed order's group count and the head / sort tiles (1024, 2048), and np2
# (4095 | 4096: 4096 | 8192, while the bound's stays 8192)
VALID_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
STREAM_SHAPES = ((64, 32), (67, 71), (9, 1), (683, 3), (64, 32))
ASYNC_COUNTS = (1, 2, 3, 5, 1366, 4757)  # 12 n and 4 n bytes: tails of 1, 2 and 3 words, no whole 16 bytes at all, both loops


def scene_depth(w, h):
    """1.5 + 0.4 sin(u / 9) cos(v / 7): a wavy wall 1.1 .. 1.9 m ahead."""
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return (1.5 + 0.4 * np.sin(u / 9.0) * np.cos(v / 7.0)).astype(F32)


def scene_intrinsics(w, h):
    """SCENE_K for the scene's own size; for the other sizes of the stream a field of view as moderate, so that every ray stays
    inside the integrator's limits."""
    if (w, h) == SCENE_WH:
        return SCENE_K
    f = 1.05 * max(w, h)
    return np.array([f, 0.97 * f, 0.5 * w - 0.2, 0.5 * h + 0.1], F32)


def with_valid_count(depth, V, seed):
    """depth with all but V seeded pixels made invalid (the invalid values in turn)."""
    d = depth.reshape(-1).copy()
    bad = np.sort(np.random.default_rng([seed, d.size, V]).permutation(d.size)[V:])
    d[bad] = INVALID[np.arange(len(bad)) % len(INVALID)]
    return d.reshape(depth.shape)
