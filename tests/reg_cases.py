"""Seeded cases of the registration cost shared by tests/test_reg_ref_cpu.py and tests/test_gpu_registration_edges.py:
reading layers (wire arrays), reference point sets [n,5], pose pairs, sample indices and no_correspondence_cost.

Everything is small: the layers have at most 27 blocks (the one from submap_cases.py has its 3 x 4 x 4 box), the point sets at
most 2 000 points.  The point placements are generated from the reading layer's geometry, with the `has` they must give, so
that the share of every class is known and not hoped for.  Weights are float32 multiples of 2^-10 below 2^10 unless a case
says otherwise: any summation order of their sum is then exact in double and scaled outputs compare bit for bit.
"""
import functools
import math

import numpy as np

import submap_cases

F = np.float32
VS = F(0.1)
CUBE_LO, CUBE_N = np.array([-2, -1, -1]), 3
CUBE_MISSING = (0, 1, 1)                                   # the cube's top corner block is left out
CUBE_ZEROS = (((-1, 0, 0), (5, 6, 7)), ((-2, 0, -1), (9, 3, 11)), ((0, -1, 1), (2, 13, 8)))   # (block, voxel) of weight 0
# wave, workgroup and four-chain partial-sum edges (4 * 256 and 4 * 256 + 1 are 1024 and 1025), the last count without striding, the first with
SAMPLE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 7 * 256, 262144, 262145, 2 * 262144 + 300)
N_SET = 300                                                # points of the set the samples are drawn into
MIN_PER_CLASS = 16


# ---- layers -----------------------------------------------------------------------------------------------------------------------
def _noise_layer(rng, idx, voxel):
    """smooth noise within +-3 voxels, positive weights: wire words [n,4096,3]"""
    centres = ((idx[:, None, :].astype(np.int64) * 16 + submap_cases.LOC[None]).astype(np.float64) + 0.5) * float(F(voxel))
    d = np.clip(submap_cases.field_values("noise", rng, centres, voxel, None), -3 * voxel, 3 * voxel).astype(F)
    w = rng.choice(np.array([0.5, 1.0, 5.0, 40.0], F), size=d.shape).astype(F)
    vox = np.zeros(d.shape + (3,), np.uint32)
    vox[..., 0], vox[..., 1] = d.view(np.uint32), w.view(np.uint32)
    return vox


@functools.lru_cache(maxsize=None)
def layer(name):
    """-> (voxel_size, idx int32[n,3], vox uint32[n,4096,3])"""
    if name == "cube":       # 26 blocks at 0.1 m, negative and positive indices, three voxels of weight 0
        rng = np.random.default_rng(501)
        idx = np.array([(x, y, z) for z in range(CUBE_N) for y in range(CUBE_N) for x in range(CUBE_N)], np.int64) + CUBE_LO
        idx = idx[~(idx == np.array(CUBE_MISSING)).all(1)].astype(np.int32)
        vox = _noise_layer(rng, idx, 0.1)
        for b, v in CUBE_ZEROS:
            vox[np.nonzero((idx == np.array(b)).all(1))[0][0], v[0] + 16 * (v[1] + 16 * v[2]), 1] = 0
        return 0.1, idx, vox
    if name == "fine":       # 2 x 2 x 2 blocks at 0.05 m around the origin
        rng = np.random.default_rng(502)
        idx = np.array([(x, y, z) for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)], np.int32)
        return 0.05, idx, _noise_layer(rng, idx, 0.05)
    if name in ("submap_mask", "submap_reading"):   # a masked layer of the submap fuzz (weight-0 salt, negative indices) and its reading twin
        seed = next(s for s in range(200) if submap_cases.case(s, ("noise", "subset70", "salt", "plain"))[0] in (0.05, 0.1))
        c = submap_cases.case(seed, ("noise", "subset70", "salt", "plain"))
        if name == "submap_reading":
            c = submap_cases.reading_case(c, seed + 1)
        return c[0], c[1], c[2]
    raise KeyError(name)


# ---- geometry of the cube layer -----------------------------------------------------------------------------------------------------
def centre(g, voxel=VS):
    """float32 centre of the global voxels g [...,3], computed as the kernels do: float(b) * block_size + (float(v) + 0.5) * voxel_size"""
    g = np.asarray(g, np.int64)
    vs = F(voxel)
    bs = F(vs * F(16))
    return (((g >> 4).astype(F) * bs).astype(F) + (((g & 15).astype(F) + F(0.5)) * vs).astype(F)).astype(F)


class _Cube:
    def __init__(self):
        _, idx, vox = layer("cube")
        self.weight = {tuple(int(v) for v in b): vox[i, :, 1].view(F) for i, b in enumerate(idx)}

    def present(self, b):
        return tuple(int(v) for v in b) in self.weight

    def voxel_ok(self, g):
        w = self.weight.get(tuple(int(v) >> 4 for v in g))
        return w is not None and w[(int(g[0]) & 15) + 16 * ((int(g[1]) & 15) + 16 * (int(g[2]) & 15))] > 0

    def cell(self, g0):
        """the cell whose lower corner is voxel g0: (its blocks, the missing ones among them, corners of weight <= 0 in present blocks)"""
        corners = [np.asarray(g0) + np.array([(i >> 2) & 1, (i >> 1) & 1, i & 1]) for i in range(8)]
        blocks = {tuple(int(v) >> 4 for v in c) for c in corners}
        missing = {b for b in blocks if not self.present(b)}
        bad = [c for c in corners if self.present(c >> 4) and not self.voxel_ok(c)]
        return blocks, missing, bad


def _placements(rng):
    """-> (pos float32[n,3] in the reading layer's frame, {class: (index array, expected has)})"""
    cube = _Cube()
    lo, hi = CUBE_LO * 16, (CUBE_LO + CUBE_N) * 16
    pos, classes = [], {}

    def draw(cond, k=MIN_PER_CLASS, prep=lambda g: g):
        out = []
        for _ in range(200000):
            g = prep(rng.integers(lo - 1, hi + 1, 3))
            if cond(g):
                out.append(g)
                if len(out) == k:
                    return np.array(out)
        raise AssertionError("placement class could not be filled")

    def add(name, p, has):
        classes[name] = (np.arange(len(p)) + sum(len(x) for x in pos), has)
        pos.append(np.asarray(p, F))

    def whole(g0):
        blocks, missing, bad = cube.cell(g0)
        return not missing and not bad

    def inside(g0, f):
        """a point of the cell above g0 at the fractions f of a voxel (none of them 0.5: the voxel of the point is certain)"""
        return (centre(g0) + (f * VS).astype(F)).astype(F)

    def fractions(k):
        return np.where(rng.random((k, 3)) < 0.5, rng.uniform(0.1, 0.4, (k, 3)), rng.uniform(0.6, 0.9, (k, 3))).astype(F)

    def n15(g0):
        return int(((np.asarray(g0) & 15) == 15).sum())

    def low_face_x(g):   # voxel 0 of its block along x for every second draw: the b--, v += 16 carry
        g = g.copy()
        if rng.random() < 0.5:
            g[0] &= ~15
        return g

    # on a voxel centre, and one float32 ulp to either side of it in all three coordinates
    g = draw(whole)
    add("centre", centre(g), True)
    g = draw(lambda g: whole(g - 1), prep=low_face_x)
    assert ((g[:, 0] & 15) == 0).sum() >= 4
    add("ulp_below", np.nextafter(centre(g), F(-np.inf)), True)
    g = draw(whole)
    add("ulp_above", np.nextafter(centre(g), F(np.inf)), True)
    # on a block's low x face: the voxel below it along x is the lower corner
    g = draw(lambda g: whole(g) and (g[0] & 15) == 15, prep=lambda g: np.array([g[0] | 15, g[1], g[2]]))
    p = inside(g, fractions(len(g)))
    p[:, 0] = ((g[:, 0] + 1) >> 4).astype(F) * F(VS * F(16))
    add("block_face", p, True)
    # cells of 2, 4 and 8 blocks, whole and with exactly one block missing that is not the point's own
    for nb, k15 in ((2, 1), (4, 2), (8, 3)):
        g = draw(lambda g: whole(g) and n15(g) == k15, prep=lambda g: np.where(rng.random(3) < 0.6, g | 15, g))
        add(f"blocks{nb}", inside(g, fractions(len(g))), True)
        got_g, got_f = [], []
        while len(got_g) < MIN_PER_CLASS:
            g1 = draw(lambda g: n15(g) == k15 and len(cube.cell(g)[1]) == 1 and not cube.cell(g)[2], k=1, prep=lambda g: np.where(rng.random(3) < 0.6, g | 15, g))[0]
            f = fractions(1)[0]
            if cube.present((g1 + (f > 0.5)) >> 4):
                got_g.append(g1)
                got_f.append(f)
        add(f"blocks{nb}_missing", inside(np.array(got_g), np.array(got_f)), False)
    # exactly one corner of weight 0
    g = np.array([np.array(b) * 16 + np.array(v) - np.array([(i >> 2) & 1, (i >> 1) & 1, i & 1]) for b, v in CUBE_ZEROS for i in range(8)])
    assert all(not cube.cell(x)[1] and len(cube.cell(x)[2]) == 1 for x in g)
    add("zero_corner", inside(g, fractions(len(g))), False)
    # the point's own block is the one that is missing: the other blocks of its cell exist.  (A cell always holds a voxel of
    # the block of its point, so "all eight corners exist elsewhere" cannot happen)
    m16 = np.array(CUBE_MISSING) * 16
    g = np.array([m16 + np.where(rng.random(3) < 0.6, -1, rng.integers(0, 15, 3)) for _ in range(MIN_PER_CLASS)])
    assert all(cube.cell(x)[1] == {CUBE_MISSING} for x in g)
    add("own_block_missing", inside(g, rng.uniform(0.6, 0.9, (len(g), 3)).astype(F)), False)
    # all block indices negative
    g = draw(lambda g: whole(g) and max(max(b) for b in cube.cell(g)[0]) < 0)
    add("negative_blocks", inside(g, fractions(len(g))), True)
    # NaN and +-inf coordinates
    p = inside(draw(whole, k=18), fractions(18))
    for i, bad in enumerate((np.nan, np.inf, -np.inf) * 6):
        p[i, i % 3] = bad
        if i >= 9:
            p[i, (i + 1) % 3] = bad
    add("non_finite", p, False)
    return np.concatenate(pos), classes


def generic_positions(rng, idx, voxel, n, margin=0.25):
    """n positions in the bounding box of the blocks idx, widened by margin (so that a share falls outside)"""
    bs = 16 * float(F(voxel))
    lo, hi = idx.min(0) * bs - margin, (idx.max(0) + 1) * bs + margin
    return rng.uniform(lo, hi, (n, 3)).astype(F)


def dyadic_weights(rng, n):
    return (rng.integers(1, 1 << 20, n).astype(np.float64) / 1024.0).astype(F)


def points_at(q, pose_ref, pose_read, d, w):
    """The reference point set [n,5] whose points land (up to float32 rounding) on the positions q of the reading frame under
    the pose pair: p = Rz(yaw_f)^T (Rz(yaw_r) q + t_r - t_f)"""
    q = np.asarray(q, np.float64)
    cf, sf, cr, sr = math.cos(pose_ref[3]), math.sin(pose_ref[3]), math.cos(pose_read[3]), math.sin(pose_read[3])
    Rf = np.array([[cf, -sf, 0], [sf, cf, 0], [0, 0, 1.0]])
    Rr = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1.0]])
    p = (q @ Rr.T + (np.asarray(pose_read[:3], np.float64) - np.asarray(pose_ref[:3], np.float64))) @ Rf
    return np.concatenate([p.astype(F), np.asarray(d, F)[:, None], np.asarray(w, F)[:, None]], 1)


# ---- poses ------------------------------------------------------------------------------------------------------------------------
PI = math.pi
BS = float(F(VS * F(16)))
# (name, reference pose, reading pose, finite and in reach: the points are mapped onto their positions through it)
POSES = (
    ("identity", (0, 0, 0, 0), (0, 0, 0, 0), True),
    ("yaw_p90", (0.1, -0.2, 0.05, PI / 2), (0, 0, 0, 0), True),
    ("yaw_m90", (0, 0, 0, 0), (0.1, 0.2, -0.05, -PI / 2), True),
    ("yaw_p180", (0, 0, 0, PI), (0.05, 0, 0, 0), True),
    ("yaw_m180", (0, 0.1, 0, 0.3), (0, 0, 0, -PI), True),
    ("yaw_3pi", (0, 0, 0, 3 * PI), (0.02, 0.01, 0, 0.1), True),
    ("yaw_m7", (0.3, 0, 0, -7.0), (0, 0.2, 0.1, 0.4), True),
    ("far_3000", (3000.0, -3000.0, 3000.0, 0.4), (3000.03, -2999.98, 3000.01, 0.38), True),
    ("one_block", (0, 0, 0, 0), (BS, 0, 0, 0), True),
    # no point can have a correspondence: J = 0 and r = w * no_correspondence_cost * scale
    ("outside", (0, 0, 0, 0.2), (100.0, 0, 0, 0), False),
    ("beyond_keys", (0, 0, 0, 0), (0, 3.0e6, 0, 0), False),
    ("nan_yaw", (0, 0, 0, math.nan), (0, 0, 0, 0), False),
    ("nan_y", (0, 0, 0, 0), (0, math.nan, 0, 0.1), False),
    ("inf_x", (0, 0, 0, 0), (math.inf, 0, 0, 0), False),
    ("ninf_z", (0, 0, -math.inf, 0.3), (0, 0, 0, 0), False),
)
FINITE_POSES = tuple(p for p in POSES if p[3] or p[0] in ("outside", "beyond_keys"))
SMALL_POSE = ((0.02, -0.01, 0.0, 0.01), (0.05, -0.03, 0.02, math.radians(1.0)))


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _case(name, layer_name, pts, pose, samples=None, ncc=0.25, dyadic=True, degenerate=None, classes=None):
    return dict(name=name, layer=layer_name, pts=np.ascontiguousarray(pts, F), pose_ref=np.array(pose[0], np.float64), pose_read=np.array(pose[1], np.float64),
                samples=samples, ncc=ncc, dyadic=dyadic, degenerate=degenerate, classes=classes or {})


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of dict(name, layer, pts[n,5], pose_ref, pose_read, samples (uint32 or None), ncc, dyadic, degenerate (None, "no_correspondence" or
    "zero_weights"), classes)"""
    out = []
    _, cube_idx, _ = layer("cube")
    # every placement class at the identity pose (the transform is exact there), among generic points
    rng = np.random.default_rng(601)
    pos, classes = _placements(rng)
    pos = np.concatenate([pos, generic_positions(rng, cube_idx, 0.1, 150)])
    n = len(pos)
    pts = np.concatenate([pos, rng.uniform(-0.3, 0.3, n).astype(F)[:, None], dyadic_weights(rng, n)[:, None]], 1)
    out.append(_case("placements", "cube", pts, ((0, 0, 0, 0), (0, 0, 0, 0)), classes=classes))
    # the poses, on generic points of the cube
    for i, (name, pf, pr, mapped) in enumerate(POSES):
        rng = np.random.default_rng(610 + i)
        q = generic_positions(rng, cube_idx, 0.1, N_SET)
        d, w = rng.uniform(-0.3, 0.3, N_SET), dyadic_weights(rng, N_SET)
        pts = points_at(q, pf, pr, d, w) if mapped else np.concatenate([q, d.astype(F)[:, None], w[:, None]], 1)
        out.append(_case("pose_" + name, "cube", pts, (pf, pr), ncc=0.25 if i % 2 else 0.0, degenerate=None if mapped else "no_correspondence"))
    # weights
    rng = np.random.default_rng(640)
    q = generic_positions(rng, cube_idx, 0.1, N_SET)
    d = rng.uniform(-0.3, 0.3, N_SET)
    out.append(_case("w_arbitrary", "cube", points_at(q, *SMALL_POSE, d, rng.uniform(0.01, 50.0, N_SET)), SMALL_POSE, dyadic=False))
    w = dyadic_weights(rng, N_SET)
    w[rng.random(N_SET) < 0.25] = 0
    out.append(_case("w_some_zero", "cube", points_at(q, *SMALL_POSE, d, w), SMALL_POSE, ncc=0.0))
    out.append(_case("w_all_zero", "cube", points_at(q, *SMALL_POSE, d, np.zeros(N_SET)), SMALL_POSE, degenerate="zero_weights"))
    # sample counts: wave, workgroup, partial-sum and striding edges, drawn with repeats into one 300-point set
    base = points_at(q, *SMALL_POSE, d, dyadic_weights(rng, N_SET))
    for cnt in SAMPLE_COUNTS:
        out.append(_case(f"samples_{cnt}", "cube", base, SMALL_POSE, samples=np.random.default_rng(900 + cnt % 9973).integers(0, N_SET, cnt).astype(np.uint32)))
    # 0.05 m voxels; a masked submap-fuzz layer and its reading twin
    for i, (lname, npts) in enumerate((("fine", 300), ("submap_mask", 2000), ("submap_reading", 1000))):
        rng = np.random.default_rng(660 + i)
        voxel, idx, _ = layer(lname)
        q = generic_positions(rng, idx, voxel, npts, margin=2.5 * voxel)
        pts = points_at(q, *SMALL_POSE, rng.uniform(-3 * voxel, 3 * voxel, npts), dyadic_weights(rng, npts))
        out.append(_case(lname, lname, pts, SMALL_POSE, ncc=0.0 if i == 1 else 0.25))
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)
