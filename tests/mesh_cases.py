"""Seeded TSDF layers for the mesher fuzz (tests/test_mesh_cpu.py, tests/test_gpu_mesh_fuzz.py), numpy only.  case(seed) draws
a voxel size, a validity threshold, a block set of tests/submap_cases.py (at most 24 blocks), a way of building the layer, where
the box lies (near the origin, a few thousand blocks out, or pinned: half a million blocks out, or where a block face rounds
into the block below it) and a field family.  The families
are chosen for what fused or analytic layers never hold: cubes that emit triangles everywhere, single unobserved voxels, weights
on the validity threshold, +-0.0 distances, neighbouring distances of opposite sign closer than mc_interpolate_vertex's 1e-6,
and missing +x / +y / +z neighbour blocks."""
import numpy as np

import submap_cases
from layer_cases import words
from submap_cases import BLOCK_SETS, BUILDS, LOC, block_set, field_values

VOXELS = (0.05, 0.08, 0.125, 0.2)   # not all powers of two apart: 0.05, 0.1, 0.2 round alike
MIN_WEIGHTS = (1.0, 1e-4)
FIELDS = ("noise", "analytic", "salt", "threshold", "zeros", "tiny", "holes")
LOS = ("near", "far", "extreme", "face")
FACE_LO = (3010, 3035, 3060)
MAX_BLOCKS = 24
TINY = np.array([1e-7, 3e-7, 4.9e-7], np.float32)
F = np.float32


def origin(kind, rng):
    """block index of the box's lower corner"""
    if kind == "near":
        return rng.integers(-3, 2, 3)
    if kind == "far":               # what +-3000 m poses reach at 3-5 cm voxels; the signs are mixed
        sign = np.array([[1, -1, 1], [-1, 1, 1], [1, 1, -1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1]])[rng.integers(6)]
        return sign * rng.integers(3000, 6501, 3)
    if kind == "face":              # pinned: at voxel size 0.08 the +x, +y and +z faces of this block are floats f with
        return np.array(FACE_LO)    # floor(f / block_size + eps) still this block, and voxel index 16 within it
    return np.array([500000, -500000, 100])     # pinned: inside the +-2^20 key range, coordinates with 3 cm between floats


def threshold_values():
    """both validity thresholds, one ulp above and one ulp below each"""
    out = []
    for m in MIN_WEIGHTS:
        m = F(m)
        out += [m, np.nextafter(m, F(2) * m), np.nextafter(m, F(0))]
    return np.array(out, F)


def exact_diff_pairs():
    """(sdf1, sdf2) with sdf1 - sdf2, in float32, exactly 1e-6f, the float above it and the float below it"""
    a = F(2.0 ** -21)
    t = F(1e-6)
    out = []
    for target in (t, np.nextafter(t, F(1)), np.nextafter(t, F(0))):
        b = F(a - target)
        assert F(a - b) == target and b < 0 < a
        out.append((a, b))
    return out


def case(seed, family=None, pow2_weights=False):
    """-> (voxel_size, idx, vox, min_weight, meta).  family = (field, block set, lo, build) pins those four draws; a None among
    them, like everything else, comes from the seed.  meta carries what submap_cases.build_layer reads.  pow2_weights: every
    non-zero weight a power of two, so that merging a block into an empty one ((d w + 0) / w) gives back d and the four builds
    hold the same observed voxels."""
    rng = np.random.default_rng(2000003 * seed + 29)
    field, blocks, build = (str(rng.choice(x)) for x in (FIELDS, BLOCK_SETS, BUILDS))
    lo_kind = LOS[int(rng.choice(2, p=[0.6, 0.4]))]     # the extreme and face families are pinned, never drawn
    if family is not None:
        field, blocks, lo_kind, build = (p if p is not None else d for p, d in zip(family, (field, blocks, lo_kind, build)))
    voxel = float(rng.choice(VOXELS))
    min_weight = float(rng.choice(MIN_WEIGHTS))
    lo = origin(lo_kind, rng)
    idx = block_set(blocks, rng, lo)[:MAX_BLOCKS]
    meta = dict(seed=seed, field=field, blocks=blocks, lo=lo_kind, build=build, voxel=voxel, min_weight=min_weight, prims=None,
                capacity=4 if build == "grow" else 0)
    if field == "holes":            # the +x, +y or +z neighbour of some blocks taken away
        have = {tuple(b) for b in idx.tolist()}
        for b in idx[rng.random(len(idx)) < 0.25].tolist():
            nb = list(b)
            nb[int(rng.integers(3))] += 1
            if tuple(nb) in have and len(have) > 1 and tuple(nb) != tuple(idx[0]):
                have.discard(tuple(nb))
        idx = idx[[tuple(b) in have for b in idx.tolist()]]
    centres = ((idx[:, None, :].astype(np.int64) * 16 + LOC[None]).astype(np.float64) + 0.5) * float(F(voxel))
    if field == "analytic":
        meta["prims"] = submap_cases.analytic_prims(rng, lo, voxel, need_plane=True)
    trunc = 3 * voxel
    d = np.clip(field_values("analytic" if field == "analytic" else "noise", rng, centres, voxel, meta["prims"]), -trunc, trunc).astype(F)
    w = rng.choice(np.array([1.0000001, 5.0, 40.0], F), size=d.shape, p=[0.05, 0.65, 0.3]).astype(F)
    if pow2_weights:
        w = np.where(w > 1.5, F(4.0), F(2.0)).astype(F)
    if field == "salt":
        w[rng.random(d.shape) < 0.02] = 0.0
    elif field == "threshold":
        r = rng.random(d.shape)
        for i, v in enumerate(threshold_values()):
            w[(r >= 0.01 * i) & (r < 0.01 * (i + 1))] = v
    elif field == "zeros":
        r = rng.random(d.shape)
        d[r < 0.01] = 0.0
        d[(r >= 0.01) & (r < 0.02)] = -0.0
    elif field == "tiny":
        d = d.reshape(len(idx), 16, 16, 16)     # [block, z, y, x]
        for axis in (3, 2, 1):                  # x, y, z neighbours inside a block
            shape = list(d.shape)
            shape[axis] -= 1
            hit = rng.random(shape) < 0.01      # 1 % per axis: 3 % of the pairs
            a, b = rng.choice(TINY, shape), rng.choice(TINY, shape)
            flip = rng.random(shape) < 0.5
            first, second = np.where(flip, -b, a).astype(F), np.where(flip, a, -b).astype(F)
            lo_s = [slice(None)] * 4
            hi_s = [slice(None)] * 4
            lo_s[axis], hi_s[axis] = slice(0, -1), slice(1, None)
            d[tuple(lo_s)] = np.where(hit, first, d[tuple(lo_s)])
            d[tuple(hi_s)] = np.where(hit, second, d[tuple(hi_s)])
        at = {tuple(b): i for i, b in enumerate(idx.tolist())}
        for i, b in enumerate(idx.tolist()):    # and across a block face: the midpoint lies on the face itself, where the block
            for axis in range(3):               # found by coordinates and the voxel clamped into it decide the colour
                nb = list(b)
                nb[axis] += 1
                j = at.get(tuple(nb))
                if j is None:
                    continue
                hit = rng.random((16, 16)) < 0.1
                a, bb = rng.choice(TINY, (16, 16)), rng.choice(TINY, (16, 16))
                flip = rng.random((16, 16)) < 0.5
                last, first = [slice(None)] * 3, [slice(None)] * 3
                last[2 - axis], first[2 - axis] = 15, 0
                d[i][tuple(last)] = np.where(hit, np.where(flip, -bb, a), d[i][tuple(last)])
                d[j][tuple(first)] = np.where(hit, np.where(flip, a, -bb), d[j][tuple(first)])
        pairs = exact_diff_pairs()
        for k in range(12):                     # the comparison's own edge: |diff| == 1e-6f and its two neighbours
            b, z, y, x = int(rng.integers(len(idx))), *(int(v) for v in rng.integers(1, 14, 3))
            p = pairs[k % 3]
            if (k // 3) % 2:
                p = (p[1], p[0])
            d[b, z, y, x], d[b, z, y, x + 1] = p
        d = d.reshape(len(idx), 4096)
    colour = rng.integers(0, 2 ** 32, d.shape, dtype=np.uint64).astype(np.uint32)
    return voxel, idx, words(d, w, colour), min_weight, meta


def build_layer(eng, c):
    """the layer of a case on an engine, built the way meta['build'] says (submap_cases.build_layer)"""
    voxel, idx, vox, _, meta = c
    return submap_cases.build_layer(eng, (voxel, idx, vox, None, None, meta))


# one case per field, per origin family and per build, whatever the seed sweep draws
FAMILY_CASES = [(200 + i, (f, ("full", "subset70", "slab", "two_components")[i % 4], "near" if i % 2 else "far", BUILDS[i % 4])) for i, f in enumerate(FIELDS)] + \
               [(220 + i, ("noise", b, "near", "plain")) for i, b in enumerate(BLOCK_SETS)] + \
               [(240 + i, ("noise", "full", lo, "plain")) for i, lo in enumerate(("near", "far"))] + \
               [(250 + i, ("salt", "subset70", "near", b)) for i, b in enumerate(BUILDS)]
FAMILY_CASES.append((270, ("tiny", "full", "far", "plain")))
FAR_CASE = (241, ("noise", "full", "far", "plain"))
TINY_CASE = next(c for c in FAMILY_CASES if c[1][0] == "tiny")
FAR_TINY_CASE = FAMILY_CASES[-1]
THRESHOLD_CASE = next(c for c in FAMILY_CASES if c[1][0] == "threshold")
EXTREME_CASE = (260, ("noise", "full", "extreme", "plain"))
FACE_CASE = (281, ("tiny", "full", "face", "plain"))     # seed 281 draws voxel size 0.08
