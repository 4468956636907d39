"""Seeded generator of TSDF layers and finishSubmap() configurations for the submap fuzz (tests/test_submap_ref_cpu.py,
tests/test_gpu_submap_fuzz.py).  case(seed) draws a family, a block set, an observation mask, a way of building the layer and
the ESDF / isosurface parameters; build_layer() makes the layer on an engine.  What the references are fed is always the
layer's own download(), so a construction that rewrites voxels (merge_from) cannot bias the comparison."""
import numpy as np

from coxgraph_amd.capi import Layer

FIELDS = ("analytic", "noise", "fused")
BLOCK_SETS = ("full", "subset70", "edges_only", "corners_only", "two_components", "single", "slab")
MASKS = ("all", "blobs", "salt", "min_weight", "zeros")
BUILDS = ("plain", "shuffled", "grow", "merge")
BOX = (3, 4, 4)   # blocks in x, y, z
LIN = np.arange(4096)
LOC = np.stack([LIN % 16, (LIN // 16) % 16, LIN // 256], axis=1)


def block_set(kind, rng, lo):
    full = np.array([[x, y, z] for z in range(BOX[2]) for y in range(BOX[1]) for x in range(BOX[0])], np.int64)
    if kind == "full":
        keep = full
    elif kind == "subset70":
        keep = full[rng.random(len(full)) < 0.7]
    elif kind == "edges_only":      # no face neighbours: the wavefront crosses through edge and corner halos only
        keep = full[full.sum(axis=1) % 2 == 0]
    elif kind == "corners_only":    # neighbours at (+-1, +-1, +-1) only
        keep = full[(full[:, 0] % 2 == full[:, 1] % 2) & (full[:, 1] % 2 == full[:, 2] % 2)]
    elif kind == "two_components":
        keep = full[full[:, 0] != 1]
    elif kind == "single":
        keep = full[:1] + np.array([1, 1, 1])
    else:                           # slab, one block thick
        keep = full[full[:, 2] == 1]
    if len(keep) == 0:
        keep = full[:1]
    return (keep + np.asarray(lo)).astype(np.int32)


def analytic_prims(rng, lo, voxel, need_plane=False):
    """1-3 disjoint solids inside the box: at most one half space and spheres clear of it and of each other"""
    bs = 16 * voxel
    a, b = np.asarray(lo) * bs, (np.asarray(lo) + BOX) * bs
    mid, ext = 0.5 * (a + b), b - a
    prims = []
    k = int(rng.integers(1, 4))
    if rng.random() < 0.7 or need_plane:
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        off = float(n @ (mid + rng.uniform(-0.15, 0.15, 3) * ext))
        prims.append(("plane", n, off))
    tries = 0
    while len(prims) < k and tries < 200:
        tries += 1
        r = float(rng.uniform(5, 14)) * voxel
        c = a + rng.uniform(0.15, 0.85, 3) * ext
        ok = True
        for kind, p, q in prims:
            gap = (c @ p - q) - r if kind == "plane" else np.linalg.norm(c - p) - q - r
            ok &= gap > 4 * voxel
        if ok:
            prims.append(("sphere", c, r))
    return prims


def field_values(kind, rng, centres, voxel, prims):
    if kind == "analytic":
        from submap_ref import analytic_sdf
        return analytic_sdf(prims, centres)[0]
    # smooth noise: a few low-frequency waves, a few voxels of amplitude
    d = np.zeros(centres.shape[:-1])
    for _ in range(4):
        kvec = rng.normal(size=3) * (2 * np.pi / (rng.uniform(12, 40) * voxel))
        d += rng.uniform(1.0, 3.0) * voxel * np.sin(centres @ kvec + rng.uniform(0, 2 * np.pi))
    return d


def case(seed, family=None, propagating=False):
    """-> (voxel_size, idx, vox, esdf cfg, iso cfg, meta).  idx / vox are None for the fused family (build_layer integrates
    frames).  family = (field, block set, mask, build) pins those four draws; the rest still comes from the seed.
    propagating pins the band to one that must propagate (fixed band 1.5 voxels, maximum 2 or 4 m, default = maximum)."""
    rng = np.random.default_rng(1000003 * seed + 17)
    field = FIELDS[int(rng.choice(3, p=[0.45, 0.4, 0.15]))]
    blocks, mask, build = (str(rng.choice(x)) for x in (BLOCK_SETS, MASKS, BUILDS))
    if family is not None:
        field, blocks, mask, build = family
    voxel = float(rng.choice([0.05, 0.1, 0.2]))
    trunc = 3 * voxel
    max_d = float(rng.choice([0.5, 2.0, 4.0]))
    min_kind = str(rng.choice(["1.5vox", "0.1", "0.2", "ge_trunc", "gt_max"], p=[0.35, 0.2, 0.2, 0.125, 0.125]))
    min_d = {"1.5vox": 1.5 * voxel, "0.1": 0.1, "0.2": 0.2, "ge_trunc": 4 * voxel, "gt_max": 1.2 * max_d}[min_kind]
    default_d = max_d * float(rng.choice([1.0, 0.5, 2.0]))
    esdf_min_w = float(rng.choice([1e-6, 1.0]))
    if propagating:
        max_d = max(max_d, 2.0)
        min_kind, min_d, default_d = "1.5vox", 1.5 * voxel, max_d
    esdf_cfg = dict(max_distance_m=max_d, min_distance_m=min_d, default_distance_m=default_d, min_weight=esdf_min_w)
    iso_cfg = dict(min_weight=float(rng.choice([1.0, 1e-4])), vertex_proximity_threshold=float(rng.choice([0.5 * voxel, 1e-3])))
    lo = rng.integers(-3, 2, 3)     # negative and positive block indices
    meta = dict(seed=seed, field=field, blocks=blocks, mask=mask, build=build, min_kind=min_kind, prims=None, voxel=voxel,
                capacity=4 if build == "grow" else 0)
    # a fixed band exists and the wavefront has room: the band is thinner than the truncation, and a default below the
    # band could only leave voxels where they start
    meta["propagates"] = min_d < trunc and min_d >= voxel and default_d > 2 * trunc and blocks not in ("single",)
    # a depth camera never observes more than the truncation band behind a surface: few negative voxels to propagate to
    meta["negative_share"] = field != "fused"
    meta["has_surface"] = blocks in ("full", "subset70", "two_components", "slab") and mask in ("all", "zeros")
    if field == "fused":
        voxel = float(rng.choice([0.05, 0.1]))   # a room of a few metres: coarser voxels leave too little surface
        iso_cfg["vertex_proximity_threshold"] = float(rng.choice([0.5 * voxel, 1e-3]))
        trunc = 3 * voxel
        meta.update(blocks="fused", mask="sensor", voxel=voxel, frames=[int(t) for t in rng.choice(200, 8, replace=False)], subsample=4)
        meta["has_surface"] = True
        meta["propagates"] = min_d < trunc and min_d >= voxel and default_d > 2 * trunc
        return voxel, None, None, esdf_cfg, iso_cfg, meta
    idx = block_set(blocks, rng, lo)
    centres = ((idx[:, None, :].astype(np.int64) * 16 + LOC[None]).astype(np.float64) + 0.5) * float(np.float32(voxel))
    if field == "analytic":
        meta["prims"] = analytic_prims(rng, lo, voxel)
        # a half space takes a large part of the box; spheres alone are a few per cent of its volume
        meta["negative_share"] = meta["prims"][0][0] == "plane"
    d = np.clip(field_values(field, rng, centres, voxel, meta["prims"]), -trunc, trunc).astype(np.float32)
    w = rng.choice(np.array([0.5, 1.0, 1.0000001, 5.0, 40.0], np.float32), size=d.shape, p=[0.02, 0.03, 0.02, 0.63, 0.3]).astype(np.float32)
    if mask == "blobs":
        for _ in range(int(rng.integers(3, 9))):
            c = centres[rng.integers(len(idx)), rng.integers(4096)]
            w[np.linalg.norm(centres - c, axis=-1) < rng.uniform(2, 7) * voxel] = 0.0
    elif mask == "salt":
        w[rng.random(d.shape) < 0.02] = 0.0
    elif mask == "min_weight":      # exactly the ESDF's and the isosurface's thresholds, and one ulp below
        r = rng.random(d.shape)
        w[r < 0.03] = np.float32(esdf_min_w)
        w[(r >= 0.03) & (r < 0.05)] = np.nextafter(np.float32(esdf_min_w), np.float32(0))
        w[(r >= 0.05) & (r < 0.08)] = np.float32(iso_cfg["min_weight"])
    elif mask == "zeros":           # exact zeros of both signs in the distance: a fixed source of the negative side
        r = rng.random(d.shape)
        d[r < 0.01] = 0.0
        d[(r >= 0.01) & (r < 0.02)] = -0.0
    vox = np.zeros(d.shape + (3,), np.uint32)
    vox[..., 0], vox[..., 1] = d.view(np.uint32), w.view(np.uint32)
    vox[..., 2] = rng.integers(0, 2 ** 32, d.shape, dtype=np.uint64).astype(np.uint32)   # colours: must not leak into the ESDF
    return voxel, idx, vox, esdf_cfg, iso_cfg, meta


def build_layer(eng, c):
    """The layer of a case on an engine, built the way meta['build'] says."""
    voxel, idx, vox, _, _, meta = c
    if idx is None:
        from util import run_frames
        return run_frames(eng, "merged", voxel, meta["frames"], subsample=meta["subsample"], capacity_blocks=2048)[0]
    rng = np.random.default_rng(meta["seed"] + 99)
    layer = Layer(eng, voxel, capacity_blocks=meta["capacity"])
    if meta["build"] == "plain":
        layer.upload(idx, vox)
    elif meta["build"] in ("shuffled", "grow"):
        p = rng.permutation(len(idx))
        for part in np.array_split(p, 3):   # several uploads: the pool fills in shuffled order (and grows from 4 blocks)
            if len(part):
                layer.upload(idx[part], vox[part])
    else:                                   # merge_from: half uploaded, the other half merged in from a second layer
        p = rng.permutation(len(idx))
        a, b = p[: len(p) // 2], p[len(p) // 2:]
        if len(b):
            layer.upload(idx[b], vox[b])
        if len(a):
            other = Layer(eng, voxel)
            other.upload(idx[a], vox[a])
            layer.merge_from(other)
    return layer


def reading_case(a, seed):
    """The reading submap of a fuzzed pair: a layer that case `a`'s isosurface points fall into, so that the registration
    residuals are not vacuous.  Same voxel size and block set as `a`, another field (smooth noise of `seed`), weights all
    positive, the band configuration of case(seed); for a fused `a` the same room seen from the neighbouring frames."""
    voxel, idx, _, _, _, meta = a
    esdf_cfg = case(seed)[3]
    rng = np.random.default_rng(7919 * seed + 3)
    m = dict(seed=seed, field="noise", blocks=meta["blocks"], mask="all", build="plain", prims=None, voxel=voxel, capacity=0)
    if idx is None:
        m.update(field="fused", frames=[(t + 5) % 200 for t in meta["frames"]], subsample=meta["subsample"])
        return voxel, None, None, esdf_cfg, None, m
    centres = ((idx[:, None, :].astype(np.int64) * 16 + LOC[None]).astype(np.float64) + 0.5) * float(np.float32(voxel))
    d = np.clip(field_values("noise", rng, centres, voxel, None), -3 * voxel, 3 * voxel).astype(np.float32)
    w = rng.choice(np.array([0.5, 1.0, 5.0, 40.0], np.float32), size=d.shape, p=[0.02, 0.05, 0.63, 0.3]).astype(np.float32)
    vox = np.zeros(d.shape + (3,), np.uint32)
    vox[..., 0], vox[..., 1] = d.view(np.uint32), w.view(np.uint32)
    return voxel, idx, vox, esdf_cfg, None, m


# every family member once (the other draws come from the seed)
FAMILY_CASES = [(100 + i, ("analytic" if i % 2 else "noise", b, MASKS[i % len(MASKS)], BUILDS[i % len(BUILDS)])) for i, b in enumerate(BLOCK_SETS)] + \
               [(120 + i, ("noise" if i % 2 else "analytic", "full" if i % 2 else "subset70", m, BUILDS[(i + 1) % len(BUILDS)])) for i, m in enumerate(MASKS)] + \
               [(140 + i, ("analytic", "full", "all", b)) for i, b in enumerate(BUILDS)] + [(150, ("fused", "fused", "sensor", "plain"))]
# the families whose wavefront crosses blocks through edge / corner halo entries only, pinned to a band that propagates
DIAGONAL_HALO_CASES = [(160, ("noise", "edges_only", "all", "shuffled")), (161, ("noise", "corners_only", "all", "plain"))]
