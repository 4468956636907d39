"""Hand-made clouds for the ray walk inside the bundle merge (tests/test_gpu_walk_in_merge.py): bundles of chosen sizes whose rays
have chosen step counts.  Everything is designed on the host with the ray caster's own float32 arithmetic and then asserted on the
CPU oracle's frame statistics (bundle count, largest bundle, record count), so a case is what it claims before any kernel runs."""
import numpy as np

VOXEL = 0.1
# 10 cm voxels, a short truncation band and a small minimum range: rays of one step (sensor and surface in one voxel) up to the
# longest the configuration allows (a diagonal ray of max_ray_length_m); the small axis cap holds (101 planes per axis at most)
CFG = dict(default_truncation_distance=0.02, min_ray_length_m=0.01, max_ray_length_m=10.0, use_const_weight=1, allow_clear=1,
           voxel_carving_enabled=1, max_weight=10000.0, use_weight_dropoff=1)
ORIGIN = np.array([0.052, 0.047, 0.055], np.float32)  # the sensor, unrotated, near the centre of voxel (0, 0, 0)
POSE = np.array([1, 0, 0, 0, *ORIGIN], np.float32)
JITTER = 0.005  # points of a bundle lie within this of their voxel's centre
F = np.float32


def ray_steps(point_g, origin=ORIGIN, cfg=CFG, voxel=VOXEL):
    """Step count of the carving ray to a (non-clearing) bundle mean, in the float32 operations of dda_setup / the oracle's RayCaster."""
    p, o = np.asarray(point_g, F), np.asarray(origin, F)
    dv = p - o
    n = np.sqrt(F(dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2], dtype=F)
    unit = (dv / n).astype(F)
    end = (p + unit * F(cfg["default_truncation_distance"])).astype(F)
    inv = F(1.0) / F(voxel)
    s, e = (o * inv).astype(F), (end * inv).astype(F)
    return int(np.abs(np.floor(e).astype(np.int64) - np.floor(s).astype(np.int64)).sum()) + 1


def centre_with_steps(target, rng, taken):
    """Centre of a voxel such that every point within JITTER (and a margin) of it gives a ray of exactly `target` steps."""
    corners = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * (JITTER + 0.002)
    for _ in range(400):
        u = rng.uniform(0.25, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
        u /= np.linalg.norm(u)
        for r in np.arange(0.08, 9.9, 0.0173):
            idx = np.floor((ORIGIN + r * u) / VOXEL).astype(np.int64)
            c = (idx + 0.5) * VOXEL
            if tuple(idx) in taken or np.linalg.norm(c - ORIGIN) > 9.9:
                continue
            if all(ray_steps(c + d) == target for d in corners):
                taken.add(tuple(idx))
                return c
    raise AssertionError(f"no voxel found for {target} steps")


def longest_steps():
    """The longest ray of CFG: towards a corner of the cube, just inside max_ray_length_m."""
    u = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    best = 0
    for r in np.arange(9.6, 9.93, 0.01):
        idx = np.floor((ORIGIN + r * u) / VOXEL).astype(np.int64)
        best = max(best, ray_steps((idx + 0.5) * VOXEL))
    return best


def bundle_cloud(bundles, seed):
    """bundles: [(size, steps)] -> (points in the sensor frame, colours, centres).  steps == 1: the sensor's own voxel.  The points of
    the bundles are interleaved (round robin), so every bundle is met early and the bundles' order is the list's."""
    rng = np.random.default_rng(seed)
    taken = {(0, 0, 0)}
    centres = []
    for _, steps in bundles:
        if steps == 1:  # in the sensor's own voxel: beyond min_ray from it, the ray's end still inside
            corners = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * JITTER
            c = ORIGIN.astype(np.float64) + np.array([0.013, -0.012, 0.012])
            assert all(ray_steps(c + d) == 1 and np.linalg.norm(c + d - ORIGIN) > 0.012 for d in corners)
            centres.append(c)
        else:
            centres.append(centre_with_steps(steps, rng, taken))
    rows = []
    for k in range(max(n for n, _ in bundles)):
        for j, (n, _) in enumerate(bundles):
            if k < n:
                rows.append(centres[j] + rng.uniform(-JITTER, JITTER, 3))
    pts = (np.array(rows) - ORIGIN.astype(np.float64)).astype(np.float32)
    rgba = rng.integers(0, 256, (len(pts), 4), dtype=np.uint8)
    return np.ascontiguousarray(pts), rgba, np.array(centres)
