"""Seeded differential fuzzing of the projective integrator: HIP engine against the CPU oracle, bit for bit.  Random voxel
sizes, interpolation schemes, sensor models (not powers of two), full random rotations, translations from zero to kilometres,
clouds of awkward sizes with NaN / inf / zero points, points at the poles, on the azimuth seam, outside the field of view and
the ray limits, shuffled so that neighbouring lanes are not neighbouring pixels, de-integrations in the middle, host and device
entry points, pools that have to double several times.

    python tests/test_gpu_projective_fuzz.py 200 [first_seed]   # a longer campaign, stops at the first mismatch
"""
import os
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from coxgraph_amd.capi import Layer, Integrator  # noqa: E402
from util import compare_layers  # noqa: E402

KEYS = ("n_points", "n_valid", "n_rays", "n_updates", "n_touched_voxels", "n_touched_blocks", "n_new_blocks")  # as tests/test_gpu_projective.py
SENSORS = [(2, 2), (3, 5), (16, 1024), (64, 1800), (480, 640), (960, 1280)]
SIZES = [0, 1, 63, 64, 65, 255, 257, 5000, 100000]
DENORM = np.float32(1.4e-45)


def scene_cloud(rng, n, reach):
    kind = int(rng.integers(0, 3))
    d = rng.normal(size=(n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    if kind == 0:    # a wall in front
        d[:, 0] = np.abs(d[:, 0]) + 0.2
        p = d * (0.7 * reach / d[:, 0])[:, None]
    elif kind == 1:  # a sphere around the sensor
        p = d * (0.6 * reach * (1.0 + 0.02 * rng.normal(size=(n, 1))))
    else:            # a room: the unit cube's faces
        p = d / np.max(np.abs(d), axis=1, keepdims=True) * 0.5 * reach
    return p.astype(np.float32)


def inject(rng, p, fov_deg, min_ray, max_ray):
    """Overwrite some points with the inputs kernels go wrong on."""
    n = len(p)
    if n == 0:
        return p
    with np.errstate(invalid="ignore", over="ignore"):
        return _inject(rng, p, n, fov_deg, min_ray, max_ray)


def _inject(rng, p, n, fov_deg, min_ray, max_ray):
    k = max(1, n // 50)
    pick = lambda: rng.integers(0, n, k)
    p[pick(), rng.integers(0, 3, k)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), k)
    p[pick()] = 0.0
    p[pick()] *= np.array([0, 0, 1], np.float32)                                   # the poles: x = y = 0
    i = pick()
    p[i, 0], p[i, 1] = -np.abs(p[i, 0]) - 0.1, rng.choice(np.array([0.0, -0.0, DENORM, -DENORM], np.float32), k)  # the azimuth seam
    i = pick()
    r = np.linalg.norm(p[i], axis=1)
    alt = np.radians(min(fov_deg, 179.0) / 2.0) * rng.choice([1.02, -1.02, 0.999, -0.999], k)  # just outside / inside the vertical field of view
    az = rng.uniform(-np.pi, np.pi, k)
    p[i] = (np.nan_to_num(r, nan=1.0, posinf=1.0)[:, None] * np.stack([np.cos(alt) * np.cos(az), np.cos(alt) * np.sin(az), np.sin(alt)], axis=1)).astype(np.float32)
    i = pick()
    p[i] = p[i] / np.maximum(np.linalg.norm(p[i], axis=1, keepdims=True), 1e-6) * np.float32(0.5 * min_ray + 0.01)  # closer than min_ray
    i = pick()
    p[i] = p[i] / np.maximum(np.linalg.norm(p[i], axis=1, keepdims=True), 1e-6) * np.float32(1.5 * max_ray)         # farther than max_ray
    p[pick()] = p[0]                                                                # duplicates
    return p


def make_case(seed):
    """Everything a case is, as a pure function of the seed."""
    rng = np.random.default_rng(seed)
    voxel = float(rng.choice([0.02, 0.05, 0.10, 0.20]))
    rows, cols = SENSORS[int(rng.integers(0, len(SENSORS)))]
    fov = float(rng.choice([20.0, 90.0, 180.0, 360.0]))
    min_ray, max_ray = float(rng.choice([0.0, 0.1, 0.5])), float(rng.uniform(3.0, 20.0))
    on_centre = bool(rng.random() < 0.15)
    if on_centre:
        min_ray = 0.0
    cfg = dict(default_truncation_distance=float(rng.integers(2, 5)) * voxel, projective_interpolation_scheme=int(rng.integers(0, 4)),
               projective_adaptive_gap_m=float(rng.choice([0.05, 0.5])), use_const_weight=int(rng.integers(0, 2)), use_weight_dropoff=int(rng.integers(0, 2)),
               voxel_carving_enabled=int(rng.integers(0, 2)), max_weight=float(rng.choice([10000.0, 3.0])), min_ray_length_m=min_ray, max_ray_length_m=max_ray,
               sensor_horizontal_resolution=cols, sensor_vertical_resolution=rows, sensor_vertical_field_of_view_degrees=fov)
    reach = min(max_ray, 120.0 * voxel)  # bounds the number of blocks (and the oracle's time), not the kinds of input
    scale = float(rng.choice([0.0, 2.0, 3000.0]))
    shuffle = bool(rng.random() < 0.5)
    entry = str(rng.choice(["host", "dev", "mix"]))
    frames = []
    for _ in range(int(rng.integers(1, 6))):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        t = rng.uniform(-1.0, 1.0, 3) * scale
        if on_centre:  # the sensor exactly on a voxel centre, not rotated: dv == 0, a 0 / 0 bearing
            q = np.array([1.0, 0, 0, 0])
            t = ((rng.integers(0, 16, 3).astype(np.float32) + np.float32(0.5)) * np.float32(voxel)).astype(np.float64)
        n = int(rng.choice(SIZES))
        p = scene_cloud(rng, n, reach)
        p = inject(rng, p, fov, min_ray, max_ray)
        if not shuffle and n:  # scan order: neighbouring points are neighbouring pixels
            p = p[np.lexsort((np.arctan2(p[:, 1], p[:, 0]), np.round(np.nan_to_num(p[:, 2], posinf=0.0, neginf=0.0), 1)))]
        frames.append([np.concatenate([q, t]).astype(np.float32), np.ascontiguousarray(p, np.float32), False, "host"])
    deint = len(frames) >= 2 and rng.random() < 0.4
    if deint:  # take an earlier frame out again, in the middle
        k = int(rng.integers(0, len(frames) - 1))
        frames.insert(int(rng.integers(k + 1, len(frames))), [frames[k][0], frames[k][1], True, "host"])
    for f in frames:
        if not f[2]:  # (de-integration has a host entry point only)
            f[3] = {"host": "host", "dev": "dev", "mix": str(rng.choice(["host", "dev"]))}[entry]
    capacity = int(rng.choice([0, 8, 64]))
    what = dict(seed=seed, voxel=voxel, cfg=cfg, frames=[(len(f[1]), f[2], f[3]) for f in frames], capacity=capacity, shuffle=shuffle, on_centre=on_centre,
                translation=scale)
    return dict(voxel=voxel, cfg=cfg, frames=frames, capacity=capacity, what=what, scheme=cfg["projective_interpolation_scheme"], sensor=(rows, cols), deintegrates=deint)


def run_case(seed, hip, oracle):
    import torch
    case = make_case(seed)
    lb = Layer(oracle, case["voxel"])
    ob = Integrator(oracle, lb, oracle.default_config(**case["cfg"]), "projective")
    la = Layer(hip, case["voxel"], capacity_blocks=case["capacity"])
    ia = Integrator(hip, la, hip.default_config(**case["cfg"]), "projective")
    keep = []
    try:
        for k, (T, p, de, entry) in enumerate(case["frames"]):
            if de:
                ob.deintegrate_points(T, p)
                ia.deintegrate_points(T, p)
            else:
                ob.integrate_points(T, p, None)
                if entry == "host":
                    ia.integrate_points(T, p, None)
                else:
                    x = torch.from_numpy(p).cuda() if len(p) else torch.zeros((1, 3), device="cuda")
                    torch.cuda.synchronize()
                    keep.append(x)
                    ia.integrate_points_dev(T, x.data_ptr(), 0, len(p))
            if entry == "host" or k == len(case["frames"]) - 1:  # per frame through the host path, at the end for the device path
                ia.sync()
                sa, sb = ia.last_stats(), ob.last_stats()
                for key in KEYS:
                    assert sa[key] == sb[key], (k, key, sa[key], sb[key])
        rep = compare_layers(la, lb, tol=0.0, check_color=False)
        assert rep["bitexact_d"] and rep["bitexact_w"], rep
    except AssertionError as e:
        raise AssertionError(f"{case['what']}: {e}") from e
    return case, rep


def default_seeds():
    n = int(os.environ.get("COX_FUZZ_SEEDS", "32"))
    return list(range(max(n, 1)))


SEEDS = default_seeds()
_OBSERVED = {}


def test_the_default_seeds_draw_every_scheme_sensor_model_and_a_deintegration():
    cases = [make_case(s) for s in range(32)]
    assert {c["scheme"] for c in cases} == {0, 1, 2, 3}
    assert {c["sensor"] for c in cases} == set(SENSORS)
    assert any(c["deintegrates"] for c in cases) and any(c["capacity"] == 8 for c in cases) and any(c["what"]["on_centre"] for c in cases)
    assert {e for c in cases for _, _, e in c["what"]["frames"]} == {"host", "dev"}
    a, b = make_case(5), make_case(5)
    assert a["what"] == b["what"] and all(np.array_equal(x[1], y[1], equal_nan=True) for x, y in zip(a["frames"], b["frames"]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_projective_cases_match_the_oracle_bit_for_bit(hip, oracle, seed):
    case, rep = run_case(seed, hip, oracle)
    _OBSERVED[seed] = (case["scheme"], case["sensor"], case["deintegrates"], rep["observed"])


@pytest.mark.gpu
def test_the_fuzz_was_not_vacuous():
    """Over the seeds that ran in this process: every scheme, every sensor model and a de-integration that make_case draws for them
    occurred in a case that left observed voxels."""
    drawn = [make_case(s) for s in _OBSERVED]
    live = [v for v in _OBSERVED.values() if v[3] > 0]
    assert {v[0] for v in live} == {c["scheme"] for c in drawn}, sorted(_OBSERVED.items())
    assert {v[1] for v in live} == {c["sensor"] for c in drawn}, sorted(_OBSERVED.items())
    assert any(v[2] for v in live) == any(c["deintegrates"] for c in drawn), sorted(_OBSERVED.items())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["minneighbour-dropoff-pose", "bilinear-invr2-nocarve-two-frames", "integrate-then-deintegrate-invr2"])
def test_hip_against_the_float64_reference_without_the_oracle(hip, name):
    """The check that does not go through the oracle at all: same rule and caps as tests/test_projective_cpu.py (clouds without
    points on decision borders are a condition of that rule, so these are three cases of its matrix, not fuzz seeds)."""
    from test_projective_cpu import CASES, build_case, run_engine, check_against_reference
    case = [c for c in CASES if c[0] == name][0]
    cfg, fov, frames = build_case(case)
    layer, stats = run_engine(hip, cfg, fov, frames)
    check_against_reference(layer, stats, cfg, frames, "hip " + name)


@pytest.mark.gpu
def test_hip_device_path_with_a_small_pool_against_the_float64_reference(hip):
    """The same rule through integrate_points_dev, no sync between the frames, a pool of 8 blocks that has to double several times."""
    import torch
    from test_projective_cpu import CASES, build_case, engine_kwargs, check_against_reference
    case = [c for c in CASES if c[0] == "adaptive-const-two-frames-360"][0]
    cfg, fov, frames = build_case(case)
    layer = Layer(hip, cfg["voxel_size"], capacity_blocks=8)
    integ = Integrator(hip, layer, hip.default_config(**engine_kwargs(cfg, fov)), "projective")
    dev = [torch.from_numpy(p).cuda() for _, p, _ in frames]
    torch.cuda.synchronize()
    stats = []
    for (T, p, _), x in zip(frames, dev):
        integ.integrate_points_dev(T, x.data_ptr(), 0, len(p))
    integ.sync()
    last = integ.last_stats()
    # the counters of the frames before the last are not kept on this path: the reference's own for those
    import proj_ref
    ref_counts = [proj_ref.range_image(p, cfg) for _, p, _ in frames[:-1]]
    stats = [dict(n_valid=r["n_valid"], n_rays=r["n_rays"]) for r in ref_counts] + [last]
    check_against_reference(layer, stats, cfg, frames, "hip device path, pool of 8")
    assert layer.capacity() > 8


if __name__ == "__main__":
    ROOT = os.path.dirname(_HERE)
    import torch
    torch.zeros(1, device="cuda")
    import coxgraph_amd
    from coxgraph_amd.capi import Engine
    hip_e = coxgraph_amd.load_engine()
    ora = Engine(os.path.join(ROOT, "oracle", "libcoxoracle.so"), "coxo_")
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    for s in range(first, first + n):
        c, r = run_case(s, hip_e, ora)
        print("ok", s, c["what"]["voxel"], c["sensor"], c["what"]["frames"], r["observed"], flush=True)
    print("all", n, "cases identical")
