"""finishSubmap() of the CPU oracle held to the plain numpy references of tests/submap_ref.py (a third opinion that shares
no code with the oracle's queue or the kernel's tiles), over the seeded layers of tests/submap_cases.py.  The check_* helpers
are engine-agnostic: tests/test_gpu_submap_fuzz.py and test_gpu_submap_edges.py run them on the HIP engine.

Bars: ESDF words / flags, box and sampler exact; isosurface as isosurface_ref() states.  Per case the test prints what it
compared (run with -s)."""
import numpy as np
import pytest

import mesh_ref
import submap_cases
import submap_ref
from coxgraph_amd.capi import Layer, RegPoints, Registration
from test_oracle_submap import analytic_layer, VOXEL

SEEDS = list(range(16))
SAMPLER_SEEDS = (0, 1, 12345678901234567)


@pytest.fixture(scope="module")
def ref_mesh(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("meshref_submap"))


def full_cfg(cfg):
    """Layer.esdf() sets default = max when only the maximum is given; the reference's caller does the same"""
    c = dict(max_distance_m=2.0, min_distance_m=0.2, default_distance_m=None, min_weight=1e-6)
    c.update({k: v for k, v in cfg.items() if v is not None})
    if c["default_distance_m"] is None:
        c["default_distance_m"] = c["max_distance_m"] if cfg.get("max_distance_m") is not None else 2.0
    return c


def check_esdf(layer, cfg, name=""):
    """engine's ESDF of `layer` == esdf_ref of its download, bit for bit -> (EsdfRef, engine's ESDF layer)"""
    idx, vox = layer.download()
    e = layer.esdf(**cfg)
    eidx, evox = e.download()
    c = full_cfg(cfg)
    ref = submap_ref.esdf_ref(idx, vox, layer.voxel_size, c["max_distance_m"], c["min_distance_m"], c["default_distance_m"], c["min_weight"])
    assert np.array_equal(eidx, idx)
    want = ref.words()
    bad = evox != want
    moved = ref.observed & ~ref.fixed & (ref.distance.view(np.uint32) != ref.initial.view(np.uint32))
    n_moved, n_neg = int(moved.sum()), int((moved & (ref.distance < 0)).sum())
    print(f"[esdf {name}] voxels {want[..., 0].size}, observed {int(ref.observed.sum())}, fixed {int(ref.fixed.sum())}, propagated {n_moved} "
          f"({n_neg} negative), reference sweeps {ref.sweeps}, mismatching words d/w/flag {int(bad[..., 0].sum())}/{int(bad[..., 1].sum())}/{int(bad[..., 2].sum())}")
    assert not bad.any(), (name, int(bad.sum()))
    return ref, e, n_moved, n_neg


def check_box(layer, name=""):
    idx, vox = layer.download()
    mn, mx, n = layer.surface_obb()
    rmn, rmx, rn = submap_ref.surface_obb_ref(idx, vox, layer.voxel_size)
    print(f"[box {name}] surface voxels {rn}")
    assert n == rn and np.array_equal(mn.view(np.uint32), rmn.view(np.uint32)) and np.array_equal(mx.view(np.uint32), rmx.view(np.uint32)), (name, mn, rmn, mx, rmx, n, rn)
    return rn


def check_sampler(eng, pts, layer, n_res=256, seeds=SAMPLER_SEEDS, name=""):
    """pts: float32 [n,5] -> the draws (last seed)"""
    g = Registration(eng, RegPoints(eng, pts), layer)
    out = None
    for seed in seeds:
        g.draw_samples(n_res, seed)
        out = g.get_samples()
        want = submap_ref.sampler_ref(pts[:, 4], n_res, seed)
        assert np.array_equal(out, want), (name, seed, int((out != want).sum()))
    return out


def _rows(a):
    return np.ascontiguousarray(a, np.float32).view(np.dtype((np.void, 12))).ravel()


def check_iso(eng, layer, ref_mesh, min_weight, threshold, name=""):
    idx, vox = layer.download()
    r = submap_ref.isosurface_ref(ref_mesh, idx, vox, layer.voxel_size, min_weight, threshold)
    P = RegPoints.from_isosurface(eng, layer, min_weight=min_weight, vertex_proximity_threshold=threshold)
    a = P.download()
    assert P.n_mesh_vertices == r.n_mesh_vertices, (name, P.n_mesh_vertices, r.n_mesh_vertices)
    # vertices within one float32 ulp of a boundary of the proximity grid may fall either way: counted, capped at 0.5 %
    assert r.near_boundary <= 0.005 * max(r.n_mesh_vertices, 1), (name, r.near_boundary)
    assert abs(P.n_connected_vertices - r.n_connected) <= r.near_boundary
    if r.near_boundary == 0:
        assert np.array_equal(a[:, :3].view(np.uint32), r.xyz32.view(np.uint32)), name   # same survivors, in mesh order
        ia = ib = np.arange(len(a))
    else:
        _, ia, ib = np.intersect1d(_rows(a[:, :3]), _rows(r.xyz32), return_indices=True)
        assert len(a) + len(r.xyz32) - 2 * len(ia) <= r.near_boundary, (name, len(a), len(r.xyz32), len(ia))
    d, w = submap_ref.fields(vox)
    with np.errstate(invalid="ignore"):
        obs = w > 0
    fd, fw = (float(np.max(np.abs(d[obs]))), float(np.max(w[obs]))) if obs.any() else (0.0, 0.0)
    ed = float(np.max(np.abs(a[ia, 3] - r.points[ib, 3]))) if len(ia) else 0.0
    ew = float(np.max(np.abs(a[ia, 4] - r.points[ib, 4]))) if len(ia) else 0.0
    print(f"[iso {name}] mesh vertices {r.n_mesh_vertices}, connected {r.n_connected}, survivors {len(r.xyz32)}, near a cell boundary {r.near_boundary}; "
          f"worst |d - ref| {ed:.2e} (bound {r.tol_scale * fd:.2e}), worst |w - ref| {ew:.2e} (bound {r.tol_scale * fw:.2e})")
    assert ed <= r.tol_scale * fd and ew <= r.tol_scale * fw, (name, ed, ew)
    return r, a


def true_bounds_apply(c, ref):
    """esdf_true_bounds needs an analytic field, every voxel of every block observed, box-shaped observed space (so that few
    straight ways to the surface leave it) and a band thicker than a voxel diagonal that holds unclamped distances"""
    voxel, _, _, cfg, _, meta = c
    return (meta["field"] == "analytic" and meta["blocks"] in ("full", "two_components", "slab") and bool(ref.observed.all())
            and np.sqrt(3.0) * voxel < cfg["min_distance_m"] <= 3 * voxel)


def run_case(eng, c, ref_mesh, name):
    voxel, _, _, esdf_cfg, iso_cfg, meta = c
    layer = submap_cases.build_layer(eng, c)
    ref, _, n_moved, n_neg = check_esdf(layer, esdf_cfg, name)
    if meta["propagates"]:
        assert n_moved >= 1000, (name, n_moved)
        if meta["negative_share"]:
            assert n_neg >= 0.05 * n_moved, (name, n_neg, n_moved)
    if true_bounds_apply(c, ref):
        idx, _ = layer.download()
        submap_ref.esdf_true_bounds(idx, ref.distance, ref.observed, ref.fixed, ref.initial, meta["prims"], voxel, esdf_cfg["max_distance_m"],
                                    esdf_cfg["min_distance_m"], name)
    check_box(layer, name)
    r, a = check_iso(eng, layer, ref_mesh, iso_cfg["min_weight"], iso_cfg["vertex_proximity_threshold"], name)
    if meta["has_surface"]:
        assert r.n_connected >= 500, (name, r.n_connected)
    if len(a):
        check_sampler(eng, a, layer, name=name)
    return layer


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_matches_references_on_seeded_layers(oracle, ref_mesh, seed):
    run_case(oracle, submap_cases.case(seed), ref_mesh, f"seed {seed}")


@pytest.mark.parametrize("seed,family", submap_cases.FAMILY_CASES, ids=["-".join(f) + f"-{s}" for s, f in submap_cases.FAMILY_CASES])
def test_oracle_matches_references_on_every_family(oracle, ref_mesh, seed, family):
    run_case(oracle, submap_cases.case(seed, family), ref_mesh, "-".join(family))


@pytest.mark.parametrize("seed,family", submap_cases.DIAGONAL_HALO_CASES, ids=[f[1] for _, f in submap_cases.DIAGONAL_HALO_CASES])
def test_oracle_matches_references_where_only_diagonal_halos_connect(oracle, ref_mesh, seed, family):
    """edges_only / corners_only block sets with a band that must propagate: the propagation floor is asserted, not incidental"""
    c = submap_cases.case(seed, family, propagating=True)
    assert c[5]["propagates"] and c[5]["negative_share"]
    run_case(oracle, c, ref_mesh, family[1])


@pytest.mark.parametrize("voxel,max_d,min_d", [(0.05, 0.5, 0.1), (0.05, 2.0, 0.1), (0.1, 2.0, 0.2), (0.1, 4.0, 0.2), (0.05, 2.0, 0.15)])
@pytest.mark.parametrize("seed", [140, 141])
def test_esdf_lies_within_the_chamfer_bounds_of_the_true_distance(oracle, seed, voxel, max_d, min_d):
    """Analytic planes / spheres in a full box, all observed: the bound that rests on no propagation rule."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(-3, 2, 3)
    prims = submap_cases.analytic_prims(rng, lo, voxel, need_plane=True)
    layer = analytic_layer(oracle, lambda p: submap_ref.analytic_sdf(prims, p)[0], lo, lo + np.array(submap_cases.BOX) - 1, voxel=voxel, trunc=3 * voxel)
    cfg = dict(max_distance_m=max_d, min_distance_m=min_d)
    ref, _, n_moved, n_neg = check_esdf(layer, cfg, f"analytic {seed}")
    assert n_moved >= 1000 and n_neg >= 0.05 * n_moved
    idx, _ = layer.download()
    rep = submap_ref.esdf_true_bounds(idx, ref.distance, ref.observed, ref.fixed, ref.initial, prims, voxel, max_d, min_d, f"analytic {seed} {voxel} {max_d} {min_d}")
    assert rep["checked"] >= 1000


def test_existing_plane_and_sphere_anchors_within_the_true_bounds(oracle):
    x0 = 0.237
    for name, prims, lo, hi, max_d in (("plane", [("plane", [1.0, 0.0, 0.0], x0)], (-2, -1, -1), (1, 0, 0), 1.0),
                                      ("sphere", [("sphere", [0.0, 0.0, 0.0], 0.4)], (-2, -2, -2), (1, 1, 1), 1.5)):
        layer = analytic_layer(oracle, lambda p: submap_ref.analytic_sdf(prims, p)[0], lo, hi)
        ref, _, n_moved, _ = check_esdf(layer, dict(max_distance_m=max_d, min_distance_m=0.1), name)
        idx, _ = layer.download()
        rep = submap_ref.esdf_true_bounds(idx, ref.distance, ref.observed, ref.fixed, ref.initial, prims, VOXEL, max_d, 0.1, name)
        assert rep["checked"] >= 1000


def exact_threshold_layer(eng):
    """Two blocks whose voxels sit exactly ON the thresholds: |d| == max_distance in a fixed band wider than the maximum (such a
    source must not propagate: `>=`), and |d| == voxel_size at the layer's outermost voxels (inside the surface box: `<=`)."""
    voxel = 0.2
    idx = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
    d = np.full((2, 16, 16, 16), 0.6, np.float32)      # [block, z, y, x]: +truncation, not fixed
    d[0, 4:12, 4:12, 4:12] = -0.6
    d[:, ::5, ::5, ::5] = np.where(d[:, ::5, ::5, ::5] > 0, np.float32(0.5), np.float32(-0.5))   # lone sources at exactly +-max
    d[0, 0, 0, 0], d[1, 15, 15, 15] = np.float32(voxel), -np.float32(voxel)
    vox = np.zeros((2, 4096, 3), np.uint32)
    vox[..., 0], vox[..., 1] = d.reshape(2, 4096).view(np.uint32), np.float32(2.0).view(np.uint32)
    layer = Layer(eng, voxel, capacity_blocks=64)
    layer.upload(idx, vox)
    return layer, dict(max_distance_m=0.5, min_distance_m=0.55, default_distance_m=1.0)


def check_exact_thresholds(eng):
    layer, cfg = exact_threshold_layer(eng)
    ref, _, n_moved, _ = check_esdf(layer, cfg, "exact thresholds")
    d0 = submap_ref.fields(layer.download()[1])[0]
    assert int((np.abs(d0) == np.float32(0.5)).sum()) > 50 and int(ref.fixed.sum()) > 50
    e = ref.distance.reshape(2, 16, 16, 16)
    assert e[0, 5, 5, 5] == np.float32(-0.5) and e[0, 5, 5, 6] == np.float32(-1.0)      # next to a source at exactly -max: untouched
    assert e[1, 10, 10, 10] == np.float32(0.5) and e[1, 10, 10, 11] == np.float32(1.0)
    assert e[0, 0, 0, 1] == np.float32(0.2) + np.float32(0.2) and n_moved > 0           # the source below the maximum does propagate
    assert check_box(layer, "exact thresholds") == 2
    mn, mx, _ = layer.surface_obb()
    assert np.allclose(mn, 0.0, atol=1e-6) and np.allclose(mx, [6.4, 3.2, 3.2], atol=1e-5)


def unit_weight_points(n=60):
    """weights of exactly one fixed-point unit (2^-20) with zero weights in between: the scaled draw u equals a cumulative
    sum on every draw, where upper bound and lower bound differ, and a zero-weight point must never be drawn"""
    pts = np.zeros((n, 5), np.float32)
    pts[::2, 4] = np.float32(2.0 ** -20)
    return pts


def test_thresholds_hit_exactly(oracle):
    check_exact_thresholds(oracle)


def test_sampler_reference_edges(oracle):
    layer = Layer(oracle, 0.1)
    rng = np.random.default_rng(3)
    pts = np.zeros((300, 5), np.float32)
    pts[:, 4] = rng.choice(np.array([0.0, 1e-7, 9.5367431640625e-07, 0.3, 1.0, 77.25, -1.0, np.nan], np.float32), 300)   # 2^-20, below it, negative, NaN
    draws = check_sampler(oracle, pts, layer, n_res=2000)
    assert np.all(pts[draws, 4] >= np.float32(2.0 ** -20))
    unit = unit_weight_points()
    draws = check_sampler(oracle, unit, layer, n_res=2000)
    assert np.all(draws % 2 == 0) and len(np.unique(draws)) == 30
    one = np.zeros((50, 5), np.float32)
    one[17, 4] = 2.5
    assert np.all(check_sampler(oracle, one, layer, n_res=100) == 17)
    assert np.all(check_sampler(oracle, np.zeros((50, 5), np.float32), layer, n_res=100) == 0)
    assert len(check_sampler(oracle, one, layer, n_res=0)) == 0
