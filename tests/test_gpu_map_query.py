"""GPU map queries (coxgraph_amd/csrc/cox_query.hip) against the test-side reference (tests/cpp/map_reference.cpp, whose
trilinear branch is the CPU checker's getVoxelsAndQVector), against analytic fields, and in the orders the engine promises."""
import os
import subprocess

import numpy as np
import pytest

import map_ref
from coxgraph_amd import synth
from coxgraph_amd.capi import Integrator, Layer
from util import run_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(m, g) for m in ("nearest", "interpolate", "adaptive") for g in (False, True)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return map_ref.build(tmp_path_factory.mktemp("mapref"))


@pytest.fixture(scope="module", params=[0.10, 0.05])
def submap(request, hip):
    """The tests/test_gpu_submap.py submap: frames 0..140 step 10 of the benchmark stream, merged, subsample 2; and its ESDF
    with coxgraph's band (esdf_max_distance 4 m, esdf_min_distance 0.1 m)."""
    voxel = request.param
    layer, _, _ = run_frames(hip, method="merged", voxel=voxel, frames=range(0, 150, 10), subsample=2, capacity_blocks=8192)
    return voxel, layer, layer.esdf(max_distance_m=4.0, min_distance_m=0.1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _query_sets(rng, voxel, idx, vox, n=100_000):
    bs = np.float32(voxel) * np.float32(16)
    lo = idx.min(axis=0).astype(np.float32) * bs - bs
    hi = (idx.max(axis=0).astype(np.float32) + 2) * bs
    uniform = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    w = vox[..., 1].view(np.float32)
    d = vox[..., 0].view(np.float32)
    cen = map_ref.voxel_centres(idx, voxel)
    band_c = cen[(w > 0) & (np.abs(d) < voxel)]
    band = (band_c[rng.integers(0, len(band_c), n)] + rng.normal(0, 0.5 * voxel, size=(n, 3))).astype(np.float32)
    faces = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    ax = rng.integers(0, 3, n)
    k = rng.integers(np.floor(lo / bs).astype(np.int64)[ax], np.ceil(hi / bs).astype(np.int64)[ax])
    f = k.astype(np.float32) * bs
    step = rng.integers(-1, 2, n)  # exactly on the face, or 1 ulp below / above
    f = np.where(step < 0, np.nextafter(f, np.float32(-np.inf)), np.where(step > 0, np.nextafter(f, np.float32(np.inf)), f)).astype(np.float32)
    faces[np.arange(n), ax] = f
    obs_c = cen[w > 0]
    centres = obs_c[rng.integers(0, len(obs_c), n)]
    far = (rng.uniform(-1, 1, size=(n // 10, 3)) * 1000).astype(np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [3e6 * float(bs), 0, 0], [0, -3e6 * float(bs), 0],
                    [1e30, 1e30, 1e30], [2e6 * float(bs), 1, 1]], np.float32)
    return np.concatenate([uniform, band, faces, centres, far, bad])


def _compare(got, exp, gradient):
    assert np.array_equal(got["status"], exp["status"])
    st = got["status"]
    v = (st & 1) != 0
    assert np.array_equal(_bits(got["distance"][v]), _bits(exp["distance"][v]))
    assert np.array_equal(_bits(got["weight"][v]), _bits(exp["weight"][v]))
    assert np.isnan(got["distance"][~v]).all() and np.isnan(got["weight"][~v]).all()
    if gradient:
        gv = (st & 4) != 0
        assert np.array_equal(_bits(got["gradient"][gv]), _bits(exp["gradient"][gv]))
        assert np.isnan(got["gradient"][~gv]).all()


@pytest.mark.parametrize("kind", ["tsdf", "esdf"])
def test_queries_are_bit_identical_to_the_reference(hip, ref, submap, kind):
    voxel, tsdf, esdf = submap
    layer = tsdf if kind == "tsdf" else esdf
    idx, vox = layer.download()
    R = ref.layer(voxel, idx, vox)
    q = _query_sets(np.random.default_rng(11), voxel, idx, vox)
    for mode, grad in COMBOS:
        got = layer.query(q, mode, gradient=grad)
        exp = R.query(q, mode, gradient=grad)
        _compare(got, exp, grad)
        st = got["status"]
        print(f"{kind} {voxel} {mode} grad={grad}: {len(q)} queries, value {np.mean(st & 1 > 0):.3f}, trilinear {np.mean(st & 2 > 0):.3f}, "
              f"gradient {np.mean(st & 4 > 0):.3f}, reference {exp['seconds']:.2f} s")
        assert np.mean(st & 1 > 0) > 0.2
        if grad:
            assert np.mean(st & 4 > 0) > 0.1
        if mode == "adaptive":
            assert (st & 2).any() and ((st & 1 > 0) & (st & 2 == 0)).any()  # both branches answer some queries


# ---- physics anchors -----------------------------------------------------------------------------------------------------
VS, CENTER, RADIUS = 0.05, np.array([0.8 + 0.013, 0.8 - 0.021, 0.8 + 0.007]), 0.35


def _field_layer(hip, vs, field, blocks=2, trunc=None):
    idx = np.array([(x, y, z) for z in range(blocks) for y in range(blocks) for x in range(blocks)], np.int32)
    c = map_ref.voxel_centres(idx, vs).astype(np.float64)
    d = field(c.reshape(-1, 3)).reshape(c.shape[:2])
    if trunc is not None:
        d = np.clip(d, -trunc, trunc)
    words = np.zeros((len(idx), 4096, 3), np.uint32)
    words[..., 0] = d.astype(np.float32).view(np.uint32)
    words[..., 1] = np.float32(1.0).view(np.uint32)
    layer = Layer(hip, vs, capacity_blocks=4 * len(idx))
    layer.upload(idx, words)
    return layer


def test_interpolated_tsdf_matches_an_analytic_sphere(hip):
    layer = _field_layer(hip, VS, lambda c: np.linalg.norm(c - CENTER, axis=1) - RADIUS, trunc=5 * VS)
    rng = np.random.default_rng(2)
    dirs = rng.normal(size=(50_000, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    r = RADIUS + rng.uniform(-2 * VS, 2 * VS, 50_000)
    p = (CENTER + dirs * r[:, None]).astype(np.float32)
    out = layer.query(p, "interpolate", gradient=True)
    ok = out["status"] == 7
    assert ok.mean() > 0.99
    truth = np.linalg.norm(p.astype(np.float64) - CENTER, axis=1) - RADIUS
    err = np.abs(out["distance"][ok] - truth[ok])
    print(f"sphere: max |d - truth| = {err.max():.2e} m, voxel {VS}")
    assert err.max() < 0.25 * VS
    g = out["gradient"][ok].astype(np.float64)
    cos = np.einsum("ij,ij->i", g / np.linalg.norm(g, axis=1)[:, None], dirs[ok])
    assert np.quantile(cos, 0.01) > 0.99


def test_esdf_gradient_of_a_plane_is_its_unit_normal(hip):
    z0 = 0.83
    tsdf = _field_layer(hip, 0.1, lambda c: c[:, 2] - z0, blocks=3, trunc=0.3)
    esdf = tsdf.esdf(max_distance_m=4.0, min_distance_m=0.1)
    rng = np.random.default_rng(4)
    p = rng.uniform([0.3, 0.3, 0.0], [4.5, 4.5, 4.8], size=(50_000, 3)).astype(np.float32)
    for mode in ("interpolate", "adaptive"):
        out = esdf.query(p, mode, gradient=True)
        ok = (out["status"] & 4) != 0
        assert ok.mean() > 0.8
        g = out["gradient"][ok].astype(np.float64)
        n = np.linalg.norm(g, axis=1)
        assert np.max(np.abs(n - 1.0)) < 1e-3, np.max(np.abs(n - 1.0))
        assert np.min(g[:, 2] / n) > 0.9999
        tri = (out["status"] & 2) != 0
        assert tri.mean() > 0.8
        d = out["distance"][tri]
        truth = p[tri, 2].astype(np.float64) - z0
        assert np.max(np.abs(d - truth)) < 1e-4


def test_esdf_distance_in_free_space_is_the_distance_to_the_scene(hip, submap):
    """The ESDF knows the surfaces the stream has seen: its distance in free space is the distance to the nearest of them.  The
    seen surface is the scene's walls and sphere sampled where the TSDF crosses zero (voxel centres within half a voxel of it),
    projected onto the analytic surface they lie on."""
    from scipy.spatial import cKDTree
    voxel, tsdf, esdf = submap
    surf = tsdf.registration_points(1e-4, 0.5 * voxel)[:, :3].astype(np.float64)
    # project every surface voxel onto the nearest analytic surface of the scene (a wall plane or the sphere)
    d_lo, d_hi = surf - synth.ROOM_MIN, synth.ROOM_MAX - surf
    rad = surf - synth.SPHERE_C
    r = np.linalg.norm(rad, axis=1)
    d_sphere = np.abs(r - synth.SPHERE_R)
    proj = surf.copy()
    wall = np.minimum(d_lo, d_hi).min(axis=1) < d_sphere
    ax = np.minimum(d_lo, d_hi).argmin(axis=1)
    lo_side = d_lo[np.arange(len(surf)), ax] < d_hi[np.arange(len(surf)), ax]
    proj[wall, ax[wall]] = np.where(lo_side, synth.ROOM_MIN[ax], synth.ROOM_MAX[ax])[wall]
    proj[~wall] = synth.SPHERE_C + rad[~wall] * (synth.SPHERE_R / r[~wall])[:, None]
    rng = np.random.default_rng(6)
    p = rng.uniform(synth.ROOM_MIN + 0.3, synth.ROOM_MAX - 0.3, size=(200_000, 3)).astype(np.float32)
    out = esdf.query(p, "interpolate")
    truth, _ = cKDTree(proj).query(p.astype(np.float64))
    outside = np.linalg.norm(p.astype(np.float64) - synth.SPHERE_C, axis=1) > synth.SPHERE_R  # free space, not inside the sphere
    sel = ((out["status"] & 1) != 0) & outside & (truth > 2 * voxel) & (truth < 1.0)
    diff = out["distance"][sel] - truth[sel]
    err = np.abs(diff)
    print(f"ESDF {voxel}: {sel.sum()} free-space points, |d - truth| q50 {np.quantile(err, 0.5):.3f} q75 {np.quantile(err, 0.75):.3f} "
          f"q90 {np.quantile(err, 0.9):.3f} max {err.max():.3f} m, d - truth q01 {np.quantile(diff, 0.01):.3f} m")
    # the typical point: within one voxel.  The tail is wider: the wavefront travels through observed
    # voxels alone and its quasi-Euclidean steps lengthen oblique paths
    assert sel.sum() > 1000 and np.quantile(err, 0.5) < voxel
    assert np.quantile(err, 0.9) < 0.25


def test_affine_field_gives_exact_gradients_on_the_gpu(hip, ref):
    idx, words = map_ref.affine_layer_arrays()
    layer = Layer(hip, float(map_ref.AFFINE_VS), capacity_blocks=64)
    layer.upload(idx, words)
    q = map_ref.affine_queries(np.random.default_rng(3))
    exact = q.astype(np.float64) @ map_ref.AFFINE_A.astype(np.float64) + float(map_ref.AFFINE_C)
    R = ref.layer(map_ref.AFFINE_VS, idx, words)
    for mode in ("interpolate", "adaptive", "nearest"):
        out = layer.query(q, mode, gradient=True)
        _compare(out, R.query(q, mode, gradient=True), True)
        assert np.all(out["status"] & 5 == 5)
        assert np.max(np.abs(out["gradient"] - map_ref.AFFINE_A)) < 2e-5
        if mode != "nearest":
            assert np.max(np.abs(out["distance"] - exact)) < 2e-6


# ---- free points -------------------------------------------------------------------------------------------------------
def _numpy_free_points(voxel, idx, vox, min_distance):
    d, w = vox[..., 0].view(np.float32), vox[..., 1].view(np.float32)
    keep = (w > 0) & (d >= np.float32(min_distance))
    return map_ref.voxel_centres(idx, voxel)[keep], d[keep]


def test_free_points_equal_a_numpy_recomputation(hip, ref, submap):
    voxel, _, esdf = submap
    idx, vox = esdf.download()
    top = float(vox[..., 0].view(np.float32).max())
    for md in (0.0, 1.0, np.nextafter(np.float32(top), np.float32(np.inf))):
        xyz, inten = esdf.free_points(md)
        ex, ei = _numpy_free_points(voxel, idx, vox, md)
        assert np.array_equal(_bits(xyz), _bits(ex)) and np.array_equal(_bits(inten), _bits(ei))
        rx, ri = ref.layer(voxel, idx, vox).free_points(md)
        assert np.array_equal(_bits(xyz), _bits(rx)) and np.array_equal(_bits(inten), _bits(ri))
        if md > top:
            assert len(xyz) == 0
        else:
            assert len(xyz) > 100


# ---- device path and ordering ----------------------------------------------------------------------------------------
def test_query_dev_on_a_side_stream_gives_the_same_bits(hip, submap):
    import torch
    voxel, tsdf, _ = submap
    idx, vox = tsdf.download()
    q = _query_sets(np.random.default_rng(12), voxel, idx, vox, n=20_000)
    s = torch.cuda.Stream()
    for mode, grad in COMBOS:
        host = tsdf.query(q, mode, gradient=grad)
        with torch.cuda.stream(s):
            x = torch.from_numpy(q).cuda()
            d = torch.full((len(q),), float("nan"), device="cuda")
            w = torch.full((len(q),), float("nan"), device="cuda")
            g = torch.full((len(q), 3), float("nan"), device="cuda")
            st = torch.zeros(len(q), dtype=torch.uint8, device="cuda")
            tsdf.query_dev(x, mode=mode, gradient=grad, distance=d, weight=w, grad=g if grad else None, status=st, stream=s)
        s.synchronize()
        dev = dict(distance=d.cpu().numpy(), weight=w.cpu().numpy(), status=st.cpu().numpy(), gradient=g.cpu().numpy())
        _compare(dev, host, grad)


def _pinned_frames(ts):
    keep = []
    for t in ts:
        T, pts, rgba, _ = synth.make_frame(t)
        keep.append((T, np.ascontiguousarray(pts[::2]), np.ascontiguousarray(rgba[::2])))
    return keep


def test_a_query_sees_the_frames_enqueued_before_it(hip):
    voxel = 0.05
    cfg = hip.default_config(**synth.integrator_overrides(voxel))
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, cfg, "merged")
    rng = np.random.default_rng(8)
    q = rng.uniform(synth.ROOM_MIN, synth.ROOM_MAX, size=(100_000, 3)).astype(np.float32)
    frames = _pinned_frames(range(0, 60, 10))
    results = []
    for T, pts, rgba in frames:
        integ.integrate_points_async(T, pts.ctypes.data, rgba.ctypes.data, len(pts))
        results.append(layer.query(q, "adaptive", gradient=True))  # no sync in between
    integ.sync()
    after = layer.query(q, "adaptive", gradient=True)
    for k in after:
        assert np.array_equal(np.asarray(results[-1][k]).view(np.uint8), np.asarray(after[k]).view(np.uint8)), k
    # the same frames one at a time, synchronised: every intermediate answer is the one the interleaved query gave
    layer2 = Layer(hip, voxel, capacity_blocks=8192)
    integ2 = Integrator(hip, layer2, cfg, "merged")
    for (T, pts, rgba), got in zip(frames, results):
        integ2.integrate_points(T, pts, rgba)
        integ2.sync()
        exp = layer2.query(q, "adaptive", gradient=True)
        for k in exp:
            assert np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(exp[k]).view(np.uint8)), k
    assert (after["status"] & 1).sum() > 1000


def test_edge_cases(hip, submap):
    voxel, tsdf, esdf = submap
    empty = Layer(hip, voxel, capacity_blocks=64)
    out = empty.query(np.zeros((5, 3), np.float32), "adaptive", gradient=True)
    assert np.all(out["status"] == 0) and np.isnan(out["distance"]).all()
    assert empty.free_points(0.0)[0].shape == (0, 3)
    z = tsdf.query(np.zeros((0, 3), np.float32), "interpolate", gradient=True)
    assert all(len(v) == 0 for v in z.values())
    tsdf.query_dev(None, n=0)
    # NULL outputs: only the status, or only the distance
    import ctypes as C
    q = np.ascontiguousarray(np.random.default_rng(1).uniform(-2, 2, size=(1000, 3)), np.float32)
    full = tsdf.query(q, "interpolate", gradient=True)
    st = np.zeros(1000, np.uint8)
    assert hip.fn("layer_query")(tsdf.h, q.ctypes.data_as(C.c_void_p), C.c_uint64(1000), C.c_int(1), C.c_int(1), None, None, None,
                                 st.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(st, full["status"])
    d = np.zeros(1000, np.float32)
    assert hip.fn("layer_query")(tsdf.h, q.ctypes.data_as(C.c_void_p), C.c_uint64(1000), C.c_int(1), C.c_int(0), d.ctypes.data_as(C.c_void_p), None,
                                 None, None) == 0
    v = (full["status"] & 1) != 0
    assert np.array_equal(_bits(d[v]), _bits(full["distance"][v]))
    assert hip.fn("layer_query")(tsdf.h, q.ctypes.data_as(C.c_void_p), C.c_uint64(1000), C.c_int(7), C.c_int(0), None, None, None, None) == -1
    # a layer that has grown between calls answers as before
    idx, vox = tsdf.download()
    grown = Layer(hip, voxel, capacity_blocks=len(idx) + 8)
    grown.upload(idx, vox)
    before = grown.query(q, "adaptive", gradient=True)
    grown.reserve(4 * len(idx) + 64)
    after = grown.query(q, "adaptive", gradient=True)
    for k in before:
        assert np.array_equal(np.asarray(before[k]).view(np.uint8), np.asarray(after[k]).view(np.uint8)), k
    n = esdf.free_points(0.0)[0].shape[0]
    import ctypes as C2
    cnt = C2.c_uint64()
    small = np.zeros((1, 3), np.float32)
    assert hip.fn("layer_free_points")(esdf.h, C2.c_float(0.0), small.ctypes.data_as(C2.c_void_p), None, C2.c_uint64(1), C2.byref(cnt)) == -7
    assert cnt.value == n


def test_cpp_map_flow_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "map_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "map_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
