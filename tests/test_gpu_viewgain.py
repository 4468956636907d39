"""The GPU view-gain evaluator (coxgraph_amd/csrc/cox_viewgain.hip) against the test-side reference
(tests/cpp/viewgain_reference.cpp), against a numpy recount of a hand-built corridor, and in the orders the engine promises.

Visible sets (voxel_xyz, cls) and all integer counts are bit-identical; value and surface_gain agree within a relative 1e-5 (atan2f
is not correctly rounded on either side).  Every input is one for which the reference reports n_borderline == 0 (no occupied voxel
whose impact is within 1e-5 of min_impact_factor), asserted here, so n_surface_counted must match exactly as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_ref
import viewgain_ref
from coxgraph_amd import synth
from coxgraph_amd.capi import VIEW_GAIN_DTYPE, CoxError, Integrator, Layer, ViewGain, ViewGainRecord, viewgain_config
from util import run_frames
from viewgain_ref import COUNTS, FRONTIER, at, pose_looking

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS = 0.05
GRIDS = {  # w, h, K
    "1x1": dict(w=1, h=1, K=(64.0, 64.0, 0.0, 0.0)),
    "7x5": dict(w=7, h=5, K=(8.0, 8.0, 3.0, 2.0)),      # a partial 8 x 8 tile
    "9x17": dict(w=9, h=17, K=(12.0, 12.0, 4.0, 8.0)),  # several tiles, partial at both edges
    "35x96": {},                                        # the configured one
}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return viewgain_ref.build(tmp_path_factory.mktemp("viewgainref"))


def _upload(hip, vs, idx, words, capacity=0):
    layer = Layer(hip, vs, capacity_blocks=capacity or len(idx) + 8)
    if len(idx):
        layer.upload(idx, words)
    return layer


def _compare(hip, layer, R, poses, visible=True, **cfg):
    """evaluate and (per pose) visible against the reference; returns the engine's output."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
    vg = ViewGain(hip, layer, **cfg)
    got, exp = vg.evaluate(poses), R.evaluate(poses, **cfg)
    print({k: got[k].tolist() for k in COUNTS}, got["gain"].tolist(), got["stats"], f"reference {exp['seconds']:.3f} s")
    assert not exp["n_borderline"].any(), exp["n_borderline"]
    for k in COUNTS:
        assert np.array_equal(got[k], exp[k]), (k, got[k], exp[k])
    assert got["stats"]["n_samples"] == int(exp["n_samples"].sum())
    assert np.allclose(got["surface_gain"], exp["surface_gain"], rtol=1e-5, atol=0)
    assert np.array_equal(got["surface_gain"], got["surface_gain_q32"].astype(np.float64) / 2.0 ** 32)
    c = vg.cfg
    want_gain = got["surface_gain"] + float(c.frontier_voxel_weight) * got["n_frontier"] + float(c.new_voxel_weight) * (got["n_unknown"] - got["n_frontier"])
    assert np.array_equal(got["gain"], want_gain)
    assert np.array_equal(got["n_visible"], got["n_free"] + got["n_occupied"] + got["n_unknown"])
    if visible:
        for i, T in enumerate(poses):
            gv, ev = vg.visible(T), R.visible(T, **cfg)
            assert np.array_equal(gv["voxel_xyz"], ev["voxel_xyz"]) and np.array_equal(gv["cls"], ev["cls"])
            assert np.allclose(gv["value"], ev["value"], rtol=1e-5, atol=0)
            assert len(gv["cls"]) == got["n_visible"][i] and int((gv["cls"] == FRONTIER).sum()) == got["n_frontier"][i]
    vg.close()
    return got


# ---- hand-built layers at 5 cm ---------------------------------------------------------------------------------------------------
def _wall():
    return viewgain_ref.corridor_wall_arrays(VS, 2.0)


def _sphere():
    return render_ref.sphere_layer_arrays(VS, np.array([0.8 + 0.013, 0.8 - 0.021, 0.8 + 0.007]), 0.35, trunc=5 * VS)


def _far_block():
    # a single allocated block 3.2 .. 4.0 m out along x, holding the plane x = 3.6 seen from the origin's side
    return render_ref.field_layer_arrays(VS, [(4, 0, 0)], lambda c: 3.6 - c[:, 0])


WALL_POSES = {
    "head-on": pose_looking((1.0, 0.4, 0.4), (1, 0, 0)),
    "along the x axis through a voxel centre line": pose_looking((0.125, 0.425, 0.425), (1, 0, 0)),
    "along a face diagonal": pose_looking((0.3, -0.3, 0.425), (1, 1, 0)),
    "origin exactly on a block face": pose_looking((0.8, 0.8, 0.0), (1, 0.2, 0.1)),
    "origin inside an occupied voxel": pose_looking((1.975, 0.41, 0.43), (-1, 0.1, 0)),
    "sideways into unobserved space": pose_looking((1.0, 0.4, 0.4), (0, 1, 0)),
    "looking away from everything": pose_looking((-1.0, 0.4, 0.4), (-1, 0, 0)),
    "30 m from the data": pose_looking((30.0, 0.4, 0.4), (-1, 0, 0)),
}


@pytest.mark.parametrize("grid", list(GRIDS))
def test_wall_layer_matches_the_reference(hip, ref, grid):
    idx, words = _wall()
    layer, R = _upload(hip, VS, idx, words), ref.layer(VS, idx, words)
    got = _compare(hip, layer, R, list(WALL_POSES.values()), visible=grid != "35x96", **GRIDS[grid])
    names = list(WALL_POSES)
    assert got["n_occupied"][names.index("head-on")] >= 1 and got["n_unknown"][names.index("head-on")] == 0
    assert got["n_visible"][names.index("origin inside an occupied voxel")] == 1  # every ray ends on its first sample
    for far in ("looking away from everything", "30 m from the data"):
        i = names.index(far)
        assert got["n_visible"][i] == got["n_unknown"][i] > 0 and got["n_frontier"][i] == 0 and got["gain"][i] == 0.0
    if grid == "35x96":
        _compare(hip, layer, R, [WALL_POSES["head-on"], WALL_POSES["sideways into unobserved space"]], **GRIDS[grid])


def test_sphere_and_a_block_in_empty_space_match_the_reference(hip, ref):
    idx, words = _sphere()
    layer, R = _upload(hip, VS, idx, words), ref.layer(VS, idx, words)
    c = np.array([0.813, 0.779, 0.807])
    poses = [pose_looking(o, c - np.array(o)) for o in ([0.8, -0.9, 0.8], [-0.7, 0.3, 1.3], [1.2, 1.4, -0.8])]
    poses.append(pose_looking(c, (0, 1, 0.2)))  # from inside the sphere: the first sample is occupied
    for grid in ("9x17", "35x96"):
        got = _compare(hip, layer, R, poses, **GRIDS[grid])
        assert (got["n_occupied"][:3] > 0).all() and got["n_visible"][3] == 1
    # a lower threshold on what counts: fewer counted than occupied from afar (weight 1: impact 0.5 where nw = 1, about 4.4 m out)
    far = [pose_looking((0.8, -3.75, 0.8), (0, 1, 0)), pose_looking((-3.0, 0.8, 0.8), (1, 0, 0))]
    got = _compare(hip, layer, R, far, min_impact_factor=0.5, w=9, h=17, K=(60.0, 60.0, 4.0, 8.0))  # a narrow grid: every ray meets the sphere
    assert (got["n_surface_counted"] < got["n_occupied"]).any()
    idx, words = _far_block()
    layer, R = _upload(hip, VS, idx, words), ref.layer(VS, idx, words)
    poses = [pose_looking((0.0, 0.4, 0.4), (1, 0, 0)), pose_looking((0.0, 0.4, 0.4), (1, 0.12, -0.1)), pose_looking((3.0, 2.0, 0.4), (0.2, -1, 0))]
    for kw in (dict(), dict(surface_frontiers=0), dict(surface_frontiers=0, accurate_frontiers=0)):
        got = _compare(hip, layer, R, poses, **kw)
        assert got["n_occupied"][0] > 0 and got["n_unknown"][0] > got["n_free"][0] > 0  # in through unallocated blocks, and (beside the plane) out again
    assert got["n_frontier"][0] > 0


def test_batches_chunks_and_repeats(hip, ref):
    idx, words = _wall()
    layer, R = _upload(hip, VS, idx, words), ref.layer(VS, idx, words)
    rng = np.random.default_rng(5)
    poses = [pose_looking(rng.uniform((0.1, -0.6, -0.6), (1.9, 1.4, 1.4)), rng.normal(size=3)) for _ in range(64)]
    poses.insert(7, poses[3])  # the same pose twice in one batch
    poses = np.array(poses, np.float32)
    cfg = GRIDS["9x17"]
    got = _compare(hip, layer, R, poses, visible=False, **cfg)
    assert got["stats"]["n_chunks"] == 1
    for k in VIEW_GAIN_DTYPE.names:
        assert got[k][7] == got[k][3], k
    vg = ViewGain(hip, layer, **cfg)
    for n in (1, 2):
        part = vg.evaluate(poses[10:10 + n])
        for k in VIEW_GAIN_DTYPE.names:
            assert np.array_equal(part[k], got[k][10:10 + n]), k
    alone = vg.evaluate(poses[40])
    for k in VIEW_GAIN_DTYPE.names:
        assert alone[k][0] == got[k][40], k
    # a workspace that fits one view at a time
    one = ViewGain(hip, layer, workspace_bytes=vg.view_bytes(), **cfg)
    cut = one.evaluate(poses)
    assert cut["stats"]["n_chunks"] == len(poses)
    for k in VIEW_GAIN_DTYPE.names:
        assert np.array_equal(cut[k], got[k]), k
    three = ViewGain(hip, layer, workspace_bytes=3 * vg.view_bytes() + 5, **cfg).evaluate(poses)
    assert three["stats"]["n_chunks"] == (len(poses) + 2) // 3
    for k in VIEW_GAIN_DTYPE.names:
        assert np.array_equal(three[k], got[k]), k
    # one byte short of one view
    with pytest.raises(CoxError) as e:
        ViewGain(hip, layer, workspace_bytes=vg.view_bytes() - 1, **cfg).evaluate(poses[:1])
    assert e.value.status == -3
    assert Layer.view_gain(layer, poses[:2], **cfg)["gain"].tolist() == got["gain"][:2].tolist()


def test_an_empty_layer_and_a_translation_out_of_range(hip, ref):
    empty = Layer(hip, VS, capacity_blocks=16)
    R = ref.layer(VS, np.zeros((0, 3), np.int32), np.zeros((0, 4096, 3), np.uint32))
    poses = [pose_looking((0.3, 0.2, 0.1), (1, 0.3, 0.2)), at((1e9, 0.0, 0.0)), at((0.0, -1e9, 3e8), q=(0.5, 0.5, 0.5, 0.5))]
    got = _compare(hip, empty, R, poses, **GRIDS["9x17"])
    assert got["n_visible"][0] == got["n_unknown"][0] > 100 and got["n_frontier"][0] == 0
    for i in (1, 2):  # outside the index range: the view is empty
        assert all(got[k][i] == 0 for k in COUNTS) and got["gain"][i] == 0.0
    assert got["stats"]["n_samples"] == 9 * 17 * 100  # every sample of the first view, none of the others


# ---- physics anchor: no reference ------------------------------------------------------------------------------------------------
def _np_rotate(q, v):
    qv = np.broadcast_to(q[1:4], v.shape)
    cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    uv = cross(qv, v)
    uv = uv + uv
    return (v + q[0] * uv) + cross(qv, uv)


def _np_sample_voxels(T, vs, w=35, h=96, K=(64.0, 64.0, 17.0, 48.0), ray_length=5.0):
    """Global voxel indices int64[rays, samples, 3] of every sample of every ray of the view, rules 1 and 2 in float32."""
    f = np.float32
    T = np.asarray(T, f)
    u, v = np.meshgrid(np.arange(w, dtype=f), np.arange(h, dtype=f))
    x, y = (u.ravel() - f(K[2])) / f(K[0]), (v.ravel() - f(K[3])) / f(K[1])
    n = np.sqrt(x * x + y * y + f(1))
    dirs = _np_rotate(T[:4], np.stack([x / n, y / n, f(1) / n], -1))
    d = np.arange(4096, dtype=f) * f(vs)
    d = d[d < f(ray_length)]
    p = T[4:][None, None, :] + d[None, :, None] * dirs[:, None, :]
    bs = f(vs) * f(16)
    bsi, vsi = f(1.0 / float(bs)), f(1.0 / float(f(vs)))
    b = np.floor(p * bsi + f(1e-6))
    vv = np.clip(np.floor((p - b * bs) * vsi + f(1e-6)), 0, 15)
    return (16 * b + vv).astype(np.int64)


def test_corridor_counts_from_a_numpy_recount(hip):
    """A wall observed only in front of the plane x = 2 m (x index 39 occupied), the free corridor observed out to it over y, z
    index -16 .. 31; nothing else is known.  The recount marches the same samples in numpy and classifies them from that
    description alone."""
    idx, words = _wall()
    layer = _upload(hip, VS, idx, words)
    observed = lambda g: (g[..., 0] >= 0) & (g[..., 0] <= 39) & (g[..., 1] >= -16) & (g[..., 1] <= 31) & (g[..., 2] >= -16) & (g[..., 2] <= 31)
    occupied = lambda g: observed(g) & (g[..., 0] == 39)
    nb = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)])

    def recount(T, surface_frontiers):
        g = _np_sample_voxels(T, VS)
        occ = occupied(g)
        first = np.where(occ.any(1), occ.argmax(1), g.shape[1])
        keep = np.arange(g.shape[1])[None, :] <= first[:, None]  # a ray ends after its first occupied sample
        vis = np.unique(g[keep], axis=0)
        unknown = ~observed(vis)
        near = vis[unknown][:, None, :] + nb[None]
        frontier = (occupied(near) if surface_frontiers else observed(near)).any(1)
        return dict(n_visible=len(vis), n_occupied=int(occupied(vis).sum()), n_free=int((observed(vis) & ~occupied(vis)).sum()),
                    n_unknown=int(unknown.sum()), n_frontier=int(frontier.sum()))

    head_on, sideways = WALL_POSES["head-on"], WALL_POSES["sideways into unobserved space"]
    for sf in (1, 0):
        got = layer.view_gain([head_on, sideways], surface_frontiers=sf)
        for i, T in enumerate((head_on, sideways)):
            want = recount(T, sf)
            print(sf, i, want)
            assert {k: int(got[k][i]) for k in want} == want
    # facing the wall from 1 m: exactly the wall voxels of the footprint, nothing unknown; turned towards unobserved space: frontiers
    # along the side of the corridor (where observed is enough), none at a surface
    assert got["n_unknown"][0] == 0 and got["n_frontier"][0] == 0 and got["n_occupied"][0] > 300
    assert got["n_frontier"][1] > 300 and got["n_occupied"][1] == 0


# ---- one fused layer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused(hip, ref):
    layer, _, _ = run_frames(hip, "merged", voxel=0.10, frames=range(0, 150, 10), subsample=2, capacity_blocks=8192)
    esdf = layer.esdf(max_distance_m=4.0, min_distance_m=0.1)
    return layer, esdf, ref.layer(0.10, *layer.download()), ref.layer(0.10, *esdf.download())


FUSED_POSES = [synth.camera_pose(70)[2], synth.camera_pose(75)[2], render_ref.look_at_pose([-3.0, -1.0, 2.0], synth.SPHERE_C)[2]]
FUSED_CONFIGS = [dict(), dict(surface_frontiers=0), dict(accurate_frontiers=0), dict(min_range=0.5), dict(ray_step=0.05),
                 dict(use_box=1, box_min=(0.0, -1.5, 0.3), box_max=(3.0, 1.5, 2.2)), dict(frontier_voxel_weight=0.0, new_voxel_weight=1.0)]


@pytest.mark.parametrize("cfg", FUSED_CONFIGS, ids=[",".join(c) or "defaults" for c in FUSED_CONFIGS])
def test_fused_layer_matches_the_reference(hip, fused, cfg):
    tsdf, esdf, R, RE = fused
    got = _compare(hip, tsdf, R, FUSED_POSES, **cfg)
    assert (got["n_occupied"][:2] > 0).all() and (got["n_free"][:2] > 0).all() and got["n_unknown"][2] > 0
    if "frontier_voxel_weight" in cfg:
        assert not got["n_frontier"].any() and np.array_equal(got["gain"], got["surface_gain"] + got["n_unknown"])
    if not cfg:
        # the ESDF of the same map: occupied where the signed distance is not positive
        _compare(hip, esdf, RE, FUSED_POSES, visible=False)


# ---- ordering and the device path ------------------------------------------------------------------------------------------------
def test_evaluate_dev_on_a_side_stream_equals_evaluate(hip, fused):
    import torch
    tsdf = fused[0]
    poses = np.array(FUSED_POSES + [synth.camera_pose(t)[2] for t in (10, 33.3)], np.float32)
    vg = ViewGain(hip, tsdf)
    host = vg.evaluate(poses)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dp = torch.from_numpy(poses).cuda()
        out = torch.full((len(poses) * 48,), 7, dtype=torch.uint8, device="cuda")  # stale contents
        vg.evaluate_dev(dp, out, stream=s)
    s.synchronize()
    rec = out.cpu().numpy().view(VIEW_GAIN_DTYPE)
    for k in VIEW_GAIN_DTYPE.names:
        assert np.array_equal(rec[k], host[k]), k
    assert (host["n_visible"] > 1000).all()


def test_a_call_sees_the_frames_enqueued_before_it_and_survives_growth(hip):
    voxel = 0.10
    cfg = hip.default_config(**synth.integrator_overrides(voxel))
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, cfg, "merged")
    vg = ViewGain(hip, layer)
    Tv = synth.camera_pose(15)[2]
    before = vg.evaluate(Tv)
    assert before["n_visible"][0] == before["n_unknown"][0]  # nothing fused yet
    frames = []
    for t in range(0, 40, 10):
        T, pts, rgba, _ = synth.make_frame(t)
        frames.append((T, np.ascontiguousarray(pts[::2]), np.ascontiguousarray(rgba[::2])))
    for T, pts, rgba in frames:
        integ.integrate_points_async(T, pts.ctypes.data, rgba.ctypes.data, len(pts))
    early = vg.evaluate(Tv)  # no sync in between
    integ.sync()
    late = vg.evaluate(Tv)
    for k in VIEW_GAIN_DTYPE.names:
        assert early[k][0] == late[k][0], k
    assert late["n_occupied"][0] > 100
    layer.reserve(layer.capacity() + 4096)  # the pool moves: the handle reads the layer again
    grown = vg.evaluate(Tv)
    for k in VIEW_GAIN_DTYPE.names:
        assert grown[k][0] == late[k][0], k


def test_error_codes_and_no_views(hip, fused):
    tsdf = fused[0]
    create, evaluate, visible = hip.fn("viewgain_create"), hip.fn("viewgain_evaluate"), hip.fn("viewgain_visible")
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def status(**cfg):
        c, h = viewgain_config(hip, **cfg), C.c_void_p()
        st = create(tsdf.h, C.byref(c), C.byref(h))
        if h:
            hip.fn("viewgain_destroy", None)(h)
        return st

    nan, inf = float("nan"), float("inf")
    assert status() == 0 and status(use_box=1, box_min=(0, 0, 0), box_max=(0, 0, 0)) == 0
    for bad in (dict(w=0), dict(h=-1), dict(K=(0, 64, 17, 48)), dict(K=(64, 0, 17, 48)), dict(K=(64, 64, nan, 48)), dict(K=(inf, 64, 17, 48)),
                dict(ray_length=nan), dict(ray_length=0.0), dict(min_range=5.0), dict(min_range=-0.1), dict(min_range=nan), dict(ray_step=-0.05),
                dict(ray_step=inf), dict(ray_step=1e-9), dict(ray_angle_x=-0.002454), dict(ray_angle_y=0.0), dict(ray_angle_x=nan),
                dict(min_weight=nan), dict(frontier_voxel_weight=inf), dict(new_voxel_weight=nan), dict(min_impact_factor=nan),
                dict(surface_distance=nan), dict(use_box=1, box_min=(0, 0, 1), box_max=(1, 1, 0)), dict(use_box=1, box_min=(0, nan, 0), box_max=(1, 1, 1))):
        assert status(**bad) == -1, bad
    h = C.c_void_p()
    assert create(None, None, C.byref(h)) == -1 and create(tsdf.h, None, None) == -1
    vg = ViewGain(hip, tsdf)
    T = np.array(FUSED_POSES[0], np.float32)
    rec = np.full(2, 7, VIEW_GAIN_DTYPE)
    n = C.c_uint64(99)
    assert evaluate(vg.h, None, C.c_uint64(0), None, None) == 0 and evaluate(vg.h, p(T), C.c_uint64(0), p(rec), None) == 0  # n_views = 0
    assert (rec["n_visible"] == 7).all()  # nothing written
    assert hip.fn("viewgain_evaluate_dev")(vg.h, None, C.c_uint64(0), None, None) == 0
    assert evaluate(vg.h, None, C.c_uint64(1), p(rec), None) == -1 and evaluate(vg.h, p(T), C.c_uint64(1), None, None) == -1
    assert evaluate(None, p(T), C.c_uint64(1), p(rec), None) == -1
    for i, v in ((5, nan), (0, inf)):
        Tb = T.copy()
        Tb[i] = v
        assert evaluate(vg.h, p(Tb), C.c_uint64(1), p(rec), None) == -1
        assert visible(vg.h, p(Tb), C.c_uint64(0), None, None, None, C.byref(n)) == -1
    assert hip.fn("viewgain_evaluate_dev")(vg.h, None, C.c_uint64(1), None, None) == -1
    assert visible(vg.h, p(T), C.c_uint64(0), None, None, None, None) == -1 and visible(None, p(T), C.c_uint64(0), None, None, None, C.byref(n)) == -1
    # cap = 0 with NULL buffers queries n; a buffer that is too small is refused; any one buffer alone is fine
    assert visible(vg.h, p(T), C.c_uint64(0), None, None, None, C.byref(n)) == 0 and n.value == vg.evaluate(T)["n_visible"][0] > 1000
    cls = np.zeros(n.value, np.uint8)
    assert visible(vg.h, p(T), C.c_uint64(n.value - 1), None, p(cls), None, C.byref(n)) == -7
    assert visible(vg.h, p(T), C.c_uint64(n.value), None, p(cls), None, C.byref(n)) == 0
    assert np.array_equal(cls, vg.visible(T)["cls"]) and set(np.unique(cls)) <= {0, 1, 2, 3}
    assert C.sizeof(ViewGainRecord) == 48


def test_cpp_yaw_sweep_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "viewgain_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "viewgain_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
