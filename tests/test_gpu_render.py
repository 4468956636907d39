"""The GPU renderer (coxgraph_amd/csrc/cox_render.hip) against the test-side reference (tests/cpp/render_reference.cpp, whose
trilinear sample is the CPU checker's getVoxelsAndQVector), against the analytic scene, round the loop into the depth front end,
and in the orders the engine promises."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_ref
from coxgraph_amd import synth
from coxgraph_amd.capi import Integrator, Layer
from render_ref import R_BUDGET, R_COLOR, R_HIT, R_NORMAL
from test_render_cpu import PHYSICS_BOUNDS
from util import run_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return render_ref.build(tmp_path_factory.mktemp("renderref"))


@pytest.fixture(scope="module", params=[0.10, 0.05])
def submap(request, hip, ref):
    """The tests/test_gpu_submap.py submap: frames 0..140 step 10 of the benchmark stream, merged, subsample 2; its ESDF with
    coxgraph's band; and the reference's copies of both."""
    voxel = request.param
    layer, _, _ = run_frames(hip, method="merged", voxel=voxel, frames=range(0, 150, 10), subsample=2, capacity_blocks=8192)
    esdf = layer.esdf(max_distance_m=4.0, min_distance_m=0.1)
    return voxel, layer, esdf, ref.layer(voxel, *layer.download()), ref.layer(voxel, *esdf.download())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare(got, exp):
    """Bit identity of status, depth, normal and colour; NaN / 0 exactly where the bits are clear; the totals."""
    assert np.array_equal(got["status"], exp["status"])
    st = got["status"]
    hit, nrm, col = (st & R_HIT) != 0, (st & R_NORMAL) != 0, (st & R_COLOR) != 0
    assert np.array_equal(_bits(got["depth"][hit]), _bits(exp["depth"][hit])) and np.isnan(got["depth"][~hit]).all()
    assert np.array_equal(_bits(got["normal"][nrm]), _bits(exp["normal"][nrm])) and np.isnan(got["normal"][~nrm]).all()
    assert np.array_equal(got["rgba"], exp["rgba"]) and not got["rgba"][~col].any()
    if "stats" in got:
        for k in ("n_hits", "n_samples", "n_block_skips", "n_budget"):
            assert got["stats"][k] == exp["stats"][k], (k, got["stats"][k], exp["stats"][k])


def _poses():
    inside_wall = np.array(synth.camera_pose(20)[2])
    inside_wall[4:] = (4.15, 0.2, 1.5)  # 15 cm behind the x = 4 wall's surface, inside the truncation band
    away = np.array(synth.camera_pose(0)[2])
    away[4:] = (30.0, 0.0, 1.5)  # looks along +x from far outside: nothing in front of it
    return {
        "fused 70": synth.camera_pose(70)[2], "fused 0": synth.camera_pose(0)[2], "between 75": synth.camera_pose(75)[2],
        "between 33.3": synth.camera_pose(33.3)[2],
        "outside looking in": render_ref.look_at_pose([-3.0, -1.0, 2.0], synth.SPHERE_C)[2],  # behind every fused camera
        "inside a wall": inside_wall, "looking away": away,
    }


@pytest.mark.parametrize("size", [(640, 480), (160, 120)])
def test_render_is_bit_identical_to_the_reference(submap, size):
    voxel, tsdf, _, R, _ = submap
    w, h = size
    K = render_ref.scaled_intrinsics(w, h)
    for name, T in _poses().items():
        got, exp = tsdf.render(T, w, h, K), R.render(T, w, h, K)
        _compare(got, exp)
        s = got["stats"]
        print(f"{voxel} {w}x{h} {name}: hits {s['n_hits']}, {s['n_samples'] / (w * h):.1f} samples per ray, skips {s['n_block_skips']}, "
              f"kernel {s['kernel_ms']:.3f} ms, reference {exp['stats']['seconds']:.2f} s")
        if name.startswith(("fused", "between")):
            assert s["n_hits"] > 0.9 * w * h
        if name == "looking away":
            assert s["n_hits"] == 0 and not got["status"].any()
        if name == "outside looking in":
            assert s["n_hits"] > 100 and s["n_block_skips"] >= w * h  # every ray starts in unallocated space


def test_other_step_rules_and_an_esdf_are_bit_identical_too(submap):
    voxel, tsdf, esdf, R, RE = submap
    K = render_ref.scaled_intrinsics(320, 240)
    T = synth.camera_pose(75)[2]
    for cfg in (dict(step_scale=1.0, min_step_voxels=0.5), dict(step_scale=0.3, min_step_voxels=0.05, max_depth=4.0, min_depth=0.5),
                dict(step_scale=0.9, min_step_voxels=1.0, max_samples=12)):
        got = tsdf.render(T, 320, 240, K, **cfg)
        _compare(got, R.render(T, 320, 240, K, **cfg))
        print(f"{voxel} {cfg}: {got['stats']}")
    assert got["stats"]["n_budget"] > 0  # the last configuration runs some rays out of samples
    for name in ("between 75", "outside looking in"):
        T = _poses()[name]
        got = esdf.render(T, 320, 240, K)
        _compare(got, RE.render(T, 320, 240, K))
        print(f"{voxel} esdf {name}: {got['stats']}")
        assert got["stats"]["n_samples"] > 320 * 240


def test_a_view_through_unallocated_space_costs_a_probe_per_block(hip, ref):
    """One allocated block 6 m in front of the camera: every ray crosses at most 6 m / block edge + 2 blocks per axis on its way
    there and beyond, and takes no more samples than that plus a small constant."""
    vs = 0.05
    idx, words = render_ref.field_layer_arrays(vs, [(8, 0, 0)], lambda c: 6.8 - c[:, 0])  # the plane x = 6.8 inside block x in [6.4, 7.2)
    layer = Layer(hip, vs, capacity_blocks=16)
    layer.upload(idx, words)
    _, _, T = render_ref.look_at_pose([0.0, 0.4, 0.4], [6.8, 0.4, 0.4])
    K = np.array([2000.0, 2000.0, 79.5, 59.5], np.float32)  # a narrow view: every ray meets the block
    got, exp = layer.render(T, 160, 120, K), ref.layer(vs, idx, words).render(T, 160, 120, K)
    _compare(got, exp)
    assert got["stats"]["n_hits"] == 160 * 120
    blocks_crossed = 8 + 2  # x: 8 unallocated blocks of 0.8 m before the plane's; y, z: at most one face each
    in_block = 12           # 6.4 -> 6.8 m through the truncation-free field at 0.75 |d| steps down to the 1.25 cm minimum
    assert exp["samples"].max() <= blocks_crossed + in_block
    assert got["stats"]["n_block_skips"] <= 160 * 120 * blocks_crossed
    miss = layer.render(T, 160, 120, K, min_depth=7.5)  # starts behind the block: 2.5 m of nothing to max_depth
    assert miss["stats"]["n_hits"] == 0 and miss["stats"]["n_samples"] <= 160 * 120 * (4 + 2)


@pytest.mark.parametrize("frame", [70, 75])
def test_gpu_fused_map_renders_the_analytic_depth(submap, frame):
    """The CPU physics bounds (tests/test_render_cpu.py) on the HIP-fused layer rendered by the HIP kernel."""
    voxel, tsdf, _, _, _ = submap
    Rm, origin, T = synth.camera_pose(frame)
    out = tsdf.render(T, 640, 480)
    share, med, p95 = render_ref.error_in_voxels(out["depth"], synth.render_depth(Rm, origin), voxel)
    print(f"voxel {voxel} frame {frame}: hit {share:.4f}, |depth - analytic| median {med:.4f} p95 {p95:.4f} voxels")
    lo_share, hi_med, hi_p95 = PHYSICS_BOUNDS[voxel]
    assert share >= lo_share and med <= hi_med and p95 <= hi_p95


def test_rendered_depth_feeds_the_depth_front_end_on_the_device(hip, submap):
    import torch
    voxel, tsdf, _, _, _ = submap
    T = synth.camera_pose(75)[2]
    K = np.asarray(synth.INTRINSICS[(640, 480)], np.float32)
    depth = torch.zeros((480, 640), dtype=torch.float32, device="cuda")
    status = torch.zeros((480, 640), dtype=torch.uint8, device="cuda")
    tsdf.render_dev(T, 640, 480, K, depth=depth, status=status)
    torch.cuda.synchronize()
    n_hits = int((status & R_HIT).ne(0).sum().item())
    assert n_hits > 0.9 * 640 * 480
    fresh = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, fresh, hip.default_config(**synth.integrator_overrides(voxel)), "merged")
    integ.integrate_depth_dev(T, depth.data_ptr(), 0, 640, 480, K)
    integ.sync()
    assert integ.last_stats()["n_valid"] == n_hits
    src = {tuple(b) for b in tsdf.download()[0]}
    ring = {(x + dx, y + dy, z + dz) for (x, y, z) in src for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)}
    new = {tuple(b) for b in fresh.download()[0]}
    assert len(new) > 10 and new <= ring


def test_a_render_sees_the_frames_enqueued_before_it(hip):
    voxel = 0.05
    cfg = hip.default_config(**synth.integrator_overrides(voxel))
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, cfg, "merged")
    frames = []
    for t in range(0, 40, 10):
        T, pts, rgba, _ = synth.make_frame(t)
        frames.append((T, np.ascontiguousarray(pts[::2]), np.ascontiguousarray(rgba[::2])))
    K = render_ref.scaled_intrinsics(320, 240)
    Tv = synth.camera_pose(15)[2]
    for T, pts, rgba in frames:
        integ.integrate_points_async(T, pts.ctypes.data, rgba.ctypes.data, len(pts))
    early = layer.render(Tv, 320, 240, K)  # no sync in between
    integ.sync()
    late = layer.render(Tv, 320, 240, K)
    for k in ("depth", "normal", "rgba", "status"):
        assert np.array_equal(early[k].view(np.uint8), late[k].view(np.uint8)), k
    assert late["stats"]["n_hits"] > 0.5 * 320 * 240


def test_render_dev_on_a_side_stream_gives_the_same_bits(submap):
    import torch
    voxel, tsdf, _, _, _ = submap
    K = render_ref.scaled_intrinsics(320, 240)
    T = _poses()["outside looking in"]
    host = tsdf.render(T, 320, 240, K)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # stale contents: every pixel must be overwritten, misses included
        d = torch.full((240, 320), 7.0, device="cuda")
        n = torch.full((240, 320, 3), 7.0, device="cuda")
        c = torch.full((240, 320, 4), 7, dtype=torch.uint8, device="cuda")
        st = torch.full((240, 320), 7, dtype=torch.uint8, device="cuda")
        tsdf.render_dev(T, 320, 240, K, depth=d, normal=n, rgba=c, status=st, stream=s)
    s.synchronize()
    _compare(dict(depth=d.cpu().numpy(), normal=n.cpu().numpy(), rgba=c.cpu().numpy(), status=st.cpu().numpy()), host)
    assert (host["status"] == 0).any() and (host["status"] & R_HIT).any()


def test_edges(hip, submap):
    voxel, tsdf, _, _, _ = submap
    K = render_ref.scaled_intrinsics(160, 120)
    T = synth.camera_pose(75)[2]
    # an empty layer: all misses, one probe per block crossed
    empty = Layer(hip, voxel, capacity_blocks=64)
    out = empty.render(T, 160, 120, K)
    assert not out["status"].any() and np.isnan(out["depth"]).all() and np.isnan(out["normal"]).all() and not out["rgba"].any()
    assert out["stats"]["n_hits"] == 0 and out["stats"]["n_block_skips"] == out["stats"]["n_samples"] > 0
    # a layer grown between two renders answers as before
    idx, vox = tsdf.download()
    grown = Layer(hip, voxel, capacity_blocks=len(idx) + 8)
    grown.upload(idx, vox)
    before = grown.render(T, 160, 120, K)
    grown.reserve(4 * len(idx) + 64)
    after = grown.render(T, 160, 120, K)
    _compare(after, before)
    # every output NULL except one
    full = tsdf.render(T, 160, 120, K)
    f = hip.fn("layer_render")
    Tp, Kp = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(K, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for k, arr in (("depth", np.zeros((120, 160), np.float32)), ("normal", np.zeros((120, 160, 3), np.float32)),
                   ("rgba", np.ones((120, 160, 4), np.uint8)), ("status", np.ones((120, 160), np.uint8))):
        args = [p(arr) if k == name else None for name in ("depth", "normal", "rgba", "status")]
        assert f(tsdf.h, p(Tp), C.c_int(160), C.c_int(120), p(Kp), None, *args, None) == 0
        assert np.array_equal(arr.view(np.uint8), full[k].view(np.uint8)), k
    assert f(tsdf.h, p(Tp), C.c_int(160), C.c_int(120), p(Kp), None, None, None, None, None, None) == 0
    # an image that is not a multiple of the tile
    odd = tsdf.render(T, 37, 19, render_ref.scaled_intrinsics(37, 19))
    assert odd["stats"]["n_hits"] == int(((odd["status"] & R_HIT) != 0).sum()) > 0
    # max_samples = 1: nothing but the budget bit
    one = tsdf.render(T, 160, 120, K, max_samples=1)
    assert np.all(one["status"] == R_BUDGET) and one["stats"]["n_budget"] == 160 * 120 and one["stats"]["n_samples"] == 160 * 120


def test_invalid_arguments(hip, submap):
    _, tsdf, _, _, _ = submap
    f, fd = hip.fn("layer_render"), hip.fn("layer_render_dev")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    T, K = np.array(synth.camera_pose(0)[2], np.float32), np.array([100, 100, 8, 8], np.float32)
    d = np.zeros((16, 16), np.float32)

    def call(layer=tsdf.h, T=T, w=16, h=16, K=K, cfg=None):
        from coxgraph_amd.capi import RenderConfig
        c = None
        if cfg is not None:
            c = RenderConfig()
            hip.fn("render_config_default", None)(C.byref(c))
            for k, v in cfg.items():
                setattr(c, k, v)
            c = C.byref(c)
        args = (layer, p(T) if T is not None else None, C.c_int(w), C.c_int(h), p(K) if K is not None else None, c, p(d), None, None, None)
        return f(*args, None), fd(*args[:6], None, None, None, None, None)

    assert call() == (0, 0)
    bad = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(np.float32)
    for kw in (dict(layer=None), dict(T=None), dict(K=None), dict(w=0), dict(h=-1), dict(w=65536, h=32768), dict(T=bad(T, 5, np.nan)),
               dict(T=bad(T, 0, np.inf)), dict(K=bad(K, 2, np.nan)), dict(K=bad(K, 0, 0.0)), dict(K=bad(K, 1, 0.0)),
               dict(cfg=dict(max_depth=0.05)), dict(cfg=dict(min_depth=-0.1)), dict(cfg=dict(step_scale=0.0)), dict(cfg=dict(step_scale=float("nan"))),
               dict(cfg=dict(max_depth=float("nan")))):
        assert call(**kw) == (-1, -1), kw


def test_cpp_render_view_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "render_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "render_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
