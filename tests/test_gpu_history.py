"""Observation histories on the GPU (coxgraph_amd/csrc/cox_history.hip) against the numpy restatement of the rule
(tests/history_ref.py), against physics that needs no restatement (two walls and a camera that turns), and end to end:
depth frames -> layer + record -> mesh message with histories -> recover mode's layer."""
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import history_ref as hr
from coxgraph_amd import synth
from coxgraph_amd.capi import CoxError, Integrator, Layer, MeshConverter, MeshLayer, MeshMsg, ObservationHistory

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERA = dict(sensor_horizontal_resolution=1280, sensor_vertical_resolution=960, sensor_vertical_field_of_view_degrees=360.0)
FRAME_IDS = (0, 31, 32, 200, 255)  # both sides of a word boundary, the last word, the last bit


def _cfg(hip, voxel, method="merged"):
    ov = synth.integrator_overrides(voxel)
    if method == "projective":
        ov.update(CAMERA)
    return hip.default_config(**ov)


def _scene(voxel, sub=2):
    """Five frames of the synthetic stream with the points no sensor driver would pass on mixed in: NaN, +-inf, and points
    on, just inside and just outside both range limits."""
    ov = synth.integrator_overrides(voxel)
    lo, hi = np.float32(ov["min_ray_length_m"]), np.float32(ov["max_ray_length_m"])
    rng = np.random.default_rng(17)
    frames = []
    for k, t in enumerate(range(0, 50, 10)):
        T, pts, _, _ = synth.make_frame(t)
        pts = np.ascontiguousarray(pts[::sub]).copy()
        d = rng.normal(size=(60, 3))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        scale = np.repeat(np.array([lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(9)), lo * np.float32(0.999), lo * np.float32(1.001),
                                    hi, np.nextafter(hi, np.float32(0)), np.nextafter(hi, np.float32(99)), hi * np.float32(0.999), hi * np.float32(1.001)], np.float32), 6)
        edge = d * scale[:, None]
        bad = np.array([[np.nan, 0, 1], [0, np.nan, 1], [1, 1, np.nan], [np.inf, 0, 1], [0, -np.inf, 1], [1, 2, np.inf], [np.nan, np.inf, -np.inf]], np.float32)
        where = rng.integers(0, len(pts), len(edge) + len(bad))
        pts[where] = np.concatenate([edge, bad])
        frames.append((T, pts, FRAME_IDS[k]))
    return ov, frames


def _reference(voxel, ov, frames):
    rec = hr.Record(voxel)
    for T, pts, fid in frames:
        rec.mark(T, pts, fid, ov["min_ray_length_m"], ov["max_ray_length_m"])
    return rec.arrays()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("voxel", [0.10, 0.05, 0.02])
def test_direct_record_is_bit_identical_to_the_reference(hip, voxel):
    ov, frames = _scene(voxel)
    want = _reference(voxel, ov, frames)
    assert len(want[0]) > 10 and np.count_nonzero(want[1]) > 100
    layer = Layer(hip, voxel, capacity_blocks=64)
    dev, host = ObservationHistory(hip, layer, 4096), ObservationHistory(hip, layer, 4096)
    keep = []
    for T, pts, fid in frames:
        x = torch.from_numpy(pts).cuda()
        keep.append(x)
        dev.set_frame(fid), host.set_frame(fid)
        dev.record_dev(T, x, ov["min_ray_length_m"], ov["max_ray_length_m"], stream=torch.cuda.current_stream())
        host.record(T, pts, ov["min_ray_length_m"], ov["max_ray_length_m"])
    dev.sync(), host.sync()
    assert _same(dev.download(), want) and _same(host.download(), want)
    st = dev.stats()
    assert st["blocks"] == len(want[0]) and st["marked_cells"] == int(np.count_nonzero(want[1].any(axis=2))) and st["bytes"] >= 4096 * 2048
    marking, atomics = dev.counts()
    n_mark = sum(int(hr.marking_points(p, ov["min_ray_length_m"], ov["max_ray_length_m"]).sum()) for _, p, _ in frames)
    print(f"voxel {voxel}: {marking} marking points, {atomics} after the wave-level merge")
    assert marking == n_mark and st["marked_cells"] <= atomics < marking


@pytest.mark.parametrize("method", ["simple", "merged", "fast", "projective"])
@pytest.mark.parametrize("voxel", [0.10, 0.05, 0.02])
def test_attached_record_is_bit_identical_to_the_reference(hip, voxel, method):
    ov, frames = _scene(voxel, sub=4)
    want = _reference(voxel, ov, frames)
    layers = []
    for attach in (True, False):
        layer = Layer(hip, voxel, capacity_blocks=8192)
        integ = Integrator(hip, layer, _cfg(hip, voxel, method), method)
        obs = ObservationHistory(hip, layer, 4096)
        if attach:
            integ.attach_history(obs)
        for T, pts, fid in frames:
            obs.set_frame(fid)
            integ.integrate_points(T, pts)
        integ.sync(), obs.sync()
        got = obs.download()
        if attach:
            assert _same(got, want)
        else:
            assert got[0].shape == (0, 3)
        layers.append(layer.download())
        integ.attach_history(None)
    # the record reads, it writes nothing of the layer's: fused with and without it, the layer is the same to the bit
    assert np.array_equal(layers[0][0], layers[1][0]) and np.array_equal(layers[0][1], layers[1][1])


@pytest.mark.parametrize("path", ["dev", "async", "dev_on_stream"])
def test_attached_device_and_async_paths(hip, path):
    voxel = 0.05
    ov, frames = _scene(voxel)
    want = _reference(voxel, ov, frames)
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, _cfg(hip, voxel), "merged")
    obs = ObservationHistory(hip, layer, 4096)
    integ.attach_history(obs)
    keep = []
    stream = torch.cuda.Stream()
    if path == "dev_on_stream":
        integ.set_input_stream(stream.cuda_stream)
    for T, pts, fid in frames:
        obs.set_frame(fid)
        if path == "async":
            keep.append(pts)
            integ.integrate_points_async(T, pts.ctypes.data, 0, len(pts))
        elif path == "dev":
            x = torch.from_numpy(pts).cuda()
            torch.cuda.synchronize()
            keep.append(x)
            integ.integrate_points_dev(T, x.data_ptr(), 0, len(pts))
        else:
            with torch.cuda.stream(stream):
                x = torch.from_numpy(pts).cuda(non_blocking=True) + 0.0  # produced on the caller's stream, not waited for
            keep.append(x)
            integ.integrate_points_dev(T, x.data_ptr(), 0, len(pts))
    early = obs.download()  # right behind the last call: orders itself behind the records in flight
    integ.sync(), obs.sync()
    assert _same(early, want) and _same(obs.download(), want)
    # the depth-image entry points do not record: refused while a history is attached, fine again afterwards
    T, _, _, depth = synth.make_frame(0)
    K = np.array(synth.INTRINSICS[(640, 480)], np.float32)
    with pytest.raises(CoxError) as e:
        integ.integrate_depth_async(T, depth.ctypes.data, 0, 640, 480, K)
    assert e.value.status == -6
    integ.attach_history(None)
    integ.integrate_depth_async(T, depth.ctypes.data, 0, 640, 480, K)
    integ.sync()
    assert _same(obs.download(), want)


def test_freespace_and_deintegration_leave_the_record_alone(hip):
    voxel = 0.10
    ov, frames = _scene(voxel, sub=4)
    layer = Layer(hip, voxel, capacity_blocks=8192)
    obs = ObservationHistory(hip, layer)
    T, pts, _ = frames[0]
    obs.record(T, pts, ov["min_ray_length_m"], ov["max_ray_length_m"], freespace=True)
    obs.record_dev(T, torch.from_numpy(pts).cuda(), ov["min_ray_length_m"], ov["max_ray_length_m"], freespace=True)
    integ = Integrator(hip, layer, _cfg(hip, voxel), "merged")
    integ.attach_history(obs)
    integ.integrate_points(T, pts, freespace=True)
    obs.sync()
    assert obs.download()[0].shape == (0, 3) and obs.stats()["blocks"] == 0
    # allow_clear only decides what a point beyond the range becomes; it marks neither way
    a, b = ObservationHistory(hip, layer), ObservationHistory(hip, layer)
    a.record(T, pts, ov["min_ray_length_m"], 2.0, allow_clear=True)
    b.record(T, pts, ov["min_ray_length_m"], 2.0, allow_clear=False)
    want = hr.Record(voxel)
    want.mark(T, pts, 0, ov["min_ray_length_m"], 2.0)
    assert _same(a.download(), want.arrays()) and _same(b.download(), want.arrays()) and len(want.arrays()[0]) > 0
    # deintegration (projective only) does not unmark, and does not mark
    player = Layer(hip, voxel, capacity_blocks=8192)
    pinteg = Integrator(hip, player, _cfg(hip, voxel, "projective"), "projective")
    pobs = ObservationHistory(hip, player)
    pinteg.attach_history(pobs)
    pobs.set_frame(3)
    pinteg.integrate_points(T, pts)
    before = pobs.download()
    pobs.set_frame(4)
    pinteg.deintegrate_points(T, pts)
    pinteg.sync()
    after = pobs.download()
    assert len(before[0]) > 0 and _same(before, after)


def _check_encoding(mesh, obs, voxel):
    g = mesh.download()
    h = mesh.history(obs)
    idx, masks = obs.download()
    tm = hr.triangle_masks(g["xyz"], voxel, idx, masks)
    hb, hist, has = hr.encode(tm, g["vertex_begin"])
    assert np.array_equal(h["history_begin"], hb) and np.array_equal(h["history"], hist) and np.array_equal(h["block_has_history"], has)
    runs = h["history"].reshape(-1, 2).astype(np.int64)
    assert np.all(runs[:, 0] <= runs[:, 1]) and np.all(runs < 256)
    same_tri = np.repeat(np.arange(mesh.n_triangles), np.diff(h["history_begin"].astype(np.int64)) // 2)
    inner = same_tri[1:] == same_tri[:-1]
    assert np.all(runs[1:, 0][inner] > runs[:-1, 1][inner] + 1)  # ascending and not adjacent
    return h


@pytest.mark.parametrize("voxel", [0.10, 0.05, 0.02])
def test_mesh_histories_equal_the_reference_encoding(hip, voxel):
    ov, _ = _scene(voxel)
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, _cfg(hip, voxel), "merged")
    obs = ObservationHistory(hip, layer)
    integ.attach_history(obs)
    # ids with gaps and neighbours, across word boundaries, up to the last bit
    ids = [0, 1, 2, 30, 31, 32, 33, 63, 65, 127, 128, 200, 253, 254, 255]
    for k, fid in enumerate(ids):
        T, pts, rgba, _ = synth.make_frame(6 * k)
        obs.set_frame(fid)
        integ.integrate_points(T, pts[::4], rgba[::4])
    mesh = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    assert mesh.n_triangles > 1000
    h = _check_encoding(mesh, obs, voxel)
    assert len(h["history"]) > 2 * mesh.n_triangles // 2 and h["block_has_history"].sum() > 0
    assert h["history"].max() == 255


def _wall_frame(yaw, wall, axis):
    """A 160 x 120 pinhole camera (f = 150) at the origin turned by yaw about z, looking at the plane <axis> = wall."""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    uu, vv = np.meshgrid((np.arange(160) - 79.5) / 150.0, (np.arange(120) - 59.5) / 150.0)
    d = np.stack([uu, vv, np.ones_like(uu)], -1).reshape(-1, 3)
    t = wall / (d @ R.T)[:, axis]
    T = np.concatenate([synth.quat_from_matrix(R), [0.0, 0.0, 0.0]]).astype(np.float32)
    return T, (d * t[:, None]).astype(np.float32)


def test_two_walls_and_a_camera_that_turns(hip):
    """Wall A (x = 2.11 m) is seen by frames 0-4 and 8-9, wall B (y = 2.11 m) by frames 10-19 after a quarter turn; frames 5-7
    look at nothing.  The walls sit in the middle of a cell, so the surface's triangles lie in the cells the points mark."""
    voxel, wall = 0.05, 2.11
    cell = 4 * voxel
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, _cfg(hip, voxel), "merged")
    obs = ObservationHistory(hip, layer)
    integ.attach_history(obs)
    seen = {}
    for fid in range(20):
        obs.set_frame(fid)
        if 5 <= fid <= 7:
            integ.integrate_points(np.array([1, 0, 0, 0, 0, 0, 0], np.float32), np.zeros((0, 3), np.float32))
            continue
        T, pts = _wall_frame(0.0, wall, 0) if fid < 10 else _wall_frame(np.pi / 2, wall, 1)
        integ.integrate_points(T, pts)
        seen["A" if fid < 10 else "B"] = hr.transform_points(T, pts)
    mesh = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    h = _check_encoding(mesh, obs, voxel)
    xyz = mesh.download()["xyz"].reshape(-1, 3, 3)
    hb = h["history_begin"].astype(np.int64)
    runs = [h["history"][hb[t]:hb[t + 1]].tolist() for t in range(mesh.n_triangles)]
    n_inner = {}
    for name, axis, want in (("A", 0, [0, 4, 8, 9]), ("B", 1, [10, 19])):
        on_wall = np.all(np.abs(xyz[:, :, axis] - wall) < voxel, axis=1) & np.all(np.abs(xyz[:, :, 1 - axis]) < 1.5, axis=1)
        assert on_wall.sum() > 1000
        lo, hi = seen[name].min(axis=0) + cell, seen[name].max(axis=0) - cell
        other = [a for a in range(3) if a != axis]
        inner = on_wall & np.all((xyz[:, :, other] >= lo[other]) & (xyz[:, :, other] <= hi[other]), axis=(1, 2))
        n_inner[name] = int(inner.sum())
        assert n_inner[name] > 500
        assert all(runs[t] == want for t in np.flatnonzero(inner))
        for t in np.flatnonzero(on_wall):
            assert all((f >= 10) == (name == "B") for f in runs[t]), (name, runs[t])
    print("triangles well inside the seen areas:", n_inner)


def test_depth_frames_to_recovered_layer(hip):
    """40 frames fused with a history attached -> mesh message with histories and the trajectory -> recover mode's layer: its
    surface lies within a voxel of the original one (the bound of test_mesh_message_feeds_recover_mode), from strictly fewer
    (triangle, frame) pairs than "every frame saw every triangle" integrates."""
    voxel, n = 0.05, 40
    cfg = _cfg(hip, voxel)
    layer = Layer(hip, voxel, capacity_blocks=16384)
    integ = Integrator(hip, layer, cfg, "merged")
    obs = ObservationHistory(hip, layer)
    integ.attach_history(obs)
    traj = []
    for k in range(n):
        T, pts, rgba, _ = synth.make_frame(10 * k)
        obs.set_frame(k)
        integ.integrate_points(T, pts[::2], rgba[::2])
        ns = 950000000 + 50000000 * k
        traj.append((1600000000 + ns // 1000000000, ns % 1000000000, T))
    m = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    original = cKDTree(m.download()["xyz"])
    h = m.history(obs)
    pairs_recorded = int((np.diff(h["history"].reshape(-1, 2).astype(np.int64), axis=1) + 1).sum())
    pairs_all = m.n_triangles * n
    quant = {}
    for name, hist in (("recorded", obs), ("all frames", lambda idx, nt: [[0, n - 1]] * nt)):
        d = m.to_msg("color", history=hist, trajectory=traj)
        fresh = Layer(hip, voxel, capacity_blocks=16384)
        rinteg = Integrator(hip, fresh, cfg, "merged")
        n_points, n_calls = MeshConverter(hip).process_mesh(rinteg, MeshMsg(**d))
        rinteg.sync()
        back = MeshLayer.from_layer(hip, fresh, min_weight=1e-4).download()["xyz"]
        dist, _ = original.query(back)
        quant[name] = (np.quantile(dist, [0.5, 0.95]) / voxel, len(back), n_calls)
        print(f"{name}: recovered surface distance quantiles 50/95 % [voxels] {quant[name][0]}, {len(back)} vertices, {n_calls} integrate calls")
    print(f"(triangle, frame) pairs: recorded {pairs_recorded}, all frames {pairs_all} ({pairs_recorded / pairs_all:.3f})")
    assert 0 < pairs_recorded < pairs_all
    assert 0 < quant["recorded"][2] <= n and quant["recorded"][1] > 0.5 * 3 * m.n_triangles
    assert quant["recorded"][0][1] < 1.0


def test_edges(hip):
    voxel = 0.05
    ov, frames = _scene(voxel)
    lo, hi = ov["min_ray_length_m"], ov["max_ray_length_m"]
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, _cfg(hip, voxel), "merged")
    for T, pts, _ in frames:
        integ.integrate_points(T, pts)
    mesh = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    # empty record, n = 0: every range empty, every flag 0
    obs = ObservationHistory(hip, layer, 4096)
    obs.record(frames[0][0], np.zeros((0, 3), np.float32), lo, hi)
    obs.record_dev(frames[0][0], 0, lo, hi, n=0)
    h = mesh.history(obs)
    assert not h["history_begin"].any() and len(h["history_begin"]) == mesh.n_triangles + 1 and len(h["history"]) == 0 and not h["block_has_history"].any()
    assert all(b.get("history") is None for b in mesh.to_msg(history=obs)["blocks"])
    # frame ids: 255 is the last one, 256 is refused and the id in use stays
    obs.set_frame(255)
    with pytest.raises(CoxError) as e:
        obs.set_frame(256)
    assert e.value.status == -5
    obs.record(*frames[0][:2], lo, hi)
    idx, masks = obs.download()
    assert len(idx) > 0 and np.all(masks[..., :7] == 0) and np.all((masks[..., 7] == 0) | (masks[..., 7] == 1 << 31))
    # clear
    obs.clear()
    assert obs.download()[0].shape == (0, 3) and obs.stats()["marked_cells"] == 0
    # growth past the initial capacity gives the bits of a large initial capacity
    want = _reference(voxel, ov, frames)
    small, big = ObservationHistory(hip, layer, 4), ObservationHistory(hip, layer, 8192)
    for T, pts, fid in frames:
        small.set_frame(fid), big.set_frame(fid)
        small.record(T, pts, lo, hi), big.record(T, pts, lo, hi)
    small.sync(), big.sync()
    assert len(want[0]) > 4 and _same(small.download(), want) and _same(big.download(), want)
    assert np.array_equal(mesh.history(small)["history"], mesh.history(big)["history"])
    # auto-grow off: a status code, no fault, and what fitted is there
    fixed = ObservationHistory(hip, layer, 4)
    fixed.set_auto_grow(False)
    for T, pts, fid in frames:
        fixed.set_frame(fid)
        fixed.record(T, pts, lo, hi)
    with pytest.raises(CoxError) as e:
        fixed.sync()
    assert e.value.status == -4
    fixed.sync()  # reported once
    got = fixed.download()
    assert len(got[0]) == 4 and fixed.stats()["blocks"] == 4
    ref = {tuple(b): m for b, m in zip(want[0].tolist(), want[1])}
    assert all(tuple(b) in ref and np.all((m & ~ref[tuple(b)]) == 0) for b, m in zip(got[0].tolist(), got[1]))
    # a mesh that has left the layer's frame is refused; one of another voxel size too
    moved = MeshLayer.from_layer(hip, layer, min_weight=1e-4)
    moved.transform(np.array([1, 0, 0, 0, 0.5, 0, 0], np.float32))
    with pytest.raises(CoxError) as e:
        moved.history(big)
    assert e.value.status == -1
    other = Layer(hip, 0.10, capacity_blocks=64)
    with pytest.raises(CoxError) as e:
        Integrator(hip, other, _cfg(hip, 0.10), "merged").attach_history(big)
    assert e.value.status == -1


def test_cpp_history_flow_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "history_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "history_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "history smoke ok" in out.stdout
