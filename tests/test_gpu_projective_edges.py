"""The projective integrator where its two kernels are not the whole story: a pool that is too small (with and without
auto-grow), more frames in flight than its event ring holds, empty frames, and layers that other integrators write too.
Every expectation is the CPU oracle run sequentially in call order, compared bit for bit.

What happens to a frame that finds no free pool block (pinned here): it is ALL OR NOTHING.  The device drops it, and every
frame queued behind it, whole; with auto-grow the host doubles the pool and enqueues them again, in order, and the caller sees
COX_OK; without auto-grow they stay dropped, the call that notices (the frame's own call on the host path, a later call or
sync() on the device path) returns the pool error, and the layer is exactly what it was before the dropped frame.
"""
import numpy as np
import pytest

from coxgraph_amd import synth
from coxgraph_amd.capi import Layer, Integrator, CoxError
from util import compare_layers
from test_oracle_projective import lidar_cloud, proj_config, IDENT
from test_gpu_projective import KEYS

pytestmark = pytest.mark.gpu

POSE = np.array([0.9990482, 0, 0, 0.0436194, 0.2, -0.1, 0.05], np.float32)
CAMERA = dict(sensor_horizontal_resolution=1280, sensor_vertical_resolution=960, sensor_vertical_field_of_view_degrees=360.0)


def oracle_run(oracle, voxel, frames, **cfg_kw):
    layer = Layer(oracle, voxel)
    integ = Integrator(oracle, layer, proj_config(oracle, **cfg_kw), "projective")
    stats = []
    for T, p in frames:
        integ.integrate_points(T, p, None)
        stats.append(integ.last_stats())
    return layer, stats


def assert_same(la, lb, min_observed=1000):
    rep = compare_layers(la, lb, tol=0.0, check_color=False)
    assert rep["bitexact_d"] and rep["bitexact_w"] and rep["observed"] >= min_observed, rep
    return rep


def assert_stats(a, b):
    for k in KEYS:
        assert a[k] == b[k], (k, a[k], b[k])


def to_device(frames):
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for _, p in frames]
    torch.cuda.synchronize()
    return dev


@pytest.mark.parametrize("path", ["host", "device"])
def test_first_frame_needs_far_more_blocks_than_the_pool_holds(hip, oracle, path):
    """8 blocks of pool, a first frame that needs hundreds: nothing to predict the growth from.  Then a far wall appears: a later
    frame that alone more than doubles the block count."""
    voxel = 0.05
    frames = [(IDENT, lidar_cloud(wall_x=1.0)), (POSE, lidar_cloud(wall_x=1.1)), (IDENT, lidar_cloud(wall_x=6.0)), (POSE, lidar_cloud(wall_x=5.8))]
    kw = dict(default_truncation_distance=0.15)
    lb, sb = oracle_run(oracle, voxel, frames, **kw)
    assert sb[0]["n_new_blocks"] > 6 * 8 and sb[2]["n_new_blocks"] > 2 * (sb[0]["n_new_blocks"] + sb[1]["n_new_blocks"])
    layer = Layer(hip, voxel, capacity_blocks=8)
    integ = Integrator(hip, layer, proj_config(hip, **kw), "projective")
    if path == "host":
        for (T, p), want in zip(frames, sb):
            integ.integrate_points(T, p, None)  # status OK: raises otherwise
            assert_stats(integ.last_stats(), want)
    else:
        dev = to_device(frames)
        for (T, _), x in zip(frames, dev):
            integ.integrate_points_dev(T, x.data_ptr(), 0, x.shape[0])
        integ.sync()
        assert_stats(integ.last_stats(), sb[-1])
    assert_same(layer, lb)
    assert layer.capacity() >= layer.stats()[0] > 500


def unique_blocks(layer):
    idx, _ = layer.download()
    assert len(np.unique(idx, axis=0)) == len(idx) == layer.stats()[0]
    return len(idx)


@pytest.mark.parametrize("path", ["host", "device"])
def test_without_auto_grow_the_frame_is_dropped_whole_and_the_integrator_goes_on_after_reserve(hip, oracle, path):
    voxel = 0.1
    small, big = (IDENT, lidar_cloud(wall_x=1.0)), (POSE, lidar_cloud(wall_x=6.0))
    after = [(IDENT, lidar_cloud(wall_x=5.5)), (POSE, lidar_cloud(wall_x=1.2))]
    l1, s1 = oracle_run(oracle, voxel, [small])
    n_small = s1[0]["n_new_blocks"]
    l_all, s_all = oracle_run(oracle, voxel, [small] + after)   # the dropped frame never happened
    layer = Layer(hip, voxel, capacity_blocks=n_small + 20)
    layer.set_auto_grow(False)
    integ = Integrator(hip, layer, proj_config(hip), "projective")
    integ.integrate_points(*small, None)
    assert_stats(integ.last_stats(), s1[0])
    with pytest.raises(CoxError):
        if path == "host":
            integ.integrate_points(*big, None)
        else:
            dev = to_device([big])
            integ.integrate_points_dev(big[0], dev[0].data_ptr(), 0, dev[0].shape[0])
            integ.sync()
    # dropped whole: neither its values nor its blocks are in the layer
    assert_same(layer, l1)
    assert unique_blocks(layer) == n_small
    integ.sync()  # the error has been reported once; the integrator is usable
    layer.reserve(4096)
    if path == "host":
        for (T, p), want in zip(after, s_all[1:]):
            integ.integrate_points(T, p, None)
            assert_stats(integ.last_stats(), want)
    else:
        dev = to_device(after)
        for (T, _), x in zip(after, dev):
            integ.integrate_points_dev(T, x.data_ptr(), 0, x.shape[0])
        integ.sync()
        assert_stats(integ.last_stats(), s_all[-1])
    assert_same(layer, l_all)
    unique_blocks(layer)


def test_ten_frames_in_flight_and_empty_frames_on_the_device_path(hip, oracle):
    """The event ring holds four frames: ten are issued without a sync.  Then empty clouds between full ones: last_stats() is
    always the last frame's."""
    import torch
    voxel = 0.1
    frames = [synth.make_frame(t)[:2] for t in range(0, 50, 5)]
    frames = [(T, np.ascontiguousarray(p[::3])) for T, p in frames]
    ov = synth.integrator_overrides(voxel)
    kw = dict(CAMERA, default_truncation_distance=ov["default_truncation_distance"], min_ray_length_m=ov["min_ray_length_m"], max_ray_length_m=ov["max_ray_length_m"])
    lb, sb = oracle_run(oracle, voxel, frames, **kw)
    layer = Layer(hip, voxel, capacity_blocks=64)
    integ = Integrator(hip, layer, proj_config(hip, **kw), "projective")
    dev = to_device(frames)
    for (T, _), x in zip(frames, dev):
        integ.integrate_points_dev(T, x.data_ptr(), 0, x.shape[0])
    integ.sync()
    assert_stats(integ.last_stats(), sb[-1])
    assert_same(layer, lb)
    # full, empty, full, empty: the oracle through its host entry point with the same clouds
    empty = torch.zeros((1, 3), device="cuda")
    ob = Integrator(oracle, lb, proj_config(oracle, **kw), "projective")
    for k in (0, None, 3, None, None, 7):
        if k is None:
            integ.integrate_points_dev(IDENT, empty.data_ptr(), 0, 0)
            ob.integrate_points(IDENT, np.zeros((0, 3), np.float32), None)
        else:
            integ.integrate_points_dev(frames[k][0], dev[k].data_ptr(), 0, dev[k].shape[0])
            ob.integrate_points(*frames[k], None)
        got, want = integ.last_stats(), ob.last_stats()
        assert_stats(got, want)
        assert (got["n_updates"] > 0) == (k is not None)
    integ.sync()
    assert_same(layer, lb)


def _merged_cfg(eng, voxel):
    return eng.default_config(**synth.integrator_overrides(voxel))


@pytest.mark.parametrize("first", ["merged", "projective"])
def test_projective_and_merged_share_a_layer_from_the_very_first_frame(hip, oracle, first):
    """The merged integrator's frames go through integrate_points_async (its submission thread enqueues them); a projective frame
    follows immediately.  Frames of different integrators must reach the layer in call order -- also when the other integrator's
    very first frame on a fresh layer has not been enqueued yet.  The two-frame opening ten times on fresh layers (a host-side
    race: repetition of an operation that passes), then a longer alternation."""
    import torch
    voxel = 0.1
    ov = synth.integrator_overrides(voxel)
    kw = dict(CAMERA, default_truncation_distance=ov["default_truncation_distance"], min_ray_length_m=ov["min_ray_length_m"], max_ray_length_m=ov["max_ray_length_m"])
    frames = [synth.make_frame(t)[:3] for t in (0, 6, 12, 18, 24, 30)]
    frames = [(T, np.ascontiguousarray(p[::2]), np.ascontiguousarray(c[::2])) for T, p, c in frames]
    pinned = [(torch.from_numpy(p).pin_memory(), torch.from_numpy(c).pin_memory()) for _, p, c in frames]
    dev = to_device([(T, p) for T, p, _ in frames])

    def run_oracle(n):
        layer = Layer(oracle, voxel)
        im, ip = Integrator(oracle, layer, _merged_cfg(oracle, voxel), "merged"), Integrator(oracle, layer, proj_config(oracle, **kw), "projective")
        for k in range(n):
            T, p, c = frames[k]
            if (k % 2 == 0) == (first == "merged"):
                im.integrate_points(T, p, c)
            else:
                ip.integrate_points(T, p, None)
        return layer

    def run_hip(n):
        layer = Layer(hip, voxel, capacity_blocks=4096)
        im, ip = Integrator(hip, layer, _merged_cfg(hip, voxel), "merged"), Integrator(hip, layer, proj_config(hip, **kw), "projective")
        for k in range(n):
            T = frames[k][0]
            if (k % 2 == 0) == (first == "merged"):
                im.integrate_points_async(T, pinned[k][0].data_ptr(), pinned[k][1].data_ptr(), pinned[k][0].shape[0])
            else:
                ip.integrate_points_dev(T, dev[k].data_ptr(), 0, dev[k].shape[0])
        im.wait_inputs()
        im.sync()
        ip.sync()
        return layer, im, ip

    want2, want6 = run_oracle(2), run_oracle(6)
    for rep in range(10):
        layer, im, ip = run_hip(2)
        r = compare_layers(layer, want2, tol=0.0, check_color=True)
        assert r["bitexact_d"] and r["bitexact_w"] and r["n_diff_color"] == 0 and r["observed"] > 1000, (rep, r)
        im.close(), ip.close(), layer.close()
    layer, im, ip = run_hip(6)
    r = compare_layers(layer, want6, tol=0.0, check_color=True)
    assert r["bitexact_d"] and r["bitexact_w"] and r["n_diff_color"] == 0 and r["observed"] > 1000, r


def test_two_projective_integrators_with_different_sensor_models_share_a_layer(hip, oracle):
    """Alternating, a pool of 16 blocks that every one of the first frames overflows, no host-side wait between the two."""
    voxel = 0.1
    clouds = [(IDENT, lidar_cloud()), (POSE, lidar_cloud(wall_x=2.8)), (IDENT, lidar_cloud(wall_x=3.3)), (POSE, lidar_cloud(wall_x=5.5))]
    out = []
    for eng in (hip, oracle):
        layer = Layer(eng, voxel, capacity_blocks=16)
        a = Integrator(eng, layer, proj_config(eng), "projective")
        b = Integrator(eng, layer, proj_config(eng, projective_interpolation_scheme=2, **CAMERA), "projective")
        stats = []
        dev = to_device(clouds) if eng is hip else None
        for k, (T, p) in enumerate(clouds):
            integ = a if k % 2 == 0 else b
            if eng is hip:
                integ.integrate_points_dev(T, dev[k].data_ptr(), 0, dev[k].shape[0])
            else:
                integ.integrate_points(T, p, None)
                stats.append(integ.last_stats())
        if eng is hip:
            a.sync(), b.sync()
        out.append((layer, stats, a, b))
    assert out[1][1][0]["n_new_blocks"] > 16
    assert_stats(out[0][2].last_stats(), out[1][1][2])
    assert_stats(out[0][3].last_stats(), out[1][1][3])
    assert_same(out[0][0], out[1][0])


@pytest.mark.parametrize("first", ["projective", "merged"])
def test_a_projective_frame_that_overflows_is_on_the_layer_before_the_next_writers_frame(hip, oracle, first):
    """Auto-grow on.  A projective frame runs out of pool on the device and is redone by the host; a merged frame on the same
    region is issued immediately behind it through integrate_points_async.  The merged frame must find the projective frame
    complete (not its half-allocated blocks), and nothing it writes may be rolled back with the dropped frame.
    projective first: a pool of 8 blocks, which the very first frame overflows.  merged first: a pool that the merged
    integrator's first frame just fits in (the ray casters do not redo an asynchronous frame) and the projective frame behind it
    does not -- unless the projective integrator already sees the merged frame's block count and grows the pool beforehand."""
    import torch
    voxel = 0.05
    ov = synth.integrator_overrides(voxel)
    kw = dict(CAMERA, default_truncation_distance=ov["default_truncation_distance"], min_ray_length_m=ov["min_ray_length_m"], max_ray_length_m=ov["max_ray_length_m"])
    times, capacity = ((0, 3, 40, 43, 80, 83), 8) if first == "projective" else ((0, 40, 43, 80, 83), 48)
    frames = [synth.make_frame(t)[:3] for t in times]   # the camera moves on: new blocks again and again
    frames = [(T, np.ascontiguousarray(p[::2]), np.ascontiguousarray(c[::2])) for T, p, c in frames]
    pinned = [(torch.from_numpy(p).pin_memory(), torch.from_numpy(c).pin_memory()) for _, p, c in frames]
    dev = to_device([(T, p) for T, p, _ in frames])
    layers = []
    for eng in (hip, oracle):
        layer = Layer(eng, voxel, capacity_blocks=capacity)
        im, ip = Integrator(eng, layer, _merged_cfg(eng, voxel), "merged"), Integrator(eng, layer, proj_config(eng, **kw), "projective")
        new_blocks = []
        for k, (T, p, c) in enumerate(frames):
            projective = (k % 2 == 0) == (first == "projective")
            if eng is oracle:
                (ip.integrate_points(T, p, None) if projective else im.integrate_points(T, p, c))
                new_blocks.append((ip if projective else im).last_stats()["n_new_blocks"])
            elif projective:
                ip.integrate_points_dev(T, dev[k].data_ptr(), 0, dev[k].shape[0])
            else:
                im.integrate_points_async(T, pinned[k][0].data_ptr(), pinned[k][1].data_ptr(), pinned[k][0].shape[0])
        if eng is hip:
            im.wait_inputs()
            im.sync()
            ip.sync()
        else:
            assert (new_blocks[0] > capacity) if first == "projective" else (new_blocks[0] <= capacity < new_blocks[0] + new_blocks[1]), new_blocks
        layers.append((layer, im, ip))
    r = compare_layers(layers[0][0], layers[1][0], tol=0.0, check_color=True)
    assert r["bitexact_d"] and r["bitexact_w"] and r["n_diff_color"] == 0 and r["observed"] > 1000, r
    unique_blocks(layers[0][0])


def test_invalid_sensor_models_are_refused_and_handles_do_not_leak(hip):
    import torch
    layer = Layer(hip, 0.1, capacity_blocks=64)
    for bad in (dict(sensor_horizontal_resolution=32768, sensor_vertical_resolution=8193),  # rows * cols > 2^28
                dict(projective_interpolation_scheme=4), dict(projective_interpolation_scheme=-1),
                dict(sensor_vertical_field_of_view_degrees=0.0)):
        with pytest.raises(CoxError):
            Integrator(hip, layer, proj_config(hip, **bad), "projective")
    rows, cols = 64, 1024
    free = {}
    for it in range(1, 201):
        integ = Integrator(hip, layer, proj_config(hip), "projective")
        integ.close()
        if it in (20, 200):
            torch.cuda.synchronize()
            free[it] = torch.cuda.mem_get_info()[0]
    # steady state against steady state; one range image of slack for the granularity of the runtime's allocator
    assert free[200] >= free[20] - 4 * rows * cols, free
