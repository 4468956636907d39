"""The input side of a frame (cox_frontend.hpp, cox_integrator.hip), at its edges: the depth front end, the kernel that reads pinned
host inputs, and the point count that stays on the device.  References: tests/frontend_ref.py; cases: tests/frontend_cases.py.

Directly, through the entries of include/coxgraph_hip_selftest.h, every comparison exact:

  * k_depth_count / k_depth_points: points, colours, tile sums and the count equal the reference for images below one 8-pixel
    strip, below, at and above one tile, with a partial last tile, with every kind of invalid value, a denormal and a huge depth,
    with and without a colour image, and with grids smaller than the tile count (the tile loops); nothing at or beyond the count is
    written, nor the guards behind the arrays
  * k_copy_from_host: destinations equal sources for every tail, for no whole 16 bytes, around one and four loads per lane
    (the 4-deep loop's exit, the remainder loop), for three grid sizes, without a second segment and with a shorter and a longer one

Through the integrator, against the point path fed the reference's points (layers equal word for word, last_stats() equal):

  * depth frames whose valid count straddles what the by-value upper bound does not: np2, the mixed order's group count, the
    head and sort tiles -- a stage that takes n_points or np2 from the bound, not from the patched block, fails here
  * COX_GRAPH=1, COX_DEPTH_CONVERT=input, COX_INPUT_STREAM=0, no colour image; a stream whose image size changes
  * cox_integrate_points_async from pinned memory through the copy kernel: odd counts, two grid sizes, a source that is not
    16-byte aligned (the copy engine takes over), with and without colours
"""
import numpy as np
import pytest

from coxgraph_amd import synth
from coxgraph_amd.capi import Integrator, Layer

import frontend_cases as fc
import frontend_ref as fr
from frontend_cases import SENTINEL, U32

pytestmark = pytest.mark.gpu

METHODS = ("merged", "fast", "simple")


# ---- directly: the depth front end ---------------------------------------------------------------------------------------------------
def check_depth(hip, w, h, pattern, colour, grid=0):
    """One image through the entry against the reference; colour: "image", "none" (no colour image: colours are 0), "unwanted"
    (no colour output: the array is left alone).  -> False where the pattern does not exist at this size."""
    mask = fc.valid_mask(pattern, w * h, seed=w)
    if mask is None:
        return False
    depth, K = fc.depth_image(w, h, mask, seed=h), fc.intrinsics(w, h)
    rgba = None if colour == "none" else fc.colour_image(w, h)
    xyz, colours, tile_sums, n = fr.depth_to_points(depth, rgba, K)
    r = fc.run_depth_points(hip, depth, rgba, K, grid=grid, want_rgba=colour != "unwanted")
    what = (w, h, pattern, colour, grid)
    assert r.status == 0, what
    assert r.n == n == int(mask.sum()), what
    assert np.array_equal(r.tile_sums, tile_sums), what
    assert np.array_equal(r.xyz[:n], xyz.view(U32)), what
    assert bool(np.all(r.xyz[n:] == SENTINEL)), what
    if colour == "unwanted":
        assert bool(np.all(r.rgba == SENTINEL)), what
    else:
        assert np.array_equal(r.rgba[:n], colours.view(U32).reshape(-1)), what
        assert bool(np.all(r.rgba[n:] == SENTINEL)), what
    assert r.guard_touched == [0, 0, 0], what
    return True


@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_depth_points_equal_the_reference(hip, w, h):
    ran = [p for p in fc.PATTERNS for colour in ("image", "none", "unwanted") if check_depth(hip, w, h, p, colour)]
    assert set(ran) >= {"all", "none", "first", "last", "random"}
    assert ("tile_edge" in ran) == (w * h > 2048) and ("tile_hole" in ran) == ((w, h) == (6145, 1))


@pytest.mark.parametrize("grid", fc.GRIDS)
@pytest.mark.parametrize("w,h", fc.STRIDED_SHAPES)
def test_depth_points_with_fewer_workgroups_than_tiles(hip, w, h, grid):
    """grid 1 and 2 on 4 and 3 tiles: one workgroup converts several tiles, through the same LDS words."""
    assert fr.depth_tiles(w * h) > max(fc.GRIDS)
    for pattern in fc.PATTERNS:
        for colour in ("image", "none"):
            check_depth(hip, w, h, pattern, colour, grid=grid)


def test_depth_entry_refuses_what_it_cannot_run(hip):
    d, K = fc.depth_image(9, 1, fc.valid_mask("all", 9)), fc.intrinsics(9, 1)
    assert fc.run_depth_points(hip, d, None, K, grid=65536).status == -1
    assert fc.run_depth_points(hip, d, None, K, device=99).status == fc.NO_DEVICE
    assert fc.run_copy(hip, fc.seeded_words(5, 0), None, 0)[0] == -1
    assert fc.run_copy(hip, fc.seeded_words(5, 0), None, 1025)[0] == -1


# ---- directly: the copy kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", fc.COPY_GROUPS)
def test_copy_kernel_equals_its_sources(hip, groups):
    for words_a in fc.copy_sizes(groups):
        a = fc.seeded_words(words_a, seed=groups)
        assert fr.host_segment(4 * words_a) == (words_a // 4, words_a % 4)
        for words_b in fc.second_sizes(words_a, groups):
            b = None if words_b is None else fc.seeded_words(words_b, seed=groups + 100)
            st, out_a, out_b, guard = fc.run_copy(hip, a, b, groups)
            what = (groups, words_a, words_b)
            assert st == 0, what
            assert np.array_equal(out_a, fr.copy_words(a)), what
            if b is not None:
                assert np.array_equal(out_b, fr.copy_words(b)), what
            assert guard == [0, 0], what


# ---- through the integrator ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """The wavy wall seen from the first pose of the synthetic trajectory, and seeded colours."""
    w, h = fc.SCENE_WH
    return synth.make_frame(0)[0], fc.scene_depth(w, h), fc.colour_image(w, h, seed=9)


def make_pair(hip, monkeypatch, method, env):
    """(layer, integrator) twice: the one under test, created under `env`, and the one that takes the point path, created without."""
    cfg = hip.default_config(integrator_threads=1, **synth.integrator_overrides(0.05))
    lb = Layer(hip, 0.05, capacity_blocks=4096)
    ib = Integrator(hip, lb, cfg, method)
    for name, value in env.items():
        monkeypatch.setenv(name, value)  # (read when the integrator is created)
    la = Layer(hip, 0.05, capacity_blocks=4096)
    ia = Integrator(hip, la, cfg, method)
    return la, ia, lb, ib


def assert_same(la, ia, lb, ib):
    sa, sb = ia.last_stats(), ib.last_stats()
    assert sa == sb, (sa, sb)
    ja, va = la.download()
    jb, vb = lb.download()
    assert len(ja) > 0 and np.array_equal(ja, jb) and np.array_equal(va, vb)


def run_depth_stream(T, frames, ia, ib, colour=True, entries=("dev", "async")):
    """frames: (depth [h, w], rgba [w h, 4], K).  All of them through the depth entries of ia, one after the other without a sync
    between them, device and host images in turn; then the reference's points through the point path of ib."""
    import torch
    on_device = [(torch.from_numpy(depth).cuda(), torch.from_numpy(rgba).cuda()) if entries[t % len(entries)] == "dev" else None
                 for t, (depth, rgba, _) in enumerate(frames)]
    torch.cuda.synchronize()  # (the uploads: the engine's streams do not wait for torch's)
    for (depth, rgba, K), dev in zip(frames, on_device):
        h, w = depth.shape
        if dev:
            ia.integrate_depth_dev(T, dev[0].data_ptr(), dev[1].data_ptr() if colour else 0, w, h, K)
        else:
            ia.integrate_depth_async(T, depth.ctypes.data, rgba.ctypes.data if colour else 0, w, h, K)
    ia.wait_inputs()
    ia.sync()
    for depth, rgba, K in frames:
        xyz, colours, _, _ = fr.depth_to_points(depth, rgba if colour else None, K)
        ib.integrate_points(T, xyz, colours)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("V", fc.VALID_COUNTS)
def test_depth_frames_with_the_count_on_the_device(hip, monkeypatch, scene, method, V):
    """Four frames back to back: V valid pixels as a device image, V others as host images, the whole image, V again.  The upper
    bound every kernel is launched for is 4757 throughout."""
    T, depth, rgba = scene
    frames = [(fc.with_valid_count(depth, V, 1), rgba, fc.SCENE_K), (fc.with_valid_count(depth, V, 2), rgba, fc.SCENE_K), (depth, rgba, fc.SCENE_K),
              (fc.with_valid_count(depth, V, 3), rgba, fc.SCENE_K)]
    la, ia, lb, ib = make_pair(hip, monkeypatch, method, {})
    run_depth_stream(T, frames, ia, ib)
    assert ia.last_stats()["n_points"] == V  # fetched from the device
    assert_same(la, ia, lb, ib)


VARIANTS = {"graph": dict(env={"COX_GRAPH": "1"}), "convert_on_input_stream": dict(env={"COX_DEPTH_CONVERT": "input"}, entries=("async",)),
            "no_input_stream": dict(env={"COX_INPUT_STREAM": "0"}), "no_colour_image": dict(colour=False)}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_depth_stream_of_every_count_under_the_switches(hip, monkeypatch, scene, method, variant):
    """Every valid count in one stream (in an order that moves np2 and the group count up and down), under each switch that
    changes where the conversion runs or how the frame's first stage is enqueued, and without a colour image (both entries)."""
    T, depth, rgba = scene
    v = VARIANTS[variant]
    order = np.random.default_rng(4).permutation(len(fc.VALID_COUNTS))
    frames = [(fc.with_valid_count(depth, fc.VALID_COUNTS[k], 10 + int(k)), rgba, fc.SCENE_K) for k in order]
    la, ia, lb, ib = make_pair(hip, monkeypatch, method, v.get("env", {}))
    run_depth_stream(T, frames, ia, ib, colour=v.get("colour", True), entries=v.get("entries", ("dev", "async")))
    assert_same(la, ia, lb, ib)


@pytest.mark.parametrize("method", METHODS)
def test_depth_stream_whose_image_size_changes(hip, monkeypatch, scene, method):
    """2048, 4757, 9, 2049, 2048 pixels in flight on one integrator: the buffers grow twice, then larger staging sets are reused
    with smaller counts and other tile counts."""
    T = scene[0]
    frames = []
    for t, (w, h) in enumerate(fc.STREAM_SHAPES):
        mask = np.random.default_rng([5, t]).random(w * h) < 0.9
        d = fc.scene_depth(w, h).reshape(-1)
        d[~mask] = fc.INVALID[np.arange(int((~mask).sum())) % len(fc.INVALID)]
        frames.append((d.reshape(h, w), fc.colour_image(w, h, seed=t), fc.scene_intrinsics(w, h)))
    la, ia, lb, ib = make_pair(hip, monkeypatch, method, {})
    run_depth_stream(T, frames, ia, ib)
    assert_same(la, ia, lb, ib)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("colour", [True, False])
@pytest.mark.parametrize("offset_words", [0, 1])
@pytest.mark.parametrize("groups", [1, 8])
def test_pinned_clouds_through_the_copy_kernel(hip, monkeypatch, scene, method, groups, offset_words, colour):
    """cox_integrate_points_async from pinned memory with COX_H2D=kernel: 12 n and 4 n bytes have tails of 1 to 3 words and, for
    n <= 3, not one whole 16 bytes.  A source 4 bytes off a 16-byte boundary goes to the copy engine instead."""
    import torch
    T, depth, rgba = scene
    xyz, colours, _, n_all = fr.depth_to_points(depth, rgba, fc.SCENE_K)
    assert n_all == max(fc.ASYNC_COUNTS)
    la, ia, lb, ib = make_pair(hip, monkeypatch, method, {"COX_H2D": "kernel", "COX_H2D_GROUPS": str(groups)})
    clouds, keep = [], []
    for n in fc.ASYNC_COUNTS:
        pick = np.sort(np.random.default_rng([6, n]).permutation(n_all)[:n])
        p, c = np.ascontiguousarray(xyz[pick]), np.ascontiguousarray(colours[pick])
        clouds.append((p, c if colour else None))
        hp, hc = torch.empty(3 * n + 4, dtype=torch.float32).pin_memory(), torch.empty(4 * n + 16, dtype=torch.uint8).pin_memory()
        assert hp.data_ptr() % 16 == 0 and hc.data_ptr() % 16 == 0
        hp[offset_words:offset_words + 3 * n] = torch.from_numpy(p.reshape(-1))
        hc[4 * offset_words:4 * offset_words + 4 * n] = torch.from_numpy(c.reshape(-1))
        keep.append((hp, hc))
        ia.integrate_points_async(T, hp.data_ptr() + 4 * offset_words, hc.data_ptr() + 4 * offset_words if colour else 0, n)
    ia.wait_inputs()
    ia.sync()
    for p, c in clouds:
        ib.integrate_points(T, p, c)
    assert_same(la, ia, lb, ib)
