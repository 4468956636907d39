"""The ray walk done by the bundle merge (k_bundle_merge<true>, IntegratorPlan::touch_in_merge, coxgraph_amd/csrc/cox_raygen.hpp): the
xyz wave of a bundle walks the ray it has just written, parks the path in the ray's own slot of the spare sort buffer and touches the
frame block table; k_emit_wave reads the slot.  Every case runs with COX_TOUCH=merge and with COX_TOUCH=kernel (the k_touch_wave launch
behind the record-offset scan) under COX_WALK=raygen and is compared with the CPU oracle: distance, weight and colour bit-equal, the
frame statistics equal.  Frames go in through the asynchronous device path, none waited for, so the record sets -- which the merge
now writes -- are reused while their previous users are in flight.  The hand-made clouds are designed and checked in walk_cases.py."""
import numpy as np
import pytest

import walk_cases as wc
from coxgraph_amd import synth
from coxgraph_amd.capi import Layer, Integrator, CoxError
from util import compare_stats
from test_gpu_walk_placement import _assert_equal, _blocks, _feed, _frames, _hip_async, _oracle_run, _to_device

pytestmark = pytest.mark.gpu

TOUCHES = ("merge", "kernel")
COX_ERR_INDEX_RANGE, COX_ERR_INTERNAL = -5, -8
_cache = {}


def _env(touch, **extra):
    return dict(COX_WALK="raygen", COX_TOUCH=touch, **extra)


def _stream(voxel):
    """8 frames of the subsampled synthetic stream: every one of the three record sets is used at least twice."""
    return _frames(voxel, 3 if voxel < 0.07 else 9, n=8)


# ---- 1-3: the synthetic stream, asynchronous ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel", [0.05, 0.10])
@pytest.mark.parametrize("touch", TOUCHES)
def test_asynchronous_stream_equals_the_oracle(hip, oracle, monkeypatch, touch, voxel):
    clouds = _stream(voxel)
    lb, sb = _oracle_run(oracle, ("wim stream", voxel), voxel, clouds)
    la, _, sa = _hip_async(hip, monkeypatch, _env(touch), voxel, clouds)
    _assert_equal(la, lb, sa, sb[-1])


@pytest.mark.parametrize("touch", TOUCHES)
def test_submission_on_the_callers_thread(hip, oracle, monkeypatch, touch):
    clouds = _stream(0.05)
    lb, sb = _oracle_run(oracle, ("wim stream", 0.05), 0.05, clouds)
    la, _, sa = _hip_async(hip, monkeypatch, _env(touch, COX_SUBMIT_THREAD="0"), 0.05, clouds)
    _assert_equal(la, lb, sa, sb[-1])


@pytest.mark.parametrize("walk", ["raygen", None])
@pytest.mark.parametrize("queues", ["4", "16"])
@pytest.mark.parametrize("touch", TOUCHES)
def test_queue_budgets(hip, oracle, monkeypatch, touch, queues, walk):
    """Four queues: the walk is on the lanes by the rule.  Sixteen: by the rule it is in stage T, where COX_TOUCH changes nothing
    (walk None), and on the lanes beside a stream each for T R and U when COX_WALK asks for it."""
    clouds = _stream(0.05)
    lb, sb = _oracle_run(oracle, ("wim stream", 0.05), 0.05, clouds)
    env = dict(COX_TOUCH=touch, COX_QUEUES=queues)
    if walk:
        env["COX_WALK"] = walk
    la, _, sa = _hip_async(hip, monkeypatch, env, 0.05, clouds)
    _assert_equal(la, lb, sa, sb[-1])


# ---- 4-6: hand-made bundles ------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200]  # chunk edges of the merge loop, behind which the walk reuses the wave's LDS


def _handmade(oracle, key, bundles, seed, frames=2):
    """The cloud of `bundles` [(size, steps)], `frames` times in a row (new blocks, then known ones), and the oracle's result; the
    oracle's statistics must show the design: one ray per bundle, the largest bundle, one record per step."""
    if key not in _cache:
        pts, rgba, _ = wc.bundle_cloud(bundles, seed)
        _cache[key] = [(wc.POSE, pts, rgba)] * frames
    clouds = _cache[key]
    lb, sb = _oracle_run(oracle, ("wim", key), wc.VOXEL, clouds, capacity_blocks=4096, cfg_overrides=wc.CFG)
    for s in sb:
        assert s["n_rays"] == len(bundles) and s["max_bundle_points"] == max(n for n, _ in bundles) and s["n_valid"] == sum(n for n, _ in bundles)
        assert s["n_updates"] == sum(st for _, st in bundles)  # (no anti-grazing, storage for every block: every record is an update)
    return clouds, lb, sb


@pytest.mark.parametrize("grid", [None, "1"], ids=["grid_default", "grid_1"])
@pytest.mark.parametrize("touch", TOUCHES)
def test_bundle_sizes_at_the_chunk_edges(hip, oracle, monkeypatch, touch, grid):
    """Bundles of 1 ... 200 points with rays of 21 ... 101 steps; with COX_GRID_MERGE=1 one workgroup takes all tasks in turn, so what
    a walk leaves in a wave's LDS meets the operand table of that wave's next bundle."""
    bundles = [(n, 21 + 10 * j) for j, n in enumerate(SIZES)]
    clouds, lb, sb = _handmade(oracle, "sizes", bundles, seed=5)
    env = _env(touch, **({"COX_GRID_MERGE": grid} if grid else {}))
    la, _, sa = _hip_async(hip, monkeypatch, env, wc.VOXEL, clouds, capacity_blocks=4096, cfg_overrides=wc.CFG)
    _assert_equal(la, lb, sa, sb[-1])


@pytest.mark.parametrize("touch", TOUCHES)
def test_step_counts_at_the_round_edges(hip, oracle, monkeypatch, touch):
    """Rays of 1, 2, 63, 64, 65, 127, 128, 129 steps and the longest the configuration allows (a diagonal ray of max_ray_length_m, 172
    steps: the bound steps_max = 310 that sizes a path slot assumes the full range on all three axes at once, which no ray has): the
    walk's rounds of 64 and the carry of the touch rule between them, behind bundles of every size of the list."""
    longest = wc.longest_steps()
    assert 129 < longest <= 3 * 103 + 1
    steps = [1, 2, 63, 64, 65, 127, 128, 129, longest]
    bundles = list(zip(SIZES[::-1], steps))
    clouds, lb, sb = _handmade(oracle, "steps", bundles, seed=6)
    la, _, sa = _hip_async(hip, monkeypatch, _env(touch), wc.VOXEL, clouds, capacity_blocks=4096, cfg_overrides=wc.CFG)
    _assert_equal(la, lb, sa, sb[-1])


def _frame_of_rays_without_steps():
    """Five one-point bundles in the last voxels of the layer's index range along x (|index| < 2^20 - 1), seen from 0.48 m: the points
    are inside the range, so they are bundled, and the ends of their rays (0.02 m behind them) are not, so dda_setup gives the rays
    no steps and flags the range error.  Checked here in the float32 operations of the kernels."""
    F = np.float32
    T = np.array([1, 0, 0, 0, 104857.0, 0.05, 0.05], F)
    pts = np.array([[0.484, 0.2 * k - 0.4, 0.1 * k - 0.2] for k in range(5)], F)
    inv, limit = F(1.0) / F(wc.VOXEL), F(1048575.0)
    for p in pts:
        pg = (p + T[4:]).astype(F)
        dv = (pg - T[4:]).astype(F)
        unit = (dv / np.sqrt((dv * dv).sum(dtype=F), dtype=F)).astype(F)
        end = (pg + unit * F(wc.CFG["default_truncation_distance"])).astype(F)
        assert np.all(np.abs(pg * inv) < limit) and not np.all(np.abs(end * inv) < limit)
    return T, pts, None


@pytest.mark.parametrize("touch", TOUCHES)
def test_rays_without_steps(hip, oracle, monkeypatch, touch):
    """0 steps: dda_setup gives a ray no steps only where it leaves the layer's index range, and the frame then reports
    COX_ERR_INDEX_RANGE at sync (the oracle has no such limit, so that frame is not fed to it).  Such rays are written, walk nothing
    and park nothing: the frame leaves the layer and the frame's tables alone, and the frames around it equal the oracle's."""
    bundles = [(n, 21 + 10 * j) for j, n in enumerate(SIZES)]
    clouds, lb, sb = _handmade(oracle, "sizes", bundles, seed=5)
    for name, value in _env(touch).items():
        monkeypatch.setenv(name, value)
    layer = Layer(hip, wc.VOXEL, capacity_blocks=4096)
    cfg = dict(synth.integrator_overrides(wc.VOXEL), **wc.CFG)
    integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **cfg), "merged")
    for name in _env(touch):
        monkeypatch.delenv(name)
    fed = [clouds[0], _frame_of_rays_without_steps(), clouds[1]]
    dev = _to_device(fed)
    _feed(integ, fed[:2], dev[:2])
    with pytest.raises(CoxError) as e:
        integ.sync()
    assert e.value.status == COX_ERR_INDEX_RANGE
    assert integ.last_stats()["n_rays"] == 5 and integ.last_stats()["n_updates"] == 0
    _feed(integ, fed[2:], dev[2:])
    integ.sync()
    _assert_equal(layer, lb, integ.last_stats(), sb[-1])


@pytest.mark.parametrize("touch", TOUCHES)
def test_axis_aligned_rays_beside_oblique_ones(hip, oracle, monkeypatch, touch):
    """Single points straight along +x, -y and +z of the sensor (two zero components: infinite crossing times, the sequential fallback
    on lane 0) and in a coordinate plane (one zero component), interleaved with oblique bundles, so workgroups take both ways."""
    key = "axis"
    if key not in _cache:
        obl, rgba, _ = wc.bundle_cloud([(3, 40), (1, 77), (5, 64), (2, 90), (1, 33), (4, 128)], seed=7)
        straight = np.array([[2.31, 0, 0], [0, -1.77, 0], [0, 0, 3.09], [1.52, 1.31, 0], [4.4, 0, 0], [0, 2.0, -2.6]], np.float32)
        rows, cols = [], []
        for j in range(6):
            rows.append(straight[j])
            cols.append(rgba[j])
            rows.append(obl[j])  # (bundle_cloud deals its first round one point per bundle)
            cols.append(rgba[j])
        rows.extend(obl[6:])
        cols.extend(rgba[6:])
        _cache[key] = [(wc.POSE, np.ascontiguousarray(np.array(rows, np.float32)), np.ascontiguousarray(np.array(cols, np.uint8)))] * 2
    clouds = _cache[key]
    lb, sb = _oracle_run(oracle, ("wim", key), wc.VOXEL, clouds, capacity_blocks=4096, cfg_overrides=wc.CFG)
    assert sb[0]["n_rays"] == 12
    la, _, sa = _hip_async(hip, monkeypatch, _env(touch), wc.VOXEL, clouds, capacity_blocks=4096, cfg_overrides=wc.CFG)
    _assert_equal(la, lb, sa, sb[-1])


# ---- 7: special bundles and frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("touch", TOUCHES)
def test_clearing_bundles_no_colours_empty_and_one_point_frames(hip, oracle, monkeypatch, touch):
    """Clearing bundles (points beyond max_ray_length_m: the ray ends at that range, only the bundle's first point counts) of 1, 64, 65
    and 130 points among plain ones; the same frame without colours; an empty frame and a one-point frame between full ones.  The
    frame table must be clean after each: the frames that follow equal the oracle's."""
    key = "special"
    if key not in _cache:
        pts, rgba, _ = wc.bundle_cloud([(n, 25 + 9 * j) for j, n in enumerate(SIZES[:6])], seed=8)
        rng = np.random.default_rng(9)
        clear = []
        for j, n in enumerate([1, 64, 65, 130]):  # voxels 10.6 - 11.3 m out, a voxel per bundle
            c = (np.array([[61, 60, 61], [-62, 61, 60], [60, -63, -61], [-61, -60, 64]][j]) + 0.5) * wc.VOXEL
            assert np.linalg.norm(c - wc.ORIGIN) > wc.CFG["max_ray_length_m"] + 0.2
            clear.append(c + rng.uniform(-wc.JITTER, wc.JITTER, (n, 3)) - wc.ORIGIN.astype(np.float64))
        clear = np.concatenate(clear).astype(np.float32)
        order = rng.permutation(len(pts) + len(clear))
        p = np.ascontiguousarray(np.concatenate([pts, clear])[order])
        c = np.ascontiguousarray(np.concatenate([rgba, rng.integers(0, 256, (len(clear), 4), dtype=np.uint8)])[order])
        T2, p2, c2 = _frames(0.10, 9, n=2)[1]
        _cache[key] = [(wc.POSE, p, c), (wc.POSE, p, None), (T2, p2, c2), (wc.POSE, np.zeros((0, 3), np.float32), None), (wc.POSE, p, c),
                       (wc.POSE, p[:1], c[:1]), (T2, p2, None), (wc.POSE, p, c)]
    clouds = _cache[key]
    lb, sb = _oracle_run(oracle, ("wim", key), wc.VOXEL, clouds, capacity_blocks=16384, cfg_overrides=wc.CFG)
    assert sb[0]["n_rays"] == 10 and sb[3]["n_rays"] == 0 and sb[5]["n_rays"] == 1
    la, _, sa = _hip_async(hip, monkeypatch, _env(touch), wc.VOXEL, clouds, capacity_blocks=16384, cfg_overrides=wc.CFG)
    _assert_equal(la, lb, sa, sb[-1])


# ---- 8: anti-grazing --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("touch", TOUCHES)
def test_anti_grazing_at_10cm(hip, oracle, monkeypatch, touch):
    """grazing_skip inside the merge: ray A runs through blocks 0 and 1 and skips the first voxel of block 1 on its way (the terminal
    voxel of bundle B), so it has to take block 1 with its next voxel; then the synthetic frames with the switch on."""
    origin = np.array([0.05, 0.05, 0.05], np.float32)
    d = np.array([1.0, 0.01, 0.02])
    A, B = origin + 3.0 * d, origin + 1.6 * d
    assert tuple(np.floor(B / 0.1).astype(int)) == (16, 0, 0) and tuple(np.floor((origin + 1.5 * d) / 0.1).astype(int)) == (15, 0, 0)
    pts = (np.stack([A, B, [-1.0, 2.0, 0.7]]) - origin).astype(np.float32)
    T = np.array([1, 0, 0, 0, *origin], np.float32)
    ag = dict(enable_anti_grazing=1)
    clouds = [(T, pts, None), (T, pts, None)] + list(_frames(0.10, 9)[:6])
    lb, sb = _oracle_run(oracle, ("wim graze",), 0.10, clouds, cfg_overrides=ag)
    la, _, sa = _hip_async(hip, monkeypatch, _env(touch), 0.10, clouds, cfg_overrides=ag)
    _assert_equal(la, lb, sa, sb[-1])


# ---- 9, 10: small record buffers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("touch", TOUCHES)
def test_record_cap_below_a_frames_records_drops_that_frame(hip, oracle, monkeypatch, touch):
    """A whole image among frames of an image's upper quarter, record buffers between the two record counts: the large frame is
    dropped whole and reported at sync; it allocates the blocks it touches and writes no voxel; the frames behind it fuse correctly."""
    small = [(T, p[:len(p) // 4], c[:len(p) // 4]) for T, p, c in _frames(0.05, 3, n=8)]
    big = _frames(0.05, 3, n=8)[2]
    kept, fed = small, small[:3] + [big] + small[3:]
    lk, sk = _oracle_run(oracle, ("wim drop kept",), 0.05, kept)
    lf, sf = _oracle_run(oracle, ("wim drop fed",), 0.05, fed)
    most, full = max(s["n_updates"] for s in sk), sf[3]["n_updates"]  # (every record is an update in this configuration)
    cap = (most + full) // 2
    assert most < cap < full
    env = _env(touch, COX_RECORD_CAP=str(cap))
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    layer = Layer(hip, 0.05, capacity_blocks=16384)
    integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **synth.integrator_overrides(0.05)), "merged")
    for name in env:
        monkeypatch.delenv(name)
    dev = _to_device(fed)
    _feed(integ, fed[:6], dev[:6])
    with pytest.raises(CoxError) as e:
        integ.sync()
    assert e.value.status == COX_ERR_INTERNAL
    _feed(integ, fed[6:], dev[6:])
    integ.sync()
    compare_stats([integ.last_stats()], [sk[-1]])
    got, voxels, blocks = _blocks(layer), _blocks(lk), _blocks(lf)
    assert set(got) == set(blocks) and layer.stats()[0] == len(blocks)
    for key, vox in got.items():
        if key in voxels:
            assert np.array_equal(vox, voxels[key]), key
        else:
            assert not vox[:, 1].any(), key


@pytest.mark.parametrize("touch", TOUCHES)
def test_record_cap_between_the_records_and_the_path_slots(hip, oracle, monkeypatch, touch):
    """Record buffers that hold every frame's records but not a path slot per ray (slots are steps_max = 376 or 379 words at 5 cm):
    the rays from cap / stride on park no path (kRayNoPath) and emit walks them itself -- the same records, the oracle's layer."""
    clouds = _stream(0.05)
    lb, sb = _oracle_run(oracle, ("wim stream", 0.05), 0.05, clouds)
    cap = 2 * max(s["n_updates"] for s in sb)
    assert all(cap // 370 + 100 < s["n_rays"] for s in sb)  # at least a hundred rays of every frame are without a slot
    la, _, sa = _hip_async(hip, monkeypatch, _env(touch, COX_RECORD_CAP=str(cap)), 0.05, clouds)
    _assert_equal(la, lb, sa, sb[-1])
