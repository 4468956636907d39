"""The merged record walk with block ordinals from the frame's own table (coxgraph_amd/csrc/cox_walk.hpp: FrameBlocks, k_bind_blocks)
and its two placements -- COX_WALK=raygen (walk and emit at the tail of stage M on the frame's ray-generation stream, stage T the
binding alone) and COX_WALK=update (all of it in stage T) -- against the CPU oracle: distance, weight and colour bit-equal, the
frame statistics equal.  Frames go in through the asynchronous device path, so frame sets and record sets are reused while their
previous users are still in flight."""
import numpy as np
import pytest

from coxgraph_amd import synth
from coxgraph_amd.capi import Layer, Integrator, CoxError
from util import compare_layers, compare_stats

pytestmark = pytest.mark.gpu

WALKS = ("raygen", "update")
N_ASYNC = 14  # frames per asynchronous stream: every one of the six frame sets and three record sets is used at least twice
_cache = {}


def _frames(voxel, sub, n=N_ASYNC, step=5):
    """The subsampled synthetic frames, made once per shape."""
    key = ("frames", sub, n, step)
    if key not in _cache:
        out = []
        for t in range(n):
            T, p, c, _ = synth.make_frame(step * t)
            out.append((T, np.ascontiguousarray(p[::sub]), np.ascontiguousarray(c[::sub])))
        _cache[key] = out
    return _cache[key]


def _oracle_run(oracle, key, voxel, clouds, capacity_blocks=16384, cfg_overrides=None, method="merged"):
    """(layer, stats per frame) of the oracle for a list of (T, points, colours or None), computed once and left unchanged."""
    if key not in _cache:
        ov = synth.integrator_overrides(voxel)
        ov.update(cfg_overrides or {})
        layer = Layer(oracle, voxel, capacity_blocks=capacity_blocks)
        integ = Integrator(oracle, layer, oracle.default_config(integrator_threads=1, **ov), method)
        stats = []
        for T, p, c in clouds:
            integ.integrate_points(T, p, c)
            stats.append(integ.last_stats())
        _cache[key] = (layer, stats, integ)
    return _cache[key][0], _cache[key][1]


def _to_device(clouds):
    import torch
    dev = [(torch.from_numpy(p).cuda() if len(p) else None, torch.from_numpy(c).cuda() if c is not None and len(c) else None) for _, p, c in clouds]
    torch.cuda.synchronize()
    return dev


def _feed(integ, clouds, dev):
    """every frame through cox_integrate_points_dev, none waited for"""
    for (T, p, _), (dp, dc) in zip(clouds, dev):
        integ.integrate_points_dev(T, dp.data_ptr() if dp is not None else 0, dc.data_ptr() if dc is not None else 0, len(p))


def _hip_async(hip, monkeypatch, env, voxel, clouds, capacity_blocks=16384, cfg_overrides=None, auto_grow=True):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    ov = synth.integrator_overrides(voxel)
    ov.update(cfg_overrides or {})
    layer = Layer(hip, voxel, capacity_blocks=capacity_blocks)
    if not auto_grow:
        layer.set_auto_grow(False)
    integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **ov), "merged")  # (the switches are read here)
    for name in env:
        monkeypatch.delenv(name)
    dev = _to_device(clouds)
    _feed(integ, clouds, dev)
    integ.sync()
    return layer, integ, integ.last_stats()


def _blocks(layer):
    """block index -> its voxel words"""
    idx, vox = layer.download()
    return {tuple(int(x) for x in i): v for i, v in zip(idx, vox)}


def _assert_equal(la, lb, sa=None, sb=None):
    rep = compare_layers(la, lb)
    assert rep["bitexact_d"] and rep["bitexact_w"] and rep["n_diff_color"] == 0, rep
    if sa is not None:
        compare_stats([sa], [sb])
    return rep


# ---- both placements against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", ["COX_QUEUES=3", "COX_QUEUES=4", "COX_QUEUES=16", "COX_SUBMIT_THREAD=0", "COX_GRAPH=1"])
@pytest.mark.parametrize("walk", WALKS)
def test_both_placements_equal_the_oracle(hip, oracle, monkeypatch, walk, extra):
    """14 asynchronous 5 cm frames per case: the queue budgets that give one stream, H P M x2 | T R U and H P M x2 | T R | U, no
    submission thread, stage graphs (which keep the walk in stage T)."""
    clouds = _frames(0.05, 3)
    lb, sb = _oracle_run(oracle, ("o", 0.05, 3), 0.05, clouds)
    env = dict([extra.split("=")], COX_WALK=walk)
    la, _, sa = _hip_async(hip, monkeypatch, env, 0.05, clouds)
    _assert_equal(la, lb, sa, sb[-1])


@pytest.mark.parametrize("walk", WALKS)
def test_both_placements_at_10cm(hip, oracle, monkeypatch, walk):
    clouds = _frames(0.10, 9)
    lb, sb = _oracle_run(oracle, ("o", 0.10, 9), 0.10, clouds)
    la, _, sa = _hip_async(hip, monkeypatch, dict(COX_WALK=walk), 0.10, clouds)
    _assert_equal(la, lb, sa, sb[-1])


# ---- bucket edges: 255, 256 and 257 touched blocks ---------------------------------------------------------------------------------
def _cloud_touching(oracle, target):
    """A 2 cm cloud for which the ORACLE counts exactly `target` touched blocks -- its n_new_blocks of the cloud on an empty layer, where
    every block a frame touches is new (the oracle keeps no count of touched blocks for the ray-casting integrators).  Points of frame 0
    are added one at a time and kept while that count stays at or below the target: a ray adds a handful of 32 cm blocks, the last
    steps need one that adds one."""
    key = ("touch", target)
    if key in _cache:
        return _cache[key]
    T, p, c, _ = synth.make_frame(0)
    cand = np.arange(0, len(p), 97)
    cfg = oracle.default_config(integrator_threads=1, **synth.integrator_overrides(0.02))

    def count(idx):
        layer = Layer(oracle, 0.02, capacity_blocks=1024)
        integ = Integrator(oracle, layer, cfg, "merged")
        integ.integrate_points(T, p[idx], c[idx])
        return integ.last_stats()["n_new_blocks"]

    # a prefix of the candidates that stays below the target (bisection; the count grows with the prefix but for bundling), then one by one
    lo, hi = 1, len(cand)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(cand[:mid]) <= target:
            lo = mid
        else:
            hi = mid - 1
    keep = list(cand[:lo])
    n = count(np.array(keep))
    for i in cand[lo:]:
        if n == target:
            break
        m = count(np.array(keep + [i]))
        if m <= target:
            keep.append(i)
            n = m
    idx = np.array(keep)
    _cache[key] = (T, np.ascontiguousarray(p[idx]), np.ascontiguousarray(c[idx]), n)
    return _cache[key]


@pytest.mark.parametrize("select", ["COX_PARTITION=records,COX_BUCKETS=1", "COX_PARTITION=records,COX_BUCKETS=0", "COX_APPLY=records"])
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("target", [255, 256, 257])
def test_bucket_edges(hip, oracle, monkeypatch, target, walk, select):
    """Up to 255 touched blocks a bucket of the one-pass partition is a tile, from 256 on tiles share buckets, and the ordinal's key
    width steps from 8 to 9 bits between 255 and 256: the frame twice (new blocks, then known ones), large axis cap (2 cm)."""
    T, p, c, n = _cloud_touching(oracle, target)
    assert n == target
    clouds = [(T, p, c), (T, p, c)]
    lb, sb = _oracle_run(oracle, ("edge", target), 0.02, clouds, capacity_blocks=1024)
    assert sb[0]["n_new_blocks"] == target and sb[1]["n_new_blocks"] == 0 and lb.stats()[0] == target
    env = dict(kv.split("=") for kv in select.split(","))
    la, _, sa = _hip_async(hip, monkeypatch, dict(env, COX_WALK=walk), 0.02, clouds, capacity_blocks=1024)
    assert sa["n_touched_blocks"] == target  # (the second frame: every block known, every block touched again)
    _assert_equal(la, lb, sa, sb[-1])


# ---- anti-grazing ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
def test_anti_grazing_first_voxel_of_a_block_skipped(hip, oracle, monkeypatch, walk):
    """Ray A runs along x through blocks 0 and 1 (10 cm voxels, 1.6 m blocks); point B sits in voxel (16, 0, 0), the first voxel of
    block 1 on A's way, so A skips it (the terminal voxel of another bundle) and has to take block 1 with its next voxel.  A third ray
    far away; then the same frame again, and the synthetic frames with the switch on."""
    origin = np.array([0.05, 0.05, 0.05], np.float32)
    d = np.array([1.0, 0.01, 0.02])
    A = origin + 3.0 * d
    B = origin + 1.6 * d
    assert tuple(np.floor(B / 0.1).astype(int)) == (16, 0, 0) and tuple(np.floor((origin + 1.5 * d) / 0.1).astype(int)) == (15, 0, 0)
    pts = (np.stack([A, B, [-1.0, 2.0, 0.7]]) - origin).astype(np.float32)  # the sensor sits at `origin`, unrotated
    T = np.array([1, 0, 0, 0, *origin], np.float32)
    ag = dict(enable_anti_grazing=1)
    clouds = [(T, pts, None), (T, pts, None)] + [(Tf, p, c) for Tf, p, c in _frames(0.10, 9)[:6]]
    lb, sb = _oracle_run(oracle, ("graze", 0.10), 0.10, clouds, cfg_overrides=ag)
    la, _, sa = _hip_async(hip, monkeypatch, dict(COX_WALK=walk), 0.10, clouds, cfg_overrides=ag)
    _assert_equal(la, lb, sa, sb[-1])


@pytest.mark.parametrize("walk", WALKS)
def test_anti_grazing_with_the_large_axis_cap(hip, oracle, monkeypatch, walk):
    """Anti-grazing at 2 cm: records (the piece walk does not read the bundle hash) through k_touch_wave<512>."""
    ag = dict(enable_anti_grazing=1)
    clouds = _frames(0.02, 9, n=4)
    lb, sb = _oracle_run(oracle, ("graze", 0.02), 0.02, clouds, capacity_blocks=40000, cfg_overrides=ag)
    la, _, sa = _hip_async(hip, monkeypatch, dict(COX_WALK=walk), 0.02, clouds, capacity_blocks=40000, cfg_overrides=ag)
    _assert_equal(la, lb, sa, sb[-1])


# ---- the pool --------------------------------------------------------------------------------------------------------------------------
def _n_blocks_raw(layer):
    import ctypes as C
    n, b = C.c_uint64(), C.c_uint64()
    layer.eng.fn("layer_stats")(layer.h, C.byref(n), C.byref(b))  # status ignored: the layer may be in its error state
    return int(n.value)


@pytest.mark.parametrize("walk", WALKS)
def test_pool_exactly_full_one_short_and_reserve(hip, oracle, monkeypatch, walk):
    clouds = _frames(0.05, 3, n=6)
    lb, sb = _oracle_run(oracle, ("pool", 6), 0.05, clouds)
    need = lb.stats()[0]
    assert need > 50
    # exactly what the oracle needs: equal to the oracle
    la, _, sa = _hip_async(hip, monkeypatch, dict(COX_WALK=walk), 0.05, clouds, capacity_blocks=need, auto_grow=False)
    _assert_equal(la, lb, sa, sb[-1])
    assert la.stats()[0] == need
    # one block less, frame by frame: -4 in the frame that runs out and in the next frame that meets the block, never more blocks than the pool has
    monkeypatch.setenv("COX_WALK", walk)
    layer = Layer(hip, 0.05, capacity_blocks=need - 1)
    layer.set_auto_grow(False)
    integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **synth.integrator_overrides(0.05)), "merged")
    monkeypatch.delenv("COX_WALK")
    failed_at = None
    for k, (T, p, c) in enumerate(clouds):
        try:
            integ.integrate_points(T, p, c)
        except CoxError as e:
            assert e.status == -4
            failed_at = k
            break
    assert failed_at is not None and sum(s["n_new_blocks"] for s in sb[:failed_at + 1]) > need - 1 >= sum(s["n_new_blocks"] for s in sb[:failed_at])
    assert _n_blocks_raw(layer) <= need - 1
    with pytest.raises(CoxError) as e:  # the same frame meets the block without storage again
        integ.integrate_points(*clouds[failed_at])
    assert e.value.status == -4 and _n_blocks_raw(layer) <= need - 1
    # after reserve() the stream continues on the same integrator: the table dropped the key without storage, the block comes back with
    # the next frame that meets it, and everything outside that one block is what the oracle has after the same calls (the frame
    # that failed went in twice, each time for every block but the one without storage)
    layer.reserve(need + 64)
    rest = clouds[failed_at + 1:] + clouds[failed_at:failed_at + 1]
    for T, p, c in rest:
        integ.integrate_points(T, p, c)
    assert layer.stats()[0] == need
    calls = clouds[:failed_at + 1] + clouds[failed_at:failed_at + 1] + rest
    lc, _ = _oracle_run(oracle, ("pool calls", failed_at), 0.05, calls)
    got, want = _blocks(layer), _blocks(lc)
    assert set(got) == set(want)
    lost = [k for k in want if not np.array_equal(got[k], want[k])]
    assert len(lost) == 1, lost  # need - 1 blocks of storage: exactly one block was without
    # ... and a stream on the cleared layer equals a fresh run: the errors left nothing behind in the integrator's tables
    layer.clear()
    dev = _to_device(clouds)
    _feed(integ, clouds, dev)
    integ.sync()
    _assert_equal(layer, lb, integ.last_stats(), sb[-1])


# ---- a dropped frame ------------------------------------------------------------------------------------------------------------------
COX_ERR_INTERNAL = -8


@pytest.mark.parametrize("select", ["", "COX_APPLY=records"])
@pytest.mark.parametrize("walk", WALKS)
def test_dropped_frame_binds_and_leaves_the_tables_clean(hip, oracle, monkeypatch, walk, select):
    """A frame with more records than the record buffers hold is dropped as a whole and reported at sync (COX_RECORD_CAP makes the
    buffers small enough for a test-sized cloud: a whole image among frames of an image's upper quarter).  It still allocates
    the blocks it touches, as the walk always has, and writes no voxel; the frames behind it on the same integrator, before and
    after the sync that reports it, are the oracle's -- so the dropped frame's binding left the frame table empty and its records
    behind.  Through the tile apply (the binding at the head of k_block_starts_bind) and the full record sort (k_bind_blocks)."""
    small = [(T, p[:len(p) // 4], c[:len(p) // 4]) for T, p, c in _frames(0.05, 3, n=8)]  # the upper quarter of the image: a quarter of the records
    big = _frames(0.05, 3, n=8)[2]  # a whole image from a pose the stream has: four times the records
    kept = small[:3] + small[3:]
    fed = small[:3] + [big] + small[3:]
    lk, sk = _oracle_run(oracle, ("drop kept",), 0.05, kept)   # what the voxels must be: the stream without the dropped frame
    lf, sf = _oracle_run(oracle, ("drop fed",), 0.05, fed)     # which blocks must exist: the dropped frame allocates what it touches
    # every record is an update in this configuration (no anti-grazing, storage for every block): the oracle's counts place the capacity
    most, full = max(s["n_updates"] for s in sk), sf[3]["n_updates"]
    cap = (most + full) // 2
    assert most < cap < full
    env = dict(COX_WALK=walk, COX_RECORD_CAP=str(cap))
    if select:
        env.update([select.split("=")])
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    layer = Layer(hip, 0.05, capacity_blocks=16384)
    integ = Integrator(hip, layer, hip.default_config(integrator_threads=1, **synth.integrator_overrides(0.05)), "merged")
    for name in env:
        monkeypatch.delenv(name)
    dev = _to_device(fed)
    _feed(integ, fed[:6], dev[:6])  # three frames, the dropped one, two more: nobody waits
    with pytest.raises(CoxError) as e:
        integ.sync()
    assert e.value.status == COX_ERR_INTERNAL
    _feed(integ, fed[6:], dev[6:])
    integ.sync()  # the error was reported once; these frames are clean
    compare_stats([integ.last_stats()], [sk[-1]])
    got, voxels, blocks = _blocks(layer), _blocks(lk), _blocks(lf)
    assert set(got) == set(blocks) and layer.stats()[0] == len(blocks)   # the pool holds the dropped frame's blocks too
    for key, vox in got.items():
        if key in voxels:
            assert np.array_equal(vox, voxels[key]), key
        else:
            assert not vox[:, 1].any(), key  # allocated by the dropped frame only: no voxel observed


# ---- a frame without a valid point between ordinary ones ----------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
def test_frames_without_valid_points_in_the_stream(hip, oracle, monkeypatch, walk):
    """Every third frame of the stream holds only points closer than min_ray_length_m (no ray, no touched block: the binding has
    nothing to do and the tables stay clean), one frame is an empty cloud."""
    base = _frames(0.05, 3, n=8)
    near = np.full((500, 3), 0.01, np.float32)
    clouds = []
    for k, (T, p, c) in enumerate(base):
        clouds.append((T, p, c))
        if k % 3 == 1:
            clouds.append((T, near, None))
        if k == 4:
            clouds.append((T, np.zeros((0, 3), np.float32), None))
    clouds.append(base[0])
    lb, sb = _oracle_run(oracle, ("novalid",), 0.05, clouds)
    la, _, sa = _hip_async(hip, monkeypatch, dict(COX_WALK=walk), 0.05, clouds)
    _assert_equal(la, lb, sa, sb[-1])


# ---- two integrators on one layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["merged", "simple"])
@pytest.mark.parametrize("walk", WALKS)
def test_two_integrators_on_one_layer(hip, oracle, monkeypatch, walk, other):
    """Frames alternate between two integrators of one layer, nobody waits: the binding of a frame follows the foreign writer's
    frames (a simple integrator inserts into the layer's table from its own touch kernel), and the layer is the oracle's in call order."""
    clouds = _frames(0.05, 9, n=N_ASYNC)
    res = []
    for eng in (hip, oracle):
        cfg = eng.default_config(integrator_threads=1, **synth.integrator_overrides(0.05))
        layer = Layer(eng, 0.05, capacity_blocks=16384)
        if eng is hip:
            monkeypatch.setenv("COX_WALK", walk)
        ints = [Integrator(eng, layer, cfg, "merged"), Integrator(eng, layer, cfg, other)]
        if eng is hip:
            monkeypatch.delenv("COX_WALK")
            dev = _to_device(clouds)
        for t, (T, p, c) in enumerate(clouds):
            k = (t % 3) % 2  # merged, other, merged | merged, other, merged ...: single frames and pairs of the same integrator
            if eng is hip:
                ints[k].integrate_points_dev(T, dev[t][0].data_ptr(), dev[t][1].data_ptr(), len(p))
            else:
                ints[k].integrate_points(T, p, c)
        for i in ints:
            i.sync()
        res.append((layer, ints))
    _assert_equal(res[0][0], res[1][0])


# ---- table growth --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
def test_layer_table_and_pool_grow_mid_stream(hip, oracle, monkeypatch, walk):
    """30 asynchronous frames into a pool of 72 blocks, auto-grow on: the layer's table and pool are reallocated while frames are in
    flight, and the frame tables with them.  The shape leaves nothing to timing: the oracle needs its 73rd block in frame 15, and the
    caller cannot enqueue frame 15 before frame 3 is done (its parameter slot is frame 9's, whose frame set was frame 3's) -- by then
    the engine has seen more than 36 blocks and doubles the pool."""
    clouds = _frames(0.05, 3, n=30, step=3)
    lb, sb = _oracle_run(oracle, ("grow",), 0.05, clouds)
    cum = np.cumsum([s["n_new_blocks"] for s in sb])
    assert cum[3] > 36 and cum[14] <= 72 < cum[-1]
    la, _, sa = _hip_async(hip, monkeypatch, dict(COX_WALK=walk), 0.05, clouds, capacity_blocks=72)
    assert la.capacity() > 72
    _assert_equal(la, lb, sa, sb[-1])
