"""GPU collision checks (coxgraph_amd/csrc/cox_collide.hip) against the test-side reference (tests/cpp/collide_reference.cpp, whose
trilinear branch is the CPU checker's getVoxelsAndQVector), against a numpy recount on an affine field, against the map queries,
and in the orders the engine promises.  Every flag, index, count and float is compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import collide_ref as cr
import map_ref
from collide_ref import C_DISTANCE, C_OBSERVED, C_TRAVERSABLE, SEG_FEASIBLE, SEG_GOAL
from coxgraph_amd import synth
from coxgraph_amd.capi import COLLIDE_RECORD_DTYPE, CollisionChecker, Integrator, Layer
from util import run_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (32, 64)
F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cr.build(tmp_path_factory.mktemp("collideref"))


def _upload(hip, idx, words):
    layer = Layer(hip, float(cr.VS), capacity_blocks=4 * len(idx) + 8)
    layer.upload(idx, words)
    return layer


@pytest.fixture(scope="module")
def wall(hip, ref):
    idx, words = cr.wall_layer_arrays(3)
    return _upload(hip, idx, words), ref.layer(cr.VS, idx, words)


@pytest.fixture(scope="module")
def room(hip, ref):
    """The analytic room, 2 000 segments in it and the reference's records of them (radius 0.5, the yaml's defaults otherwise)."""
    idx, words = cr.room_layer_arrays()
    a, b = cr.room_segments(np.random.default_rng(21))
    exp = ref.layer(cr.VS, idx, words).segments(a, b, collision_radius=0.5)
    return _upload(hip, idx, words), a, b, exp["records"]


@pytest.fixture(scope="module")
def submap(hip):
    """The 10 cm submap tests/test_gpu_submap.py fuses (frames 0..140 step 10 of the benchmark stream, merged, subsample 2) and its
    ESDF with coxgraph's band (esdf_max_distance 4 m, coxgraph_client.yaml:68)."""
    layer, _, _ = run_frames(hip, method="merged", voxel=0.10, frames=range(0, 150, 10), subsample=2, capacity_blocks=8192)
    return layer, layer.esdf(max_distance_m=4.0, min_distance_m=0.1)


def _as_records(out):
    rec = np.zeros(len(out["flags"]), cr.RECORD_DTYPE)
    for k in out:
        if k in cr.RECORD_DTYPE.names:
            rec[k] = out[k]
    return rec


def _same(got, exp):
    bad = cr.records_equal(got if isinstance(got, np.ndarray) else _as_records(got), exp)
    assert bad is None, bad


# ---- round and group edges -------------------------------------------------------------------------------------------------
SAMPLE_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 128, 129)
H = 1.0 / 64.0  # sample spacing of the edge cases: a binary fraction, so are all sample positions
EDGE = dict(collision_radius=0.5, sample_spacing=H, max_extension_range=0.0)


def _edge_cases():
    """(samples m, first blocked k or None): k at index 0, at the last lane of a round and the first lane of the next (for both group
    sizes), at the last sample, and nowhere.  Sample i sits at x0 + i / 64 on the wall d = 4 - x: blocked from x = 3.5 on, so x0 =
    3.5 + 1/128 - k / 64 puts sample k 1/128 inside and sample k - 1 1/128 outside."""
    cases = []
    for m in SAMPLE_COUNTS:
        for k in sorted({0, 31, 32, 63, 64, m - 1} & set(range(m))) + [None]:
            x0 = 3.5 + H / 2 - k * H if k is not None else 3.5 - H / 2 - (m - 1) * H
            cases.append((m, k, x0))
    return cases


def test_round_and_group_edges(hip, wall):
    layer, R = wall
    cases = _edge_cases()
    seg = [(m, k, x0) for m, k, x0 in cases if m >= 2]  # a segment has at least two samples
    a = np.array([[x0, 0.75, 0.75] for _, _, x0 in seg], np.float32)
    b = np.array([[x0 + (m - 1) * H, 0.75, 0.75] for m, _, x0 in seg], np.float32)
    exp = R.segments(a, b, **EDGE)["records"]
    assert exp["n_samples"].tolist() == [m - 1 for m, _, _ in seg]
    assert exp["first_blocked"].tolist() == [k if k is not None else m for m, k, _ in seg]  # the reference finds what was placed
    # the same samples as stored trajectories, with the one-sample cases
    pts = [np.array([[x0 + i * H, 0.75, 0.75] for i in range(m)], np.float32) for m, _, x0 in cases]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.uint64)
    xyz = np.concatenate(pts)
    exp_t = R.trajectories(offsets, xyz, **EDGE)
    assert exp_t["first_blocked"].tolist() == [k if k is not None else m for m, k, _ in cases]
    for g in GROUPS:
        cc = CollisionChecker(hip, layer, group_size=g, **EDGE)
        _same(cc.segments(a, b), exp)
        _same(cc.trajectories(offsets, xyz), exp_t)
        cc.close()


# ---- mixed batch on the analytic room --------------------------------------------------------------------------------------
def test_mixed_batch_on_the_analytic_room(hip, room):
    layer, a, b, exp = room
    feasible = (exp["flags"] & SEG_FEASIBLE) != 0
    cropped = ((exp["flags"] & SEG_GOAL) != 0) & ~feasible
    print(f"room: feasible {feasible.mean():.3f}, cropped goal {cropped.mean():.3f}, first_blocked max {exp['first_blocked'].max()}")
    assert 0.10 <= feasible.mean() <= 0.90 and cropped.mean() >= 0.05  # on the reference's output
    for g in GROUPS:
        cc = CollisionChecker(hip, layer, group_size=g, collision_radius=0.5)
        _same(cc.segments(a, b), exp)
        cc.close()
    _same(layer.check_segments(a, b, collision_radius=0.5), exp)


def test_records_do_not_depend_on_the_batch(hip, room):
    layer, a, b, exp = room
    for g in GROUPS:
        cc = CollisionChecker(hip, layer, group_size=g, collision_radius=0.5)
        for n in (1, 2, 65, 2000):
            _same(cc.segments(a[:n], b[:n]), exp[:n])
        _same(cc.segments(a[::-1], b[::-1]), exp[::-1])
        halves = [cc.segments(a[:1000], b[:1000]), cc.segments(a[1000:], b[1000:])]
        _same(np.concatenate([_as_records(h) for h in halves]), exp)
        cc.close()


# ---- the fused layer --------------------------------------------------------------------------------------------------------
def _observed_starts(rng, idx, vox, n):
    """Start points in known space: centres of observed voxels, moved by up to half a voxel."""
    w = vox[..., 1].view(np.float32)
    obs = map_ref.voxel_centres(idx, 0.1)[w > 0]
    return (obs[rng.integers(0, len(obs), n)] + rng.uniform(-0.05, 0.05, size=(n, 3))).astype(np.float32)


def _random_trajectories(rng, starts, lengths):
    """Random walks of 5 cm steps from the starts."""
    pts = []
    for s, m in zip(starts, lengths):
        steps = rng.normal(size=(m, 3))
        steps *= 0.05 / np.linalg.norm(steps, axis=1)[:, None]
        steps[0] = 0.0
        pts.append((s.astype(np.float64) + np.cumsum(steps, axis=0)).astype(np.float32))
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    return offsets, np.concatenate(pts)


@pytest.mark.parametrize("kind,radius", [("esdf", 0.3), ("tsdf", 0.02)])
def test_fused_layer(hip, ref, submap, kind, radius):
    layer = submap[1] if kind == "esdf" else submap[0]
    idx, vox = layer.download()
    R = ref.layer(0.1, idx, vox)
    rng = np.random.default_rng(22)
    a = _observed_starts(rng, idx, vox, 1000)
    b = cr.ball_segments(rng, a, synth.ROOM_MIN, synth.ROOM_MAX).astype(np.float32)
    exp = R.segments(a, b, collision_radius=radius)["records"]
    share = ((exp["flags"] & SEG_FEASIBLE) != 0).mean()
    print(f"{kind} radius {radius}: feasible {share:.3f}, goals {((exp['flags'] & SEG_GOAL) != 0).mean():.3f}")
    assert 0.10 <= share <= 0.90  # on the reference's output
    lengths = rng.integers(1, 201, 200)
    offsets, xyz = _random_trajectories(rng, _observed_starts(rng, idx, vox, 200), lengths)
    exp_t = R.trajectories(offsets, xyz, collision_radius=radius)
    assert 0 < ((exp_t["flags"] & SEG_FEASIBLE) != 0).sum() < 200
    for g in GROUPS:
        cc = CollisionChecker(hip, layer, group_size=g, collision_radius=radius)
        _same(cc.segments(a, b), exp)
        _same(cc.trajectories(offsets, xyz), exp_t)
        cc.close()


# ---- trajectories ----------------------------------------------------------------------------------------------------------
def test_trajectories_in_csr_form(hip, ref, room):
    layer = room[0]
    idx, words = cr.room_layer_arrays()
    R = ref.layer(cr.VS, idx, words)
    rng = np.random.default_rng(23)
    lengths = np.array([0, 1, 0, 64, 65, 200, 0, 1, 64, 65, 200, 0, 0, 200, 1], np.int64)
    starts = rng.uniform([0.8, 0.8, 0.3], [5.6, 5.6, 2.9], size=(len(lengths), 3))
    offsets, xyz = _random_trajectories(rng, starts, np.maximum(lengths, 1))
    keep = np.concatenate([np.arange(o, o + m) for o, m in zip(offsets[:-1].astype(np.int64), lengths)])  # drop the point of the empty ones
    xyz = xyz[keep]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    exp = R.trajectories(offsets, xyz, collision_radius=0.5)
    assert exp["n_samples"].tolist() == lengths.tolist()
    empty = lengths == 0
    assert np.all(exp["flags"][empty] == SEG_FEASIBLE) and np.all(exp["first_blocked"][empty] == 0)
    assert len(set(exp["flags"][~empty].tolist())) == 2  # feasible and blocked ones
    for g in GROUPS:
        cc = CollisionChecker(hip, layer, group_size=g, collision_radius=0.5)
        _same(cc.trajectories(offsets, xyz), exp)
        # offsets as given: a CSR that starts inside the point array and uses part of it
        _same(cc.trajectories(offsets[3:9], xyz), exp[3:8])
        cc.close()


# ---- trees -----------------------------------------------------------------------------------------------------------------
def _random_forest(rng, n, roots=7):
    """Parents in shuffled node order: node order[i] hangs under an earlier node of the order, the first `roots` are roots."""
    order = rng.permutation(n)
    parent = np.full(n, -1, np.int32)
    for i in range(roots, n):
        parent[order[i]] = order[rng.integers(0, i)]
    return parent


def test_trees(hip, ref, wall):
    cc = CollisionChecker(hip, wall[0])
    rng = np.random.default_rng(24)
    # a chain takes the most rounds; 1 025 nodes run in one workgroup, 5 000 with one launch per round
    chain = np.arange(-1, 1024, dtype=np.int32)
    for blocked in ([], [1024], [0], [512], [3, 700]):
        f = np.ones(1025, np.uint8)
        f[blocked] = 0
        keep = cc.prune(chain, f)
        assert np.array_equal(keep, ref.prune(chain, f))
        first = min(blocked) if blocked else 1025
        assert keep[:first].all() and not keep[first:].any()
    rev = chain[::-1].copy()  # the same chain with every parent at the higher index
    rev = np.where(rev >= 0, 1024 - rev, -1).astype(np.int32)
    f = np.ones(1025, np.uint8)
    f[100] = 0
    assert np.array_equal(cc.prune(rev, f), ref.prune(rev, f))
    for n in (5000, 4096, 4097):
        parent = _random_forest(rng, n)
        f = (rng.uniform(size=n) > 0.01).astype(np.uint8)
        keep = cc.prune(parent, f)
        assert np.array_equal(keep, ref.prune(parent, f))
        assert 0 < keep.sum() < n
    # a long chain in the launch-per-round path, with a cycle and a bad parent spliced into the forest
    parent = _random_forest(rng, 5000)
    parent[:3000] = np.arange(-1, 2999)
    parent[4000], parent[4001] = 4001, 4000
    parent[4500] = 5000
    f = np.ones(5000, np.uint8)
    f[2500] = 0
    keep = cc.prune(parent, f)
    assert np.array_equal(keep, ref.prune(parent, f))
    assert keep[4000] == keep[4001] == keep[4500] == cr.TREE_INVALID and keep[2499] == 1 and keep[2999] == 0
    for name, (parent, feasible, expect) in cr.TREES.items():
        assert cc.prune(parent, feasible).tolist() == expect, name
    cc.close()


def test_tree_is_trajectories_followed_by_prune(hip, ref, room):
    import torch
    layer = room[0]
    rng = np.random.default_rng(25)
    for n in (300, 5000):
        parent = _random_forest(rng, n, roots=3)
        lengths = rng.integers(0, 12, n)
        starts = rng.uniform([0.8, 0.8, 0.3], [5.6, 5.6, 2.9], size=(n, 3))
        offsets, xyz = _random_trajectories(rng, starts, np.maximum(lengths, 1))
        cc = CollisionChecker(hip, layer, collision_radius=0.5)
        traj = cc.trajectories(offsets, xyz)
        keep = cc.prune(parent, (traj["flags"] & SEG_FEASIBLE).astype(np.uint8))
        tree = cc.tree(offsets, parent, xyz)
        _same(tree, _as_records(traj))
        assert np.array_equal(tree["keep"], keep)
        assert np.array_equal(keep, ref.prune(parent, (traj["flags"] & 1).astype(np.uint8)))
        assert 0 < (keep == 1).sum() < n
        # the device form, and prune_dev reading the flags of the records directly (stride 32)
        d_off, d_par, d_xyz = torch.from_numpy(offsets.astype(np.int64)).cuda(), torch.from_numpy(parent).cuda(), torch.from_numpy(xyz).cuda()
        d_rec = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        d_keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_keep2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        cc.tree_dev(d_off, d_par, n, d_xyz, len(xyz), d_rec, d_keep)
        cc.prune_dev(d_par, d_rec.data_ptr() + 8, d_keep2, n=n, feasible_stride=32)
        torch.cuda.synchronize()
        _same(d_rec.cpu().numpy().view(cr.RECORD_DTYPE), _as_records(traj))
        assert np.array_equal(d_keep.cpu().numpy(), keep) and np.array_equal(d_keep2.cpu().numpy(), keep)
        cc.close()


# ---- engine promises -------------------------------------------------------------------------------------------------------
def test_a_check_sees_the_frames_enqueued_before_it(hip):
    voxel = 0.10
    cfg = hip.default_config(**synth.integrator_overrides(voxel))
    layer = Layer(hip, voxel, capacity_blocks=8192)
    integ = Integrator(hip, layer, cfg, "merged")
    cc = CollisionChecker(hip, layer, collision_radius=0.02)
    rng = np.random.default_rng(26)
    a = rng.uniform(synth.ROOM_MIN, synth.ROOM_MAX, size=(4000, 3)).astype(np.float32)
    b = cr.ball_segments(rng, a, synth.ROOM_MIN, synth.ROOM_MAX, 0.5).astype(np.float32)
    keep = []
    for t in (0, 10, 20):
        T, pts, rgba, _ = synth.make_frame(t)
        keep.append((T, np.ascontiguousarray(pts[::2]), np.ascontiguousarray(rgba[::2])))
        integ.integrate_points_async(T, keep[-1][1].ctypes.data, keep[-1][2].ctypes.data, len(keep[-1][1]))
    right_after = cc.segments(a, b)  # no sync in between
    integ.sync()
    after = cc.segments(a, b)
    _same(right_after, _as_records(after))
    assert 0 < (after["first_blocked"] > 0).sum() < len(a)  # some segments start in free known space


def test_dev_forms_on_a_side_stream(hip, room):
    import torch
    layer, a, b, exp = room
    cc = CollisionChecker(hip, layer, collision_radius=0.5)
    host_pts = cc.points(a)
    s = torch.cuda.Stream()
    n = len(a)
    with torch.cuda.stream(s):
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        rec = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        state = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dist = torch.full((n,), float("nan"), device="cuda")
        cc.segments_dev(da, db, rec, stream=s)
        cc.points_dev(da, state=state, distance=dist, stream=s)
        offsets = torch.arange(0, n + 1, 8, dtype=torch.int64, device="cuda")
        trec = torch.zeros((n // 8) * 32, dtype=torch.uint8, device="cuda")
        cc.trajectories_dev(offsets, n // 8, da, n, trec, stream=s)
    s.synchronize()
    _same(rec.cpu().numpy().view(COLLIDE_RECORD_DTYPE), exp)
    assert np.array_equal(state.cpu().numpy(), host_pts["state"])
    has_d = (host_pts["state"] & C_DISTANCE) != 0
    got_d = dist.cpu().numpy()
    assert np.array_equal(got_d[has_d].view(np.uint32), host_pts["distance"][has_d].view(np.uint32))
    assert has_d.any() and np.isnan(got_d[~has_d]).all() and np.isnan(host_pts["distance"][~has_d]).all()  # left as it was / NaN
    _same(trec.cpu().numpy().view(COLLIDE_RECORD_DTYPE), _as_records(cc.trajectories(np.arange(0, n + 1, 8), a)))
    cc.close()


def test_edge_cases_and_error_codes(hip, room):
    layer, a, b, exp = room
    f = hip.fn
    empty = Layer(hip, 0.1, capacity_blocks=64)
    out = CollisionChecker(hip, empty).segments(a[:10], b[:10])
    assert np.all(out["first_blocked"] == 0) and np.all(out["flags"] & SEG_FEASIBLE == 0)  # nothing is observed
    assert np.all(CollisionChecker(hip, empty, collision_optimistic=1).segments(a[:10], b[:10])["flags"] & SEG_FEASIBLE)
    st = CollisionChecker(hip, empty).points(a[:10])
    assert np.all(st["state"] == 0) and np.isnan(st["distance"]).all()
    cc = CollisionChecker(hip, layer, collision_radius=0.5)
    # n = 0 is COX_OK whatever else is passed
    z = C.c_uint64(0)
    assert f("collide_points")(cc.h, None, z, None, None) == 0
    assert f("collide_points_dev")(cc.h, None, z, None, None, None) == 0
    assert f("collide_segments")(cc.h, None, None, z, None) == 0
    assert f("collide_segments_dev")(cc.h, None, None, z, None, None) == 0
    assert f("collide_trajectories")(cc.h, None, z, None, z, None) == 0
    assert f("collide_trajectories_dev")(cc.h, None, z, None, z, None, None) == 0
    assert f("collide_prune_dev")(cc.h, None, None, C.c_uint64(1), z, None, None) == 0
    assert f("collide_tree")(cc.h, None, None, z, None, z, None, None) == 0
    assert f("collide_tree_dev")(cc.h, None, None, z, None, z, None, None, None) == 0
    assert len(cc.segments(a[:0], b[:0])["flags"]) == 0 and len(cc.points(a[:0])["state"]) == 0
    # NULL outputs: only the state, or only the distance
    full = cc.points(a)
    state = np.zeros(len(a), np.uint8)
    assert f("collide_points")(cc.h, a.ctypes.data_as(C.c_void_p), C.c_uint64(len(a)), state.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(state, full["state"])
    dist = np.zeros(len(a), np.float32)
    assert f("collide_points")(cc.h, a.ctypes.data_as(C.c_void_p), C.c_uint64(len(a)), None, dist.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(dist.view(np.uint32), full["distance"].view(np.uint32))
    # error codes
    one = C.c_uint64(1)
    assert f("collide_segments")(cc.h, a.ctypes.data_as(C.c_void_p), None, one, None) == -1
    assert f("collide_points")(cc.h, None, one, None, None) == -1
    assert f("collide_set_group_size")(cc.h, C.c_int(48)) == -1
    bad_offsets = np.array([0, 5, 3], np.uint64)
    rec = np.zeros(2, COLLIDE_RECORD_DTYPE)
    args = (a.ctypes.data_as(C.c_void_p), C.c_uint64(len(a)), rec.ctypes.data_as(C.c_void_p))
    assert f("collide_trajectories")(cc.h, bad_offsets.ctypes.data_as(C.c_void_p), C.c_uint64(2), *args) == -1
    beyond = np.array([0, 5, len(a) + 1], np.uint64)
    assert f("collide_trajectories")(cc.h, beyond.ctypes.data_as(C.c_void_p), C.c_uint64(2), *args) == -1
    from coxgraph_amd.capi import CoxError
    for bad in (dict(collision_radius=np.nan), dict(sample_spacing=-0.1), dict(clearing_radius=-1.0), dict(max_samples=(1 << 24) + 1),
                dict(crop_margin=np.inf)):
        with pytest.raises(CoxError) as e:
            CollisionChecker(hip, layer, **bad)
        assert e.value.status == -1
    # sample_spacing 0 is the layer's voxel size
    _same(CollisionChecker(hip, layer, collision_radius=0.5, sample_spacing=0.0).segments(a[:100], b[:100]),
          _as_records(CollisionChecker(hip, layer, collision_radius=0.5, sample_spacing=float(cr.VS)).segments(a[:100], b[:100])))
    # a layer that has grown between calls answers as before
    idx, words = cr.room_layer_arrays()
    grown = Layer(hip, 0.1, capacity_blocks=len(idx) + 8)
    grown.upload(idx, words)
    cg = CollisionChecker(hip, grown, collision_radius=0.5)
    _same(cg.segments(a, b), exp)
    grown.reserve(4 * len(idx) + 64)
    _same(cg.segments(a, b), exp)
    cc.close()


def test_clearing_centre_moves_between_calls(hip, ref, room):
    layer, a, b, _ = room
    idx, words = cr.room_layer_arrays()
    R = ref.layer(cr.VS, idx, words)
    cc = CollisionChecker(hip, layer, collision_radius=0.5, clearing_radius=1.0, clearing_centre=(2.4, 4.0, 0.8))
    _same(cc.segments(a, b), R.segments(a, b, collision_radius=0.5, clearing_radius=1.0, clearing_centre=(2.4, 4.0, 0.8))["records"])
    cc.set_clearing_centre((5.6, 0.8, 2.4))  # inside the other removed blocks
    exp = R.segments(a, b, collision_radius=0.5, clearing_radius=1.0, clearing_centre=(5.6, 0.8, 2.4))
    _same(cc.segments(a, b), exp["records"])
    st = cc.points(a)["state"]
    assert np.array_equal(st, R.points(a, collision_radius=0.5, clearing_radius=1.0, clearing_centre=(5.6, 0.8, 2.4))["state"])
    assert (st & cr.C_CLEARED).any()
    cc.close()


def test_stats_show_the_early_exit(hip, room):
    layer, a, b, exp = room
    feasible = (exp["flags"] & SEG_FEASIBLE) != 0
    for g in GROUPS:
        cc = CollisionChecker(hip, layer, group_size=g, collision_radius=0.5)
        cc.set_profiling(True)
        cc.segments(a[feasible], b[feasible])
        st = cc.stats(reset=True)
        assert st["n_samples_skipped"] == 0 and st["n_launches"] == 1 and st["kernel_ms"] > 0.0
        assert st["n_samples_evaluated"] == int((exp["n_samples"][feasible].astype(np.int64) + 1).sum())
        # the wall of the room blocks long segments at their first sample: everything after the first round is skipped
        far = np.array([[0.2, 3.0, 1.0]] * 50, np.float32)
        to = np.array([[0.2, 3.0 + 0.05 * 200, 1.0]] * 50, np.float32)
        cc2 = CollisionChecker(hip, layer, group_size=g, collision_radius=0.5, max_extension_range=0.0)
        out = cc2.segments(far, to)
        st = cc2.stats()
        assert np.all(out["first_blocked"] == 0) and np.all(out["n_samples"] == 200)
        assert st["n_samples_evaluated"] == 50 * g and st["n_samples_skipped"] == 50 * (201 - g)
        assert cc.stats()["n_samples_evaluated"] == 0  # reset
        cc.close()
        cc2.close()


# ---- no reference needed ---------------------------------------------------------------------------------------------------
def test_axis_parallel_segments_on_the_affine_wall_match_a_numpy_recount(hip, wall):
    """d = 4 - x is affine, so its trilinear value is the field: sample i of a segment along +-x is blocked iff 4 - x_i <= 0.5 (or
    x_i leaves the part of the layer with complete cells).  Thresholds stay 1e-3 clear of every sample."""
    layer, _ = wall
    rng = np.random.default_rng(27)
    n = 500
    ds = 0.05
    xa = rng.uniform(0.2, 4.5, n)
    sign = rng.choice([-1.0, 1.0], n)
    length = rng.uniform(0.0, 1.5, n)
    yz = rng.uniform(0.2, 1.4, size=(n, 2))
    a = np.column_stack([xa, yz]).astype(np.float32)
    b = a.copy()
    b[:, 0] = (xa + sign * length).astype(np.float32)
    out = CollisionChecker(hip, layer, collision_radius=0.5, sample_spacing=ds, max_extension_range=0.0, crop=0).segments(a, b)
    checked = 0
    for i in range(n):
        lenf = abs(float(b[i, 0]) - float(a[i, 0]))
        steps = lenf / ds
        if abs(steps - round(steps)) < 1e-3:
            continue  # the number of samples itself is on a threshold
        ns = max(int(np.ceil(steps)), 1)
        x = float(a[i, 0]) + np.arange(ns + 1) / ns * (float(b[i, 0]) - float(a[i, 0]))
        if np.min(np.abs(x - 3.5)) < 1e-3 or np.min(np.abs(x - 0.05)) < 1e-3 or np.min(np.abs(x - 4.75)) < 1e-3:
            continue
        blocked = (x >= 3.5) | (x < 0.05)
        first = int(np.argmax(blocked)) if blocked.any() else ns + 1
        assert out["n_samples"][i] == ns and out["first_blocked"][i] == first, i
        assert bool(out["flags"][i] & SEG_FEASIBLE) == (not blocked.any())
        checked += 1
    assert checked > 400
    assert 0.1 < np.mean(out["flags"] & SEG_FEASIBLE != 0) < 0.9


# ---- agreement with the existing queries -----------------------------------------------------------------------------------
def test_states_agree_with_the_map_queries(hip, submap, room):
    rng = np.random.default_rng(28)
    for layer, lo, hi, radius in ((submap[1], synth.ROOM_MIN - 0.5, synth.ROOM_MAX + 0.5, 0.3), (room[0], [-0.5] * 3, [6.9, 6.9, 3.7], 0.5)):
        p = rng.uniform(lo, hi, size=(10_000, 3)).astype(np.float32)
        p[:8] = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [5e6, 0, 0], [0, -5e6, 0], [1e30, 1e30, 1e30], [4e6, 1, 1]],
                         np.float32)
        near = layer.query(p, "nearest")
        tri = layer.query(p, "interpolate")
        with np.errstate(invalid="ignore", over="ignore"):
            sc = p * (F(1.0) / (F(0.1) * F(16)))
            in_range = np.all((sc > F(-1048575.0)) & (sc < F(1048575.0)), axis=1)
        observed = (near["status"] & 1) != 0
        has_d = observed & ((tri["status"] & 1) != 0)
        exp = np.where(observed, C_OBSERVED, 0) | np.where(has_d, C_DISTANCE, 0) | np.where(has_d & (tri["distance"] > F(radius)), C_TRAVERSABLE, 0)
        exp = np.where(in_range, exp, cr.C_INVALID).astype(np.uint8)
        got = CollisionChecker(hip, layer, collision_radius=radius).points(p)
        assert np.array_equal(got["state"], exp)
        assert np.array_equal(got["distance"][has_d].view(np.uint32), tri["distance"][has_d].view(np.uint32))
        assert np.isnan(got["distance"][~has_d]).all()
        assert has_d.sum() > 500 and (observed & ~has_d).any() and (~observed).sum() > 500 and (exp & C_TRAVERSABLE).any()


# ---- C++ -------------------------------------------------------------------------------------------------------------------
def test_cpp_planning_flow_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "collide_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "collide_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
