"""The pose-candidate sweep and the coarse-to-fine search on the GPU (coxgraph_amd/csrc/cox_align.hip, include/coxgraph_hip_align.h)
against the numpy statement tests/align_ref.py: the three integers of every record exactly, cost within the reordering bound of a
sum of m terms, records that depend on their own pose only, the search's trace level by level and bit for bit, and the C++ host
class.  DESIGN.md section 7o."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import align_ref as A
import reg_cases
import reg_ref
import track_ref
from coxgraph_amd.capi import ALIGN_SCORE_DTYPE, CoxError, Layer, RegPoints, Registration, SubmapAligner
from test_align_ref_cpu import room_search
from test_reg_ref_cpu import EngineLayers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.2
POSE_REF0, POSE_READ = (np.array(p, np.float64) for p in reg_cases.SMALL_POSE)
INTS = ("score", "n_corr", "n_inlier")
# reference poses that leave no point a correspondence against POSE_READ: beyond the packed keys, +-inf, NaN, out of reach
EXTRA_POSES = ((0, 3.0e6, 0, 0), (math.inf, 0, 0, 0), (0, math.nan, 0, 0.1), (100.0, 0, 0, 0.2), (0, 0, -math.inf, 0.3), (-3.0e6, 0, 0, 3.0))
N_SPECIAL = len(reg_cases.POSES) + len(EXTRA_POSES)


@pytest.fixture(scope="module")
def layers(hip):
    return EngineLayers(hip)


@functools.lru_cache(maxsize=None)
def candidates():
    """the reference poses of reg_cases.POSES and EXTRA_POSES, then 250 seeded jitters of SMALL_POSE's"""
    rng = np.random.default_rng(4242)
    jit = POSE_REF0 + rng.uniform(-1, 1, (250, 4)) * np.array([0.15, 0.15, 0.15, 0.1])
    return np.concatenate([np.array([p[1] for p in reg_cases.POSES] + list(EXTRA_POSES), np.float64), jit])


def base_points():
    return reg_cases.by_name("samples_1")["pts"]            # 300 points on the cube layer under SMALL_POSE


@functools.lru_cache(maxsize=None)
def ref_layer(name):
    return A.RefLayer(*reg_cases.layer(name))


@functools.lru_cache(maxsize=None)
def cube_reference(ncc):
    return A.sweep(ref_layer("cube"), base_points(), candidates(), POSE_READ, TAU, ncc)


def check(got, want, what):
    """records against A.sweep()'s (rec, sum_abs, scale, m)"""
    rec, sum_abs, scale, m = want
    assert got.dtype == ALIGN_SCORE_DTYPE and len(got) == len(rec), what
    for k in INTS:
        assert np.array_equal(got[k], rec[k]), (what, k, np.nonzero(got[k] != rec[k])[0][:8])
    bound = A.cost_bound(m, scale, sum_abs)
    err = np.abs(got["cost"] - rec["cost"])
    worst = int(np.argmax(err - bound))
    print(f"[{what}] M {len(rec)} m {m}: max |dcost| {err.max():.3g} (bound there {bound[np.argmax(err)]:.3g}), inliers {int(rec['n_inlier'].min())}..{int(rec['n_inlier'].max())}")
    assert np.all(err <= bound), (what, worst, float(err[worst]), float(bound[worst]))


@pytest.mark.parametrize("ncc", (0.0, 0.25))
@pytest.mark.parametrize("M", (1, 63, 64, 65, 257))
def test_sweep_matches_the_reference(hip, layers, M, ncc):
    want = cube_reference(ncc)
    rec = want[0]
    # the candidates exercise every class: no correspondence at all, inliers and outliers side by side, a quantum of every size
    assert (rec["n_corr"][:N_SPECIAL] == 0).sum() >= 3 + len(EXTRA_POSES) and (rec["n_corr"] > 100).sum() >= 250
    assert ((rec["n_inlier"] > 0) & (rec["n_inlier"] < rec["n_corr"])).sum() >= 250
    al = SubmapAligner(hip, RegPoints(hip, base_points()), layers("cube"), inlier_distance=TAU, no_correspondence_cost=ncc)
    got = al.sweep(candidates()[:M], POSE_READ)
    check(got, tuple(w[:M] if isinstance(w, np.ndarray) else w for w in want), f"cube M={M} ncc={ncc}")
    none = rec["n_corr"][:M] == 0
    w = base_points()[:, 4].astype(np.float64)
    flat = 0.5 * (len(w) / w.sum()) ** 2 * float(((w * ncc) ** 2).sum())     # what a pose without any correspondence costs
    assert np.allclose(got["cost"][none], flat, rtol=1e-12, atol=0)
    assert got["score"][none].sum() == 0 and got["n_inlier"][none].sum() == 0


@functools.lru_cache(maxsize=None)
def sample_reference():
    """per-point terms of the three candidates once; the counts only gather them"""
    poses = candidates()[[N_SPECIAL, 1, N_SPECIAL + 1]]
    poses[0] = POSE_REF0
    return poses, A.point_terms(ref_layer("cube"), base_points(), poses, POSE_READ, TAU, 0.25)


@pytest.mark.parametrize("count", reg_cases.SAMPLE_COUNTS)
def test_stored_samples_at_every_launch_shape(hip, layers, count, monkeypatch):
    c = reg_cases.by_name(f"samples_{count}")
    poses, terms = sample_reference()
    monkeypatch.setattr(A, "point_terms", lambda *a, **k: terms)
    want = A.sweep(ref_layer("cube"), c["pts"], poses, POSE_READ, TAU, 0.25, c["samples"])
    al = SubmapAligner(hip, RegPoints(hip, c["pts"]), layers("cube"), inlier_distance=TAU, no_correspondence_cost=0.25)
    al.set_samples(c["samples"])
    got = al.sweep(poses, POSE_READ)
    check(got, want, f"samples {count}")
    assert got.tobytes() == al.sweep(poses, POSE_READ).tobytes()
    if count == 257:      # NULL drops the stored list: all 300 points in order again
        al.set_samples(None)
        monkeypatch.undo()
        check(al.sweep(poses, POSE_READ), A.sweep(ref_layer("cube"), c["pts"], poses, POSE_READ, TAU, 0.25), "samples dropped")


def test_other_readings_and_degenerate_inputs(hip, layers):
    poses = np.concatenate([POSE_REF0[None], candidates()[N_SPECIAL:][:20]])
    # 0.05 m voxels
    c = reg_cases.by_name("fine")
    al = SubmapAligner(hip, RegPoints(hip, c["pts"]), layers("fine"), inlier_distance=0.1, no_correspondence_cost=0.25)
    jit = poses.copy()
    jit[:, :3] = POSE_REF0[:3] + (poses[:, :3] - POSE_REF0[:3]) * 0.3
    want = A.sweep(ref_layer("fine"), c["pts"], jit, POSE_READ, 0.1, 0.25)
    assert want[0]["n_inlier"].max() > 50
    check(al.sweep(jit, POSE_READ), want, "fine")
    # the ESDF of the cube layer as the reading; the reference is fed its download()
    esdf = layers("cube").esdf(max_distance_m=2.0)
    idx, vox = esdf.download()
    al = SubmapAligner(hip, RegPoints(hip, base_points()), esdf, inlier_distance=0.4)
    want = A.sweep(A.RefLayer(0.1, idx, vox), base_points(), poses, POSE_READ, 0.4, 0.0)
    assert want[0]["n_corr"].max() > 50
    check(al.sweep(poses, POSE_READ), want, "esdf")
    # an empty reading layer: no correspondence anywhere
    empty = Layer(hip, 0.1, capacity_blocks=64)
    al = SubmapAligner(hip, RegPoints(hip, base_points()), empty, inlier_distance=TAU, no_correspondence_cost=0.25)
    want = A.sweep(A.RefLayer(0.1, np.zeros((0, 3), np.int32), np.zeros((0, 4096, 3), np.uint32)), base_points(), poses, POSE_READ, TAU, 0.25)
    got = al.sweep(poses, POSE_READ)
    check(got, want, "empty layer")
    assert not got["n_corr"].any() and not got["score"].any() and (got["cost"] > 0).all()
    # all-zero weights: scale is 0 and so is the cost; the integers do not look at the weights
    c = reg_cases.by_name("w_all_zero")
    al = SubmapAligner(hip, RegPoints(hip, c["pts"]), layers("cube"), inlier_distance=TAU, no_correspondence_cost=0.25)
    want = A.sweep(ref_layer("cube"), c["pts"], poses, POSE_READ, TAU, 0.25)
    got = al.sweep(poses, POSE_READ)
    check(got, want, "zero weights")
    assert want[2] == 0.0 and not got["cost"].any() and got["n_corr"].max() > 100
    # an empty point set
    al = SubmapAligner(hip, RegPoints(hip, np.zeros((0, 5), np.float32)), layers("cube"))
    assert not al.sweep(poses, POSE_READ).view(np.uint8).any()


def test_tau_edges(hip, layers):
    """tau on one observed e: that point is an inlier and adds max(0, Q - u); tau one float below: it is not"""
    pts = base_points()
    pose = POSE_REF0[None]
    pp = reg_ref.per_point(ref_layer("cube"), pts, pose[0], POSE_READ)
    hi = np.nonzero(pp["has"])[0]
    # e of every point with a correspondence, as the rule computes it: |d - val| = |r / w| only up to rounding, so recompute
    has, dd, off = ref_layer("cube").cell(pp["pos"])
    val, _ = ref_layer("cube").value_and_gradient(dd, off)
    e = np.abs((pts[hi, 3] - val).astype(np.float32))
    al = SubmapAligner(hip, RegPoints(hip, pts), layers("cube"))
    order = np.argsort(e)
    for j in (order[len(order) // 2], order[len(order) // 4], order[-1]):
        assert e[j] > 0
        at, below = np.float32(e[j]), np.nextafter(np.float32(e[j]), np.float32(0))
        want_at, want_below = (A.sweep(ref_layer("cube"), pts, pose, POSE_READ, t)[0] for t in (at, below))
        got_at, got_below = (al.sweep(pose, POSE_READ, inlier_distance=float(t)) for t in (at, below))
        n_on = int((e == at).sum())
        assert int(want_at["n_inlier"][0]) == int((e <= at).sum()) and int(want_below["n_inlier"][0]) == int((e <= below).sum()) == int(want_at["n_inlier"][0]) - n_on
        u = int(np.floor(np.float32(at * np.float32(np.float32(1024.0) / at))))
        assert max(0, A.Q - u) in (0, 1)       # a point on the edge of the inlier band adds at most one quantum
        for k in INTS:
            assert got_at[k][0] == want_at[k][0] and got_below[k][0] == want_below[k][0], (k, float(at))
        print(f"[tau edge] e {float(at):.9g}: inliers {int(got_at['n_inlier'][0])} at, {int(got_below['n_inlier'][0])} below; scores {int(got_at['score'][0])}, {int(got_below['score'][0])}")


def test_records_depend_on_their_own_pose_only(hip, layers):
    al = SubmapAligner(hip, RegPoints(hip, base_points()), layers("cube"), inlier_distance=TAU, no_correspondence_cost=0.25)
    poses = candidates()[:65]
    batch = al.sweep(poses, POSE_READ)
    assert batch.tobytes() == al.sweep(poses, POSE_READ).tobytes()                 # run to run
    perm = np.random.default_rng(5).permutation(65)
    shuffled = al.sweep(poses[perm], POSE_READ)
    for i in range(65):
        alone = al.sweep(poses[i:i + 1], POSE_READ)
        assert alone.tobytes() == batch[i:i + 1].tobytes(), i
    for j, i in enumerate(perm):
        assert shuffled[j:j + 1].tobytes() == batch[i:i + 1].tobytes(), (j, i)
    # ... and with samples that stride (more than 1024 workgroups' worth), inside a larger batch
    c = reg_cases.by_name("samples_262145")
    al.set_samples(c["samples"])
    big = al.sweep(candidates()[:257], POSE_READ)
    assert big[100:103].tobytes() == al.sweep(candidates()[100:103], POSE_READ).tobytes()
    # ... and across the passes a sweep is cut into when candidates x chunks outgrow the partial sums (8 192 candidates at 1 024 chunks)
    M = 8192 + 5
    cyc = al.sweep(candidates()[np.arange(M) % 257], POSE_READ)
    assert cyc.tobytes() == big[np.arange(M) % 257].tobytes()


def test_cost_agrees_with_the_registration_cost(hip, layers):
    """at five poses, the sweep's cost and Registration.normal_eq's are each within their own bound of the reference"""
    pts = base_points()
    names = ("identity", "yaw_p90", "yaw_m7", "far_3000", "nan_yaw")
    ref_points = RegPoints(hip, pts)
    al = SubmapAligner(hip, ref_points, layers("cube"), inlier_distance=TAU, no_correspondence_cost=0.25)
    reg = Registration(hip, ref_points, layers("cube"), 0.25)
    for name in names:
        _, pf, pr, _ = next(p for p in reg_cases.POSES if p[0] == name)
        pf, pr = np.array(pf, np.float64), np.array(pr, np.float64)
        ne = reg_ref.normal_eq(ref_layer("cube"), pts, pf, pr, None, 0.25)
        rec, sum_abs, scale, m = A.sweep(ref_layer("cube"), pts, pf[None], pr, TAU, 0.25)
        got = al.sweep(pf[None], pr)
        cost_reg, n_corr_reg = reg.normal_eq(pf, pr)[2:]
        b_sweep, b_reg = float(A.cost_bound(m, scale, sum_abs)[0]), float(reg_ref.sum_bounds(ne)[2])
        print(f"[cost {name}] sweep {got['cost'][0]!r} registration {cost_reg!r} reference {ne['cost']!r} bounds {b_sweep:.3g} {b_reg:.3g}")
        assert abs(ne["cost"] - rec["cost"][0]) <= b_sweep                          # the two numpy statements agree
        assert abs(got["cost"][0] - rec["cost"][0]) <= b_sweep and abs(cost_reg - ne["cost"]) <= b_reg
        assert int(got["n_corr"][0]) == n_corr_reg == ne["n_corr"]


# ---- the search -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(hip):
    idx, words = track_ref.analytic_layer_arrays(A.ROOM_VOXEL, truncation=A.ROOM_TRUNCATION)
    lay = Layer(hip, A.ROOM_VOXEL, capacity_blocks=64)
    lay.upload(idx, words)
    return lay


def room_aligner(hip, room, pts):
    return SubmapAligner(hip, RegPoints(hip, pts), room, inlier_distance=A.ROOM_SEARCH["tau"])


def gpu_search(al, n_pts, **kw):
    s = A.ROOM_SEARCH
    return al.search((0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP, levels=s["levels"], keep=s["keep"], min_corr=n_pts // 4, tau_min=s["tau_min"], **kw)


@pytest.mark.parametrize("k", range(2))
def test_search_trace_equals_the_references(hip, room, k):
    true_pose, pts, want = room_search(k)
    got = gpu_search(room_aligner(hip, room, pts), len(pts), trace=True)
    assert len(got["levels"]) == len(want["levels"]) == 5
    for lv, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        assert g["n_candidates"] == w["n_candidates"] and g["inlier_distance"] == w["inlier_distance"], lv
        assert g["step"].tobytes() == w["step"].tobytes(), lv
        assert np.array_equal(g["kept_index"], w["kept_index"]), (lv, g["kept_index"], w["kept_index"])
        assert g["kept_pose"].tobytes() == w["kept_pose"].tobytes(), lv
        for name in INTS:
            assert np.array_equal(g["kept_score"][name], w["kept_score"][name]), (lv, name)
        assert np.allclose(g["kept_score"]["cost"], w["kept_score"]["cost"], rtol=1e-12, atol=0), lv
    assert got["poses"].tobytes() == want["poses"].tobytes() and got["n_found"] == 8
    assert got["scores"].tobytes() == got["levels"][-1]["kept_score"].tobytes()


@pytest.mark.parametrize("k", range(6))
def test_search_finds_the_true_pose_and_refine_does_not_raise_the_cost(hip, room, k):
    true_pose = A.room_true_poses(6)[k]
    pts = A.room_problem(true_pose)
    al = room_aligner(hip, room, pts)
    got = gpu_search(al, len(pts), refine=True)
    err = A.pose_error_steps(got["best"], true_pose)
    err_refined = A.pose_error_steps(got["refined"], true_pose)
    print(f"[search {k}] error in final steps {np.round(err, 3)}, refined {np.round(err_refined, 3)}; cost {got['cost_before']:.6g} -> {got['cost_after']:.6g}; "
          f"record {got['scores'][0]}")
    assert np.all(err <= 1.0), err
    assert got["cost_after"] <= got["cost_before"]
    reg = Registration(hip, al.ref, room, 0.0)
    zero = np.zeros(4)
    assert reg.normal_eq(got["refined"], zero)[2] <= reg.normal_eq(got["best"], zero)[2]
    assert got["cost_before"] == reg.normal_eq(got["best"], zero)[2]
    # no candidate meets an impossible min_corr: nothing found, no error
    if k == 0:
        none = al.search((0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP, levels=1, keep=8, min_corr=len(pts) + 1, tau_min=0.1, refine=True, trace=True)
        assert none["n_found"] == 0 and none["best"] is None and len(none["poses"]) == 0 and len(none["levels"]) == 1 and "refined" not in none


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(hip, layers):
    pts = base_points()
    ref_points = RegPoints(hip, pts)
    al = SubmapAligner(hip, ref_points, layers("cube"))
    poses = candidates()[:4].copy()
    good = al.sweep(poses, POSE_READ)

    def status(fn):
        with pytest.raises(CoxError) as e:
            fn()
        return e.value.status

    for tau in (0.0, -0.1, math.nan, math.inf, -math.inf):
        assert status(lambda: al.sweep(poses, POSE_READ, inlier_distance=tau)) == -1, tau
        assert status(lambda: SubmapAligner(hip, ref_points, layers("cube"), inlier_distance=tau)) == -1, tau
        assert status(lambda: al.search((0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP, inlier_distance=tau)) == -1, tau
        assert status(lambda: al.search((0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP, tau_min=tau)) == -1, tau
    for keep in (0, 65, 1000):
        assert status(lambda: al.search((0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP, keep=keep)) == -1, keep
    assert status(lambda: al.search((0, 0, 0, 0), A.ROOM_HALF, A.ROOM_STEP, levels=17)) == -1
    assert status(lambda: al.search((0, 0, math.nan, 0), A.ROOM_HALF, A.ROOM_STEP)) == -1
    assert status(lambda: al.search((0, 0, 0, 0), (1.0, -1.0, 0, 0), A.ROOM_STEP)) == -1
    for bad in (np.array([0, len(pts)], np.uint32), np.array([2 ** 32 - 1], np.uint32)):
        assert status(lambda: al.set_samples(bad)) == -1
    # raw calls: NULL pointers, too many candidates, M = 0
    f, h, tau = hip.fn("align_sweep"), al.h, C.c_float(0.2)
    out = np.zeros(4, ALIGN_SCORE_DTYPE)
    pr, pp, po = (a.ctypes.data_as(C.c_void_p) for a in (POSE_READ, poses, out))
    assert f(h, pr, pp, C.c_uint64(4), tau, po) == 0
    assert f(None, pr, pp, C.c_uint64(4), tau, po) == -1 and f(h, None, pp, C.c_uint64(4), tau, po) == -1
    assert f(h, pr, None, C.c_uint64(4), tau, po) == -1 and f(h, pr, pp, C.c_uint64(4), tau, None) == -1
    assert f(h, pr, pp, C.c_uint64((1 << 20) + 1), tau, po) == -1
    before = out.copy()
    assert f(h, pr, pp, C.c_uint64(0), tau, po) == 0 and out.tobytes() == before.tobytes()       # M = 0: COX_OK, nothing written
    assert len(al.sweep(np.zeros((0, 4)), POSE_READ)) == 0
    g = hip.fn("align_create")
    hh = C.c_void_p()
    assert g(None, layers("cube").h, None, C.byref(hh)) == -1 and g(ref_points.h, None, None, C.byref(hh)) == -1 and g(ref_points.h, layers("cube").h, None, None) == -1
    assert hip.fn("align_set_samples")(None, None, C.c_uint64(0)) == -1 and hip.fn("align_kernel_time")(None, None, None, C.c_int(0)) == -1
    s = hip.fn("align_search")
    assert s(h, pr, None, pp, po, C.byref(C.c_uint32()), None) == -1 and s(None, pr, None, pp, po, C.byref(C.c_uint32()), None) == -1
    # the refused calls left the handle as it was
    assert al.sweep(poses, POSE_READ).tobytes() == good.tobytes()
    ms, n = al.kernel_time(reset=True)
    assert ms > 0 and n >= 3 and al.kernel_time() == (0.0, 0)
    # a closed owner is caught before C is reached
    ref_points.close()
    assert status(lambda: al.sweep(poses, POSE_READ)) == -1


# ---- C++ --------------------------------------------------------------------------------------------------------------------------
def test_cpp_submap_aligner_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "align_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "align_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
