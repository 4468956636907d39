"""Parity of the HIP registration cost (K4) against the CPU oracle, through the C ABI.

Bar: same explicit sample indices, f32 interpolation, f64 outputs; residual
vector within 1e-4 abs, Jacobians within 1e-3 rel, reduced H / b / cost within 1e-6 rel.
"""
import numpy as np
import pytest

import layer_ref
from coxgraph_amd import synth
from coxgraph_amd.capi import Layer, RegPoints, Registration
from util import run_frames

pytestmark = pytest.mark.gpu


def registration_points(layer, trunc, min_weight=1.0):
    """voxgraph 'implicit_to_implicit' point set: voxel centres with weight > min_weight and |d| < trunc,
    in (z,y,x) block order / linear voxel order -> float32 [n,5] = x,y,z,distance,weight (submap frame)."""
    idx, vox = layer.download()
    return layer_ref.relevant_points_ref(idx, vox, layer.voxel_size, min_weight, trunc)


@pytest.fixture(scope="module")
def submaps(hip, oracle):
    """Two overlapping submaps of one client (frames 0-11 and 6-17, every 6th pixel), built by the ORACLE and
    uploaded to both engines so the registration inputs are identical on both sides."""
    la, _, _ = run_frames(oracle, method="merged", voxel=0.10, frames=range(0, 60, 5), subsample=6)
    lb, _, _ = run_frames(oracle, method="merged", voxel=0.10, frames=range(30, 90, 5), subsample=6)
    pts = registration_points(la, 0.3)
    idx, vox = lb.download()
    lh = Layer(hip, 0.10, capacity_blocks=4096)
    lh.upload(idx, vox)
    return pts, lb, lh


def _pair(hip, oracle, submaps, ncc=0.0):
    pts, lb, lh = submaps
    return Registration(hip, RegPoints(hip, pts), lh, ncc), Registration(oracle, RegPoints(oracle, pts), lb, ncc), pts


@pytest.mark.parametrize("pose", [((0, 0, 0, 0), (0, 0, 0, 0)), ((0.02, -0.01, 0.0, 0.01), (0.05, -0.03, 0.02, np.radians(1.0))),
                                  ((1.0, 2.0, -0.5, 0.7), (1.04, 1.97, -0.52, 0.68))])
def test_evaluate_matches_oracle(hip, oracle, submaps, pose):
    gh, go, pts = _pair(hip, oracle, submaps)
    pr, pd = np.array(pose[0], float), np.array(pose[1], float)
    rh, jfh, jrh = gh.evaluate(pr, pd)
    ro, jfo, jro = go.evaluate(pr, pd)
    assert len(ro) == len(pts) > 5000
    assert np.count_nonzero(ro) > 0.3 * len(ro)
    assert np.max(np.abs(rh - ro)) <= 1e-4
    for a, b in ((jfh, jfo), (jrh, jro)):
        assert np.max(np.abs(a - b)) <= 1e-3 * max(1.0, float(np.max(np.abs(b))))
    print("max |dr|", np.max(np.abs(rh - ro)), "bit-exact residuals:", np.array_equal(rh, ro), "J:", np.array_equal(jfh, jfo), np.array_equal(jrh, jro))


def test_sampled_evaluate_and_normal_equations(hip, oracle, submaps):
    gh, go, pts = _pair(hip, oracle, submaps, ncc=0.05)
    rng = np.random.default_rng(7)
    w = pts[:, 4].astype(np.float64)
    n_res = int(0.3 * len(pts))  # sampling_ratio 0.3 (coxgraph/config/server.yaml:30), weight-proportional, with replacement
    idx = rng.choice(len(pts), size=n_res, replace=True, p=w / w.sum()).astype(np.uint32)
    pr, pd = np.array([0.0, 0, 0, 0]), np.array([0.05, -0.03, 0.02, np.radians(1.0)])
    rh, jfh, jrh = gh.evaluate(pr, pd, idx)
    ro, jfo, jro = go.evaluate(pr, pd, idx)
    assert np.max(np.abs(rh - ro)) <= 1e-4
    Hh, bh, ch, nh = gh.normal_eq(pr, pd, idx)
    Ho, bo, co, no = go.normal_eq(pr, pd, idx)
    assert nh == no and 0 < nh <= n_res
    scale = max(1.0, float(np.max(np.abs(Ho))))
    assert np.max(np.abs(Hh - Ho)) <= 1e-6 * scale
    assert np.max(np.abs(bh - bo)) <= 1e-6 * max(1.0, float(np.max(np.abs(bo))))
    assert abs(ch - co) <= 1e-6 * max(1.0, co)
    # the fused reduction equals J^T J of the materialised Jacobian
    J = np.concatenate([jfh, jrh], axis=1)
    assert np.allclose(Hh, J.T @ J, rtol=1e-9, atol=1e-9 * scale)
    assert np.allclose(bh, J.T @ rh, rtol=1e-9, atol=1e-9 * scale)
    assert np.allclose(Hh, Hh.T)
    # reproducible run to run (fixed reduction order)
    H2, b2, c2, _ = gh.normal_eq(pr, pd, idx)
    assert np.array_equal(Hh, H2) and np.array_equal(bh, b2) and ch == c2


def test_begin_finish_and_stored_samples_give_the_same_numbers(hip, oracle, submaps):
    """The split form a pose-graph evaluation uses (begin all constraints, then collect) and sample indices kept on the
    GPU: identical to the one-call form, on both engines."""
    from coxgraph_amd.capi import CoxError
    pts, lb, lh = submaps
    rng = np.random.default_rng(11)
    idx = rng.integers(0, len(pts), size=4000).astype(np.uint32)
    poses = [(np.array([0.0, 0, 0, 0]), np.array([0.05, -0.03, 0.02, 0.02])), (np.array([0.1, 0.2, 0.0, -0.01]), np.array([0.12, 0.18, 0.01, 0.0])),
             (np.zeros(4), np.zeros(4))]
    for eng, layer in ((hip, lh), (oracle, lb)):
        regs = [Registration(eng, RegPoints(eng, pts), layer, 0.05) for _ in poses]
        want = [g.normal_eq(pr, pd, idx) for g, (pr, pd) in zip(regs, poses)]
        for g in regs:
            g.set_samples(idx)
        for g, (pr, pd) in zip(regs, poses):
            g.normal_eq_begin(pr, pd)             # stored samples, nothing waited for yet
        got = [g.normal_eq_finish() for g in regs]
        for (H0, b0, c0, n0), (H1, b1, c1, n1) in zip(want, got):
            assert np.array_equal(H0, H1) and np.array_equal(b0, b1) and c0 == c1 and n0 == n1
        r0, _, _ = regs[0].evaluate(*poses[0], idx)
        r1, _, _ = regs[0].evaluate(*poses[0])    # stored samples through the Ceres-shaped call as well
        assert np.array_equal(r0, r1)
        regs[0].normal_eq_begin(*poses[0])
        with pytest.raises(CoxError):             # one begin outstanding per handle
            regs[0].normal_eq_begin(*poses[0])
        regs[0].normal_eq_finish()
        with pytest.raises(CoxError):
            regs[0].normal_eq_finish()
        regs[0].set_samples(None)                 # back to "all points in order"
        ra, _, _ = regs[0].evaluate(*poses[0])
        assert len(ra) == len(pts)


def test_jacobian_against_central_differences_on_gpu(hip, oracle, submaps):
    gh, _, pts = _pair(hip, oracle, submaps)
    pr, pd = np.array([0.01, 0.02, -0.01, 0.01]), np.array([0.03, -0.02, 0.01, -0.01])
    r0, jf, jr = gh.evaluate(pr, pd)
    h = 2e-3
    ok = r0 != 0
    for k in range(4):
        e = np.zeros(4)
        e[k] = h
        rp = gh.evaluate(pr + e, pd, jacobians=False)[0]
        rm = gh.evaluate(pr - e, pd, jacobians=False)[0]
        m = ok & (rp != 0) & (rm != 0)
        num = (rp - rm) / (2 * h)
        # trilinear field is only piecewise smooth: compare in the median, not pointwise
        err = np.abs(num[m] - jf[m, k])
        assert np.median(err) < 0.05 * max(1e-3, float(np.median(np.abs(jf[m, k])))) + 1e-3, (k, np.median(err))


def test_edge_cases(hip, oracle, submaps):
    pts, lb, lh = submaps
    # empty point set
    g0 = Registration(hip, RegPoints(hip, np.zeros((0, 5), np.float32)), lh)
    H, b, c, n = g0.normal_eq(np.zeros(4), np.zeros(4))
    assert not H.any() and not b.any() and c == 0 and n == 0
    # reference far away from the reading submap: no correspondences at all -> residual = w * no_correspondence_cost * scale
    far = pts[:300].copy()
    far[:, :3] += 500.0
    gh = Registration(hip, RegPoints(hip, far), lh, 0.25)
    go = Registration(oracle, RegPoints(oracle, far), lb, 0.25)
    rh, jfh, _ = gh.evaluate(np.zeros(4), np.zeros(4))
    ro, _, _ = go.evaluate(np.zeros(4), np.zeros(4))
    assert np.array_equal(rh, ro) or np.max(np.abs(rh - ro)) < 1e-12
    assert not jfh.any()
    assert gh.normal_eq(np.zeros(4), np.zeros(4))[3] == 0


def test_registration_points_extracted_on_the_gpu(hip, oracle, submaps):
    pts, lb, lh = submaps
    a = lh.registration_points(1.0, 0.3)
    b = lb.registration_points(1.0, 0.3)
    assert a.shape == b.shape and a.shape[0] > 1000 and np.array_equal(a, b)
    # and straight into a device-resident point set used by the cost
    rp = RegPoints.from_layer(hip, lh, 1.0, 0.3)
    assert rp.n == len(b)
    gh = Registration(hip, rp, lh)
    go = Registration(oracle, RegPoints(oracle, b), lb)
    pose = np.array([0.02, -0.01, 0.01, 0.005])
    rh, _, _ = gh.evaluate(np.zeros(4), pose)
    ro, _, _ = go.evaluate(np.zeros(4), pose)
    assert np.max(np.abs(rh - ro)) <= 1e-4


def test_two_stage_optimize_recovers_a_perturbed_submap_pose(hip, oracle):
    """The server flow of coxgraph_server.cpp:396-476 on the GPU: two overlapping submaps of one client are fused on the GPU,
    the second one is handed over (wire format) with a perturbed pose, a loop closure + forced registration constraint are
    added and PoseGraphInterface::optimize runs its two stages.  Same flow driven by the oracle gives the same poses."""
    from coxgraph_amd.posegraph import PoseGraphInterface
    delta = np.array([0.05, -0.03, 0.02, np.radians(1.0)])  # SURVEY.md section 8d perturbation
    poses = {}
    for name, eng in (("hip", hip), ("oracle", oracle)):
        kw = dict(capacity_blocks=4096) if eng is hip else {}
        la, _, _ = run_frames(eng, method="merged", voxel=0.10, frames=range(0, 60, 5), subsample=6, **kw)
        lb, _, _ = run_frames(eng, method="merged", voxel=0.10, frames=range(30, 90, 5), subsample=6, **kw)
        ref_pts = RegPoints.from_layer(eng, la, 1.0, 0.3)
        assert ref_pts.n > 3000
        reg = Registration(eng, ref_pts, lb)
        g = PoseGraphInterface()
        g.addSubmap(0, [0, 0, 0, 0])
        g.addSubmap(1, delta)  # both submaps were built in the same world frame: the true relative pose is identity
        # a sloppy loop closure (place recognition) that is 2 cm / 0.5 deg off, then the registration constraint refines it
        g.addLoopClosureMeasurement(0, 1, [0.02, 0.0, -0.01, np.radians(0.5)])
        g.addForceRegistrationConstraint(0, 1, reg)
        first, second = g.optimize(enable_registration=True)
        poses[name] = g.getPoseMap()[1]
        cost0 = reg.normal_eq(np.zeros(4), delta)[2]
        cost1 = reg.normal_eq(np.zeros(4), poses[name])[2]
        cost_true = reg.normal_eq(np.zeros(4), np.zeros(4))[2]  # not 0: the two submaps saw the scene from different poses
        print(name, "pose", poses[name], "registration cost", cost0, "->", cost1, "(at the true pose:", cost_true, ")", second)
        assert cost1 < 0.6 * cost0 and cost1 < 1.1 * cost_true
        assert np.linalg.norm(poses[name][:3]) < 0.03 and abs(poses[name][3]) < np.radians(0.6)
    assert np.allclose(poses["hip"], poses["oracle"], atol=1e-6)
