"""The HIP registration cost (coxgraph_amd/csrc/cox_reg.hip) against the numpy reference tests/reg_ref.py and the closed form
for an affine layer, on the seeded cases of tests/reg_cases.py: poses up to |yaw| = 3 pi and 3 km, non-finite poses and
points, every cell placement, weights with a zero sum, sample counts on wave / workgroup / partial-sum edges and across the
striding threshold of k_reg_normal_eq (1024 workgroups x 256), begin / finish out of order, batches with empty constraints
and more entries than the initial table.  The bars are those of tests/test_reg_ref_cpu.py, where the oracle meets them:
bit for bit per point, the reordering bound on the sums."""
import numpy as np
import pytest

import map_ref
import reg_cases
import reg_ref
import submap_cases
from coxgraph_amd.capi import CoxError, Layer, RegPoints, Registration
from test_reg_ref_cpu import (CASES, TOL_J_T, TOL_J_YAW, TOL_R, EngineLayers, affine_inputs, check_evaluate, check_normal_eq, closed_form_deviation,
                              compare_case, reference_of, same_normal_eq)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def layers(hip):
    return EngineLayers(hip)


def sample_case(count):
    return reg_cases.by_name(f"samples_{count}")


def poses_of(c):
    return c["pose_ref"], c["pose_read"]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_hip_matches_reference(layers, c):
    compare_case(layers, c)


def run_launch_shapes(layers):
    """one handle, sample counts that stride, then a single residual, then 4 workgroups and a tail, then one past the striding
    threshold: the ticket re-arms, the partials of the larger launch do not leak into the smaller one"""
    g = layers.registration(sample_case(1))
    for count in (2 * 262144 + 300, 1, 4 * 256 + 1, 262145):
        c = sample_case(count)
        _, ne = reference_of(c)
        got = g.normal_eq(*poses_of(c), c["samples"])
        check_normal_eq(got, ne, f"{count} samples")
        assert same_normal_eq(got, g.normal_eq(*poses_of(c), c["samples"])), count


def test_launch_shapes_on_one_handle(layers):
    run_launch_shapes(layers)


def run_begin_finish(layers):
    counts = (262145, 1, 1025, 257)
    cs = [sample_case(n) for n in counts]
    regs = [layers.registration(c) for c in cs]
    want = [g.normal_eq(*poses_of(c), c["samples"]) for g, c in zip(regs, cs)]
    for g, c in zip(regs, cs):
        g.normal_eq_begin(*poses_of(c), c["samples"])
    got = [g.normal_eq_finish() for g in reversed(regs)][::-1]
    for a, b, c in zip(want, got, cs):
        assert same_normal_eq(a, b), c["name"]
        check_normal_eq(b, reference_of(c)[1], c["name"])


def test_begin_back_to_back_finish_in_reverse(layers):
    run_begin_finish(layers)


def run_batches(layers):
    base = sample_case(1)
    regs, refs = [], []
    for k, count in enumerate((0, 1, 257, 262145, None, "empty")):
        c = dict(base if count in (0, None, "empty") else sample_case(count))
        c["pose_read"] = c["pose_read"] + k * np.array([0.01, -0.02, 0.01, 0.02])   # another pose per constraint
        if count == "empty":
            c["pts"], c["samples"] = np.zeros((0, 5), np.float32), None
        elif count == 0:
            c["samples"] = np.zeros(0, np.uint32)
        elif count is None:
            c["samples"] = None
        g = layers.registration(c)
        if c["samples"] is not None:
            g.set_samples(c["samples"])
        regs.append(g)
        refs.append((c, None if count in (0, "empty") else reference_of(c)[1]))

    own = {}

    def check(order):
        out = Registration.normal_eq_batch([regs[i] for i in order], [refs[i][0]["pose_ref"] for i in order], [refs[i][0]["pose_read"] for i in order])
        assert len(out) == len(order)
        for i, got in zip(order, out):
            c, ne = refs[i]
            if i not in own:   # the handle's own call: stored samples / all points
                own[i] = regs[i].normal_eq(*poses_of(c))
            assert same_normal_eq(got, own[i]), (order, i)
            if ne is None:
                assert not got[0].any() and not got[1].any() and got[2] == 0.0 and got[3] == 0, (order, i)
            else:
                check_normal_eq(got, ne, f"batch entry {i}")

    check([0, 1, 2, 3, 4, 5])
    check([0] + [(1, 2, 4, 5)[k % 4] for k in range(37)] + [3, 3])           # 40 constraints: above the 32-entry table of the first handle
    check([0, 4])                                                            # and a small batch on the grown table


def test_batches_with_empty_constraints_and_a_growing_table(layers):
    run_batches(layers)


def run_closed_form(eng):
    _, q, d, w = affine_inputs()
    lay = Layer(eng, float(map_ref.AFFINE_VS), capacity_blocks=64)
    lay.upload(*map_ref.affine_layer_arrays())
    for name, pf, pr, mapped in reg_cases.FINITE_POSES:
        if not mapped:
            continue
        pts = reg_cases.points_at(q, pf, pr, d, w)
        r, jf, jr = Registration(eng, RegPoints(eng, pts), lay, 0.25).evaluate(np.array(pf, np.float64), np.array(pr, np.float64))
        scale = len(pts) / float(np.sum(pts[:, 4].astype(np.float64)))   # exact in any order: multiples of 2^-10
        dev = closed_form_deviation(r / scale, np.concatenate([jf, jr], 1) / scale, pts, pf, pr)
        print(f"[closed form, engine] {name}: |dr|/w {dev[0]:.3g}  |dJ_t|/w {dev[1]:.3g}  |dJ_yaw|/w {dev[2]:.3g}")
        assert dev[0] <= TOL_R and dev[1] <= TOL_J_T and dev[2] <= TOL_J_YAW, (name, dev)


def test_evaluate_matches_the_closed_form_on_the_affine_layer(hip):
    run_closed_form(hip)


def run_reading_layers(eng):
    """readings that are not plain uploads: the ESDF of a masked submap-fuzz layer, and a layer whose pool filled in shuffled
    order while it grew from 4 blocks; the reference is fed each reading's own download()"""
    seed = next(s for s in range(200) if submap_cases.case(s, ("noise", "full", "salt", "grow"))[0] in (0.05, 0.1))
    c = submap_cases.case(seed, ("noise", "full", "salt", "grow"))
    grown = submap_cases.build_layer(eng, c)
    assert c[5]["capacity"] == 4 and len(c[1]) > 4
    rng = np.random.default_rng(seed)
    for what, reading in (("grown", grown), ("esdf", grown.esdf(**c[3]))):
        idx, vox = reading.download()
        q = reg_cases.generic_positions(rng, idx, c[0], 1000, margin=2.5 * c[0])
        pts = reg_cases.points_at(q, *reg_cases.SMALL_POSE, rng.uniform(-3 * c[0], 3 * c[0], len(q)), reg_cases.dyadic_weights(rng, len(q)))
        case = dict(name=what, pts=pts, pose_ref=np.array(reg_cases.SMALL_POSE[0]), pose_read=np.array(reg_cases.SMALL_POSE[1]), samples=None, ncc=0.25)
        rl = reg_ref.RefLayer(c[0], idx, vox)
        ev = reg_ref.evaluate(rl, pts, case["pose_ref"], case["pose_read"], None, 0.25)
        ne = reg_ref.normal_eq(rl, pts, case["pose_ref"], case["pose_read"], None, 0.25)
        print(f"[reading {what}] {len(idx)} blocks, {ne['n_corr']} of {len(pts)} with a correspondence")
        assert 0.3 * len(pts) <= ne["n_corr"] <= 0.9 * len(pts), what
        g = Registration(eng, RegPoints(eng, pts), reading, 0.25)
        check_evaluate(g.evaluate(*poses_of(case)), ev, True, what)
        check_normal_eq(g.normal_eq(*poses_of(case)), ne, what)


def test_esdf_and_grown_layers_as_readings(hip):
    run_reading_layers(hip)


def run_errors(layers):
    c = sample_case(257)
    g = layers.registration(c)
    n = len(c["pts"])
    g.set_samples(c["samples"][:10])
    g.stored_n = 11                                   # what the binding passes as n_res: not the size of the stored set
    with pytest.raises(CoxError):
        g.evaluate(*poses_of(c))
    with pytest.raises(CoxError):
        g.normal_eq(*poses_of(c))
    g.set_samples(None)
    with pytest.raises(CoxError):                     # an index past the point set
        g.normal_eq(*poses_of(c), np.array([0, n], np.uint32))
    with pytest.raises(CoxError):
        g.evaluate(*poses_of(c), np.array([n - 1, 2 ** 32 - 1], np.uint32))
    g.normal_eq_begin(*poses_of(c), c["samples"])
    with pytest.raises(CoxError):                     # one begin outstanding per handle
        g.normal_eq_begin(*poses_of(c), c["samples"])
    ev, ne = reference_of(c)
    check_normal_eq(g.normal_eq_finish(), ne, "after the refused calls")
    check_evaluate(g.evaluate(*poses_of(c), c["samples"]), ev, True, "after the refused calls")
    check_normal_eq(g.normal_eq(*poses_of(c), c["samples"]), ne, "after the refused calls")


def test_refused_calls_leave_the_handle_usable(layers):
    run_errors(layers)
