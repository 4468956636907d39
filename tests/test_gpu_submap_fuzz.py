"""Differential fuzz of finishSubmap() on the GPU (cox_submap.hip, the sampler of cox_reg.hip) over the seeded layers of
tests/submap_cases.py: sparse / disconnected / corner-touching block sets, shuffled and grown pools, merged layers, negative
indices, observation masks and every ESDF band configuration.

Per seed: HIP against the oracle bit for bit (ESDF words, isosurface points and their three counts, box, sampler draws for
three seeds) AND HIP against the numpy references of tests/submap_ref.py directly, so that a defect the oracle shares still
fails; then the server's configured constraint on a fuzzed pair (isosurface points of this case against the ESDF of the next
one's reading submap and of its own, drawn samples) with the bars of tests/test_gpu_submap.py.

COX_FUZZ_SEEDS=N widens the sweep (the convention of tests/test_gpu_projective_fuzz.py)."""
import os
import zlib

import numpy as np
import pytest

import reg_ref
import submap_cases
from coxgraph_amd.capi import Layer, RegPoints, Registration
from test_reg_ref_cpu import check_evaluate
from test_submap_ref_cpu import SAMPLER_SEEDS, ref_mesh, run_case  # noqa: F401  (ref_mesh is a module fixture)

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get("COX_FUZZ_SEEDS", "32"))


def oracle_twin(oracle, layer):
    """the same layer on the oracle, from the HIP layer's own download"""
    idx, vox = layer.download()
    twin = Layer(oracle, layer.voxel_size, capacity_blocks=max(64, len(idx)))
    if len(idx):
        twin.upload(idx, vox)
    return twin


def compare_engines(hip, oracle, lh, lo, esdf_cfg, iso_cfg, name=""):
    """HIP vs oracle, bit for bit -> (HIP points, oracle points, HIP ESDF, oracle ESDF)"""
    eh, eo = lh.esdf(**esdf_cfg), lo.esdf(**esdf_cfg)
    (ih, vh), (io, vo) = eh.download(), eo.download()
    assert np.array_equal(ih, io) and np.array_equal(vh, vo), (name, int((vh != vo).sum()))
    bh, bo = lh.surface_obb(), lo.surface_obb()
    assert bh[2] == bo[2] and np.array_equal(bh[0].view(np.uint32), bo[0].view(np.uint32)) and np.array_equal(bh[1].view(np.uint32), bo[1].view(np.uint32)), name
    ph, po = RegPoints.from_isosurface(hip, lh, **iso_cfg), RegPoints.from_isosurface(oracle, lo, **iso_cfg)
    assert (ph.n_mesh_vertices, ph.n_connected_vertices, ph.n) == (po.n_mesh_vertices, po.n_connected_vertices, po.n), name
    assert np.array_equal(ph.download().view(np.uint32), po.download().view(np.uint32)), name
    if po.n:
        gh, go = Registration(hip, ph, lh), Registration(oracle, po, lo)
        for seed in SAMPLER_SEEDS:
            gh.draw_samples(max(1, int(0.3 * po.n)), seed)
            go.draw_samples(max(1, int(0.3 * po.n)), seed)
            assert np.array_equal(gh.get_samples(), go.get_samples()), (name, seed)
    return ph, po, eh, eo


def check_pair(hip, oracle, ph, po, readings, name):
    """evaluate + normal_eq of the points against each (label, HIP ESDF, oracle ESDF), with drawn samples; the bars are those
    of tests/test_gpu_submap.py::test_explicit_to_implicit_registration_matches_oracle, its floor on the non-zero residuals
    (more than a fifth of the samples) included"""
    n_res = max(1, int(0.3 * po.n))
    pr, pd = np.zeros(4), np.array([0.05, -0.03, 0.02, np.radians(1.0)])
    for what, eh, eo in readings:
        gh, go = Registration(hip, ph, eh), Registration(oracle, po, eo)
        gh.draw_samples(n_res, 42)
        go.draw_samples(n_res, 42)
        a, b = gh.evaluate(pr, pd), go.evaluate(pr, pd)
        print(f"[pair {name} / {what}] {n_res} samples, {np.count_nonzero(b[0])} non-zero residuals")
        assert np.count_nonzero(b[0]) > 0.2 * n_res, (name, what, np.count_nonzero(b[0]), n_res)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (name, what)
        Hh, bh, ch, nh = gh.normal_eq(pr, pd)
        Ho, bo, co, no = go.normal_eq(pr, pd)
        assert nh == no and np.allclose(Hh, Ho, rtol=1e-9, atol=1e-9 * np.abs(Ho).max()) and abs(ch - co) <= 1e-9 * max(1.0, co), (name, what)
        # and against the numpy restatement of the cost (tests/reg_ref.py), at a seeded pose of this pair the oracle
        # comparison does not visit: yaw anywhere, up to two voxels of translation.  The isosurface weights are arbitrary
        # floats, so only the order of their sum can differ: check_evaluate's (n + 2) 2^-53 |value|
        rng = np.random.default_rng(zlib.crc32(f"{name} {what}".encode()))
        pd2 = np.concatenate([rng.uniform(-2, 2, 3) * eh.voxel_size, rng.uniform(-np.pi, np.pi, 1)])
        ev = reg_ref.evaluate(reg_ref.RefLayer(eh.voxel_size, *eh.download()), ph.download(), pr, pd2, gh.get_samples())
        print(f"[pair {name} / {what}] reference at yaw {pd2[3]:+.2f}: {int(ev['has'].sum())} of {n_res} with a correspondence")
        check_evaluate(gh.evaluate(pr, pd2), ev, False, (name, what, "reg_ref"))


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_fuzz_finish_submap(hip, oracle, ref_mesh, seed):  # noqa: F811
    c = submap_cases.case(seed)
    name = f"seed {seed}"
    lh = run_case(hip, c, ref_mesh, name)                 # HIP against the numpy references
    lo = oracle_twin(oracle, lh)
    ph, po, eh_own, eo_own = compare_engines(hip, oracle, lh, lo, c[3], c[4], name)
    if po.n == 0:
        return
    # explicit-to-implicit on a fuzzed pair: these points against the ESDF of a reading submap built over the same blocks
    # (submap_cases.reading_case) and against this case's own ESDF
    c2 = submap_cases.reading_case(c, (seed + 1) % N_SEEDS)
    rh = submap_cases.build_layer(hip, c2)
    ro = oracle_twin(oracle, rh)
    check_pair(hip, oracle, ph, po, (("reading", rh.esdf(**c2[3]), ro.esdf(**c2[3])), ("own", eh_own, eo_own)), name)


@pytest.mark.parametrize("seed,family", submap_cases.DIAGONAL_HALO_CASES, ids=[f[1] for _, f in submap_cases.DIAGONAL_HALO_CASES])
def test_diagonal_halo_families_propagate(hip, oracle, ref_mesh, seed, family):  # noqa: F811
    """Blocks touching at edges / corners only, with a band that must propagate: run_case asserts >= 1000 propagated voxels,
    5 % of them negative."""
    c = submap_cases.case(seed, family, propagating=True)
    assert c[5]["propagates"] and c[5]["negative_share"]
    lh = run_case(hip, c, ref_mesh, family[1])
    compare_engines(hip, oracle, lh, oracle_twin(oracle, lh), c[3], c[4], family[1])
