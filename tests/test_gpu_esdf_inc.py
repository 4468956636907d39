"""The incremental ESDF (cox_esdf.hip, include/coxgraph_hip_esdf.h) against the batch on the same TSDF: after every update the
borrowed layer must hold exactly the words Layer.esdf(**cfg) returns -- compare_layers at tolerance 0 with bit-exact distances,
weights and flags.  Edit sequences are those of tests/esdf_inc_ref.py (the numpy statement of the rule is held to the
from-scratch relaxation in tests/test_esdf_inc_cpu.py).  No timing is asserted."""
import math
import os
import subprocess

import numpy as np
import pytest

import esdf_inc_ref
import submap_cases
from coxgraph_amd import synth
from coxgraph_amd.capi import CoxError, EsdfIntegrator, Integrator, Layer
from util import compare_layers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_SEEDS = esdf_inc_ref.uploaded_seeds(24, False)
# the pinhole stream as the projective integrator takes it (tests/test_gpu_history.py)
CAMERA = dict(sensor_horizontal_resolution=1280, sensor_vertical_resolution=960, sensor_vertical_field_of_view_degrees=360.0)


def same_as_batch(inc, tsdf, cfg, what=""):
    rep = compare_layers(inc.layer, tsdf.esdf(**cfg), tol=0.0)
    assert rep["bitexact_d"] and rep["bitexact_w"] and rep["n_diff_color"] == 0, (what, rep)
    return rep


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_edit_sequences(hip, seed):
    c = submap_cases.case(seed)
    voxel, idx_all, vox_all, cfg, meta = c[0], c[1], c[2], c[3], c[5]
    tsdf = Layer(hip, voxel, capacity_blocks=4 if meta["build"] == "grow" else 64)
    first = esdf_inc_ref.start_half(c)[0]
    tsdf.upload(idx_all[first], vox_all[first])
    inc = tsdf.esdf_integrator(**cfg)
    st = inc.update()
    assert st["rebuilt"] == 1 and st["n_blocks"] == len(first)
    same_as_batch(inc, tsdf, cfg, (seed, "start"))
    log = []
    for kind in esdf_inc_ref.EDITS:
        idx, vox, action = esdf_inc_ref.make_edit(kind, c, *tsdf.download(), seed)
        if action == 1:
            other = Layer(hip, voxel, capacity_blocks=64)
            other.upload(idx, vox)
            tsdf.merge_from(other)
        else:
            tsdf.upload(idx, vox, action)
        st = inc.update()
        log.append((kind, st["n_dirty_blocks"], st["n_swept_blocks"], st["n_raise_sweeps"], st["n_lower_sweeps"], st["n_reset_voxels"]))
        assert st["rebuilt"] == 0, (seed, kind, st)
        same_as_batch(inc, tsdf, cfg, (seed, kind, st))
    print(f"[seed {seed}] {meta['blocks']}/{meta['mask']}/{meta['build']} cfg {cfg}: (edit, dirty, swept, raise, lower, reset) {log}")


@pytest.mark.parametrize("method,voxel", [("merged", 0.10), ("merged", 0.05), ("projective", 0.10), ("projective", 0.05)])
def test_fused_stream_with_frames_in_flight(hip, method, voxel):
    cfgs = [dict(max_distance_m=4.0, min_distance_m=0.1), dict(max_distance_m=2.0, min_distance_m=1.5 * voxel)]
    tsdf = Layer(hip, voxel, capacity_blocks=256)
    ov = synth.integrator_overrides(voxel)
    if method == "projective":
        ov.update(CAMERA)
    integ = Integrator(hip, tsdf, hip.default_config(**ov), method)
    incs = [tsdf.esdf_integrator(**cfg) for cfg in cfgs]   # two integrators with different configurations on one TSDF
    n_updates = 0
    for i, t in enumerate(range(0, 150, 10)):
        T, pts, rgba, _ = synth.make_frame(t)
        integ.integrate_points(T, pts[::4], rgba[::4])
        if i % 3 != 2:
            continue
        for inc, cfg in zip(incs, cfgs):   # no sync: the frame is still in flight
            st = inc.update()
            rep = same_as_batch(inc, tsdf, cfg, (method, voxel, t, st))
            assert st["rebuilt"] == (1 if n_updates == 0 else 0) and rep["blocks"] == st["n_blocks"] > 0
            print(f"[{method} {voxel} frame {t} max {cfg['max_distance_m']}] {st}")
        n_updates += 1
    assert n_updates == 5
    # readers take the incremental layer as they take the batch's
    rng = np.random.default_rng(7)
    pts = rng.uniform([-1.0, -3.0, 0.0], [4.5, 3.0, 3.0], (1000, 3)).astype(np.float32)
    a, b = pts[:200], pts[200:400]
    for inc, cfg in zip(incs, cfgs):
        batch = tsdf.esdf(**cfg)
        qa, qb = inc.layer.query(pts, gradient=True), batch.query(pts, gradient=True)
        assert np.count_nonzero(qb["status"]) > 100
        for k in qa:
            assert np.array_equal(qa[k].view(np.uint8), qb[k].view(np.uint8)), k
        ra, rb = inc.layer.check_segments(a, b, collision_radius=0.3), batch.check_segments(a, b, collision_radius=0.3)
        print(f"[{method} {voxel}] values at {np.count_nonzero(qb['status'])} of 1000 points, {np.count_nonzero(rb['flags'] & 1)} of {len(rb['flags'])} segments feasible")
        assert len(rb["flags"]) == 200 and np.count_nonzero(rb["n_samples"]) > 0
        for k in ra:
            assert ra[k].tobytes() == rb[k].tobytes(), k


def plane_field(idx, voxel, z0, bump=0.0):
    cen = esdf_inc_ref._centres(np.asarray(idx), voxel)
    d = cen[..., 2] - z0 + bump * np.sin(3.0 * cen[..., 0]) * np.cos(2.0 * cen[..., 1])
    vox = np.zeros(d.shape + (3,), np.uint32)
    vox[..., 0] = np.clip(d, -3 * voxel, 3 * voxel).astype(np.float32).view(np.uint32)
    vox[..., 1] = np.float32(5.0).view(np.uint32)
    return vox


SLAB = np.array([[x, y, z] for z in range(3) for y in range(3) for x in range(8)], np.int32)
SLAB_CFG = dict(max_distance_m=0.5, min_distance_m=0.15)


def slab_layer(hip, voxel=0.10):
    tsdf = Layer(hip, voxel, capacity_blocks=128)
    tsdf.upload(SLAB, plane_field(SLAB, voxel, 2.37))
    return tsdf


def test_second_update_is_a_no_op(hip):
    tsdf = slab_layer(hip)
    inc = tsdf.esdf_integrator(**SLAB_CFG)
    st = inc.update()
    assert st["n_dirty_blocks"] == 72 and st["n_lower_sweeps"] > 0 and st["n_changed_voxels"] > 0
    before = inc.layer.download()
    st = inc.update()
    assert st["n_dirty_blocks"] == 0 and st["n_raise_sweeps"] == 0 and st["n_lower_sweeps"] == 0 and st["n_swept_blocks"] == 0, st
    assert st["n_new_blocks"] == 0 and st["n_reset_voxels"] == 0 and st["n_changed_voxels"] == 0 and st["rebuilt"] == 0, st
    after = inc.layer.download()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    same_as_batch(inc, tsdf, SLAB_CFG)


def test_an_edit_is_answered_locally(hip):
    """One block edited at the x = 0 end of an 8 x 3 x 3 slab.  An ESDF value depends on TSDF voxels within ceil(max / voxel) + 1
    voxels only, i.e. on blocks within Rb = ceil((ceil(max / voxel) + 1) / 16) blocks, and activation adds one ring: no block
    further than Rb + 1 (Chebyshev) from a dirty block may be visited."""
    voxel = 0.10
    tsdf = slab_layer(hip, voxel)
    inc = tsdf.esdf_integrator(**SLAB_CFG)
    inc.update()
    edited = np.array([[0, 1, 1]], np.int32)
    tsdf.upload(edited, plane_field(edited, voxel, 2.21, bump=0.08))
    st = inc.update()
    same_as_batch(inc, tsdf, SLAB_CFG, st)
    rb = math.ceil((math.ceil(SLAB_CFG["max_distance_m"] / voxel) + 1) / 16)
    assert rb == 1
    bound = int((np.abs(SLAB - edited[0]).max(axis=1) <= rb + 1).sum())
    assert bound == 27
    print(st)
    assert st["n_dirty_blocks"] == 1 and st["rebuilt"] == 0 and st["n_new_blocks"] == 0
    assert st["n_reset_voxels"] > 0 and st["n_raise_sweeps"] > 0 and st["n_lower_sweeps"] > 0   # support was taken away and found again
    assert 0 < st["n_swept_blocks"] <= bound, st


def test_clear_and_invalidate_rebuild(hip):
    voxel, cfg = 0.10, dict(max_distance_m=2.0, min_distance_m=0.15)
    tsdf = Layer(hip, voxel, capacity_blocks=256)
    integ = Integrator(hip, tsdf, hip.default_config(**synth.integrator_overrides(voxel)), "merged")
    inc = tsdf.esdf_integrator(**cfg)
    for t in (0, 10, 20):
        T, pts, rgba, _ = synth.make_frame(t)
        integ.integrate_points(T, pts[::4], rgba[::4])
    assert inc.update()["rebuilt"] == 1
    tsdf.clear()
    for t in (60, 70):
        T, pts, rgba, _ = synth.make_frame(t)
        integ.integrate_points(T, pts[::4], rgba[::4])
    st = inc.update()
    assert st["rebuilt"] == 1 and st["n_blocks"] > 0
    same_as_batch(inc, tsdf, cfg, st)
    first = inc.layer.download()
    inc.invalidate()
    st = inc.update()
    assert st["rebuilt"] == 1 and st["n_dirty_blocks"] > 0
    second = inc.layer.download()
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    same_as_batch(inc, tsdf, cfg, st)


def test_empty_single_block_and_grown_pool(hip):
    voxel, cfg = 0.10, dict(max_distance_m=2.0, min_distance_m=0.15, default_distance_m=1.0)
    tsdf = Layer(hip, voxel, capacity_blocks=4)
    inc = tsdf.esdf_integrator(**cfg)
    st = inc.update()                                   # an empty layer
    assert st["n_blocks"] == 0 and st["n_swept_blocks"] == 0
    assert same_as_batch(inc, tsdf, cfg)["blocks"] == 0
    tsdf.upload(SLAB[:1], plane_field(SLAB[:1], voxel, 0.77))
    st = inc.update()                                   # a single block
    assert st["n_blocks"] == 1 and st["n_new_blocks"] == 1
    same_as_batch(inc, tsdf, cfg)
    tsdf.upload(SLAB[1:3], plane_field(SLAB[1:3], voxel, 0.77))
    inc.update()
    tsdf.upload(SLAB[3:], plane_field(SLAB[3:], voxel, 0.77, bump=0.05))   # the TSDF's pool grows from 4 blocks, the ESDF's follows
    assert tsdf.capacity() >= 72
    st = inc.update()
    assert st["n_blocks"] == 72 and st["n_new_blocks"] == 69 and st["rebuilt"] == 0 and inc.layer.capacity() >= 72
    same_as_batch(inc, tsdf, cfg, st)
    clone = inc.layer.clone_to_device(0)                # the borrowed layer is an ordinary layer
    assert compare_layers(clone, inc.layer, tol=0.0)["bitexact_d"]


def test_borrowed_layer_refuses_use_after_close(hip):
    tsdf = slab_layer(hip)
    inc = EsdfIntegrator(hip, tsdf, **SLAB_CFG)
    inc.update()
    borrowed = inc.layer
    assert borrowed.n_blocks() == 72
    inc.close()
    for call in (borrowed.download, borrowed.n_blocks, lambda: borrowed.query(np.zeros((1, 3), np.float32))):
        with pytest.raises(CoxError):
            call()
    with pytest.raises(CoxError):
        inc.update()
    borrowed.close()
    with pytest.raises(CoxError):
        EsdfIntegrator(hip, tsdf, max_distance_m=-1.0)
    # the other way round: the TSDF closed under a live integrator
    inc = EsdfIntegrator(hip, tsdf, **SLAB_CFG)
    inc.update()
    tsdf.close()
    with pytest.raises(CoxError):
        inc.update()
    assert inc.layer.n_blocks() == 72   # what it had stays readable
    inc.close()


def test_cpp_incremental_esdf_on_the_gpu(hip, tmp_path):
    exe = str(tmp_path / "esdf_smoke")
    libdir = os.path.dirname(hip.path)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "esdf_smoke.cpp"),
                           "-L" + libdir, "-lcoxgraph_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
