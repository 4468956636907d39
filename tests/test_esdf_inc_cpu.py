"""The incremental ESDF rule (classify, raise, lower: DESIGN.md section 7l) as tests/esdf_inc_ref.py states it in numpy, held to
the from-scratch relaxation of tests/submap_ref.py bit for bit after every edit of a seeded sequence; and the C ABI of
include/coxgraph_hip_esdf.h as far as it goes without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import esdf_inc_ref
import submap_cases
import submap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


SEEDS = esdf_inc_ref.uploaded_seeds(12, True)


@pytest.mark.parametrize("seed", SEEDS)
def test_incremental_rule_equals_from_scratch_after_every_edit(seed):
    c = submap_cases.case(seed, propagating=True)
    voxel, idx_all, vox_all, cfg = c[0], c[1], c[2], c[3]
    inc = esdf_inc_ref.IncrementalEsdfRef(voxel, **cfg)
    first = esdf_inc_ref.start_half(c)[0]
    idx, vox = esdf_inc_ref.apply_upload(np.zeros((0, 3), np.int32), np.zeros((0, 4096, 3), np.uint32), idx_all[first], vox_all[first], 0)
    n_reset = 0
    for step in ("start",) + esdf_inc_ref.EDITS:
        if step != "start":
            idx, vox = esdf_inc_ref.apply_upload(idx, vox, *esdf_inc_ref.make_edit(step, c, idx, vox, seed))
        got = inc.update(idx, vox)
        want = submap_ref.esdf_ref(idx, vox, voxel, cfg["max_distance_m"], cfg["min_distance_m"], cfg["default_distance_m"], cfg["min_weight"])
        bad = got != want.words()
        assert not bad.any(), (seed, step, int(bad.sum()))
        assert inc.stats["rebuilt"] == 0
        if step != "start":
            n_reset += inc.stats["n_reset_voxels"]
    print(f"[seed {seed}] reset voxels over the sequence {n_reset}")
    assert n_reset > 0   # the sequence did take support away somewhere: the raise is not vacuous


def test_lost_blocks_rebuild():
    c = submap_cases.case(SEEDS[0], propagating=True)
    voxel, idx, vox, cfg = c[0], c[1], c[2], c[3]
    inc = esdf_inc_ref.IncrementalEsdfRef(voxel, **cfg)
    inc.update(idx, vox)
    got = inc.update(idx[1:], vox[1:])
    assert inc.stats["rebuilt"] == 1
    want = submap_ref.esdf_ref(idx[1:], vox[1:], voxel, cfg["max_distance_m"], cfg["min_distance_m"], cfg["default_distance_m"], cfg["min_weight"])
    assert np.array_equal(got, want.words())


def test_nan_weight_and_signed_zero_follow_the_batch():
    """a NaN weight is observed, a NaN distance free and negative, +-0 fixed: edits that put them in and take them out"""
    voxel, cfg = 0.1, dict(max_distance_m=2.0, min_distance_m=0.15, default_distance_m=2.0, min_weight=1e-6)
    idx = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
    x = (np.arange(32) + 0.5) * voxel
    d = np.clip(np.broadcast_to(x[None, None, :] - 1.37, (16, 16, 32)), -0.3, 0.3).astype(np.float32)
    vox = np.zeros((2, 4096, 3), np.uint32)
    for b in range(2):
        vox[b, :, 0] = np.ascontiguousarray(d[:, :, 16 * b:16 * b + 16]).reshape(-1).view(np.uint32)
        vox[b, :, 1] = np.float32(1.0).view(np.uint32)
    inc = esdf_inc_ref.IncrementalEsdfRef(voxel, **cfg)
    rng = np.random.default_rng(5)
    for step in range(4):
        if step:
            v = rng.integers(0, 4096, 40)
            vox[step % 2, v[:10], 1] = np.float32(np.nan).view(np.uint32)
            vox[step % 2, v[10:20], 0] = np.float32(np.nan).view(np.uint32)
            vox[step % 2, v[20:30], 0] = np.float32(0.0).view(np.uint32)
            vox[(step + 1) % 2, v[30:], 0] = np.float32(-0.0).view(np.uint32)
        got = inc.update(idx, vox)
        want = submap_ref.esdf_ref(idx, vox, voxel, cfg["max_distance_m"], cfg["min_distance_m"], cfg["default_distance_m"], cfg["min_weight"])
        assert np.array_equal(got, want.words()), step


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def test_esdf_header_symbols_are_exported(hip):
    syms = _declared("coxgraph_hip_esdf.h")
    assert syms == ["cox_esdf_create", "cox_esdf_destroy", "cox_esdf_invalidate", "cox_esdf_layer", "cox_esdf_update"]
    assert not [s for s in syms if not hasattr(hip.lib, s)]
    from coxgraph_amd import capi
    assert C.sizeof(capi.EsdfUpdateStats) == 80


def test_esdf_create_fails_cleanly_without_a_gpu(hip):
    h = C.c_void_p()
    if hip.device_count() > 0:   # with a device the argument check is reached
        assert hip.fn("esdf_create")(None, None, C.byref(h)) == -1 and not h
        return
    fake = C.c_void_p(1)   # never dereferenced: the device check comes first
    assert hip.fn("esdf_create")(fake, None, C.byref(h)) == -2 and not h
    assert hip.fn("esdf_update")(None, None) == -2
    assert hip.fn("esdf_invalidate")(None) == -2
