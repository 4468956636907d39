"""The C ABI of include/coxgraph_hip_depthfuse.h as far as it goes without a GPU: exported symbols, the defaults and the layouts of
the two structures against tests/depthfuse_ref.py, the device check, and the candidate box (a host computation, cox_selftest_depthfuse_box) against the box of
blocks the rule's steps 2-3 can reach.  DESIGN.md section 7m."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import depthfuse_ref as dr
from coxgraph_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cox_depthfuse_config_default", "cox_depthfuse_create", "cox_depthfuse_destroy", "cox_depthfuse_integrate",
           "cox_depthfuse_integrate_dev", "cox_depthfuse_last_stats", "cox_depthfuse_pool_order", "cox_depthfuse_sync"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def test_depthfuse_header_symbols_are_exported(hip):
    syms = _declared("coxgraph_hip_depthfuse.h")
    assert syms == SYMBOLS
    assert not [s for s in syms if not hasattr(hip.lib, s)]
    # the candidate box is for the tests only and is declared with the other self-test entries
    assert "cox_selftest_depthfuse_box" in _declared("coxgraph_hip_selftest.h") and hasattr(hip.lib, "cox_selftest_depthfuse_box")


def test_default_config_is_the_references(hip):
    c = capi.depthfuse_config(hip)
    for k, v in dr.DEFAULTS.items():
        got = getattr(c, k)
        assert got == (np.float32(v) if isinstance(v, float) else v), (k, got, v)
    assert [n for n, _ in capi.DepthFuseConfig._fields_] == list(dr.DEFAULTS)  # the fields of Config, in that order


@pytest.mark.parametrize("mine,ref", [(capi.DepthFuseConfig, dr.Config), (capi.DepthFuseStats, dr.Stats)], ids=["config", "stats"])
def test_structures_have_the_references_layout(mine, ref):
    assert C.sizeof(mine) == C.sizeof(ref)
    assert [(n, t) for n, t in mine._fields_] == [(n, t) for n, t in ref._fields_]
    for n, _ in ref._fields_:
        assert getattr(mine, n).offset == getattr(ref, n).offset and getattr(mine, n).size == getattr(ref, n).size, n
    assert C.sizeof(capi.DepthFuseConfig) == 40 and C.sizeof(capi.DepthFuseStats) == 56


def test_the_header_states_the_structures_in_that_order():
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_depthfuse.h")).read()
    for name, ref in (("cox_depthfuse_config", dr.Config), ("cox_depthfuse_stats", dr.Stats)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b(\w+);", body) == [n for n, _ in ref._fields_]


def test_create_fails_cleanly_without_a_gpu(hip):
    h = C.c_void_p()
    if hip.device_count() > 0:   # with a device the argument check is reached
        assert hip.fn("depthfuse_create")(None, None, C.byref(h)) == -1 and not h
        return
    fake = C.c_void_p(1)   # never dereferenced: the device check comes first
    assert hip.fn("depthfuse_create")(fake, None, C.byref(h)) == -2 and not h
    assert hip.fn("depthfuse_sync")(None) == -2
    assert hip.fn("depthfuse_integrate")(None, None, None, None, 1, 1, None) == -2
    assert hip.fn("depthfuse_integrate_dev")(None, None, None, None, 1, 1, None, None) == -2
    assert hip.fn("depthfuse_last_stats")(None, None) == -2
    assert hip.fn("depthfuse_pool_order")(None, None, C.c_uint64(0), None) == -2
    hip.fn("depthfuse_destroy", None)(None)


# ---- the candidate box (no GPU needed) -------------------------------------------------------------------------------------------
def _box(hip, voxel, T, w, h, K, **cfg):
    c = capi.depthfuse_config(hip, **cfg)
    T, K = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(K, np.float32)
    lo, dims = np.zeros(3, np.int32), np.zeros(3, np.uint32)
    st = hip.fn("selftest_depthfuse_box")(C.c_float(voxel), C.byref(c), capi._fp(T), C.c_int(w), C.c_int(h), capi._fp(K), capi._fp(lo), capi._fp(dims))
    return st, lo, dims.astype(np.int64)


def _reachable_blocks(voxel, T, w, h, K, min_depth, max_depth):
    """blocks with a voxel centre that passes steps 2-3 in float64, from every voxel of the reference's generous box"""
    T, K = np.asarray(T, np.float32).astype(np.float64), np.asarray(K, np.float32).astype(np.float64)
    R, t = dr.rotation_matrix(T[:4]), T[4:]
    ax = max(abs((-0.5 - K[2]) / K[0]), abs((w - 0.5 - K[2]) / K[0]))
    ay = max(abs((-0.5 - K[3]) / K[1]), abs((h - 0.5 - K[3]) / K[1]))
    reach, bs = max_depth * np.sqrt(1 + ax * ax + ay * ay), 16.0 * float(np.float32(voxel))
    lo, hi = np.floor((t - reach) / bs).astype(int) - 1, np.floor((t + reach) / bs).astype(int) + 1
    B = np.array([(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1)])
    lin = np.arange(4096)
    loc = np.stack([lin & 15, (lin >> 4) & 15, lin >> 8], 1)
    out = []
    for i in range(0, len(B), 1024):
        b = B[i:i + 1024]
        q = (((b[:, None, :] * 16 + loc[None]) + 0.5) * float(np.float32(voxel)) - t) @ R
        z = q[..., 2]
        with np.errstate(all="ignore"):
            u, v = K[0] * q[..., 0] / z + K[2], K[1] * q[..., 1] / z + K[3]
        ok = (z >= min_depth) & (z <= max_depth) & (u >= -0.5) & (u < w - 0.5) & (v >= -0.5) & (v < h - 0.5)
        out.append(b[ok.any(1)])
    return np.concatenate(out), len(B)


def _poses():
    rng = np.random.default_rng(11)
    out = [(f[0], dr.W, dr.H, f[3]) for f in dr.scene_frames(3)]
    sizes = [(48, 36), (1, 1), (2, 2), (1, 5), (47, 35)]
    for i in range(10):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, h = sizes[i % 5]
        K = dr.scaled_intrinsics(w, h) if i % 3 else np.array([30.0, 25.0, w + 40.0, -20.0], np.float32)  # principal point outside
        out.append((np.concatenate([q, rng.uniform(-3, 3, 3) - (200.0 if i % 4 == 0 else 0.0)]).astype(np.float32), w, h, K))
    return out


@pytest.mark.parametrize("k", range(13))
def test_candidate_box_holds_every_block_the_rule_can_reach(hip, k):
    T, w, h, K = _poses()[k]
    st, lo, dims = _box(hip, dr.VOXEL, T, w, h, K, **dr.BASE)
    assert st == 0
    reach, n_ref = _reachable_blocks(dr.VOXEL, T, w, h, K, dr.BASE["min_depth_m"], dr.BASE["max_depth_m"])
    assert len(reach) > 0
    assert np.all((reach >= lo) & (reach < lo + dims))
    assert int(np.prod(dims)) <= n_ref   # ... and is no larger than the reference's sphere of blocks
    # one block to spare on every side
    assert np.all(reach.min(0) - lo >= 1) and np.all(lo + dims - 1 - reach.max(0) >= 1)


def test_candidate_box_statuses(hip):
    T, _, _, K = dr.scene_frames(1)[0]
    big = 2 ** 21
    assert big == 1 << 21   # COX_DEPTHFUSE_MAX_CANDIDATES
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_depthfuse.h")).read()
    assert "#define COX_DEPTHFUSE_MAX_CANDIDATES (1u << 21)" in text
    # 1280 x 720, 10 m, 1 cm fits in every orientation tried here
    K720 = np.array([916.74, 916.74, 640.0, 360.0], np.float32)
    rng = np.random.default_rng(3)
    worst = 0
    for i in range(40):
        q = rng.normal(size=4) if i else np.array([1.0, 0, 0, 0])
        Tq = np.concatenate([q / np.linalg.norm(q), [0.3, -0.2, 0.1]]).astype(np.float32)
        st, lo, dims = _box(hip, 0.01, Tq, 1280, 720, K720, truncation_distance=0.03, max_depth_m=10.0)
        assert st == 0
        worst = max(worst, int(np.prod(dims)))
    print("largest 1280 x 720 / 10 m / 1 cm box:", worst)
    assert worst <= big
    # beyond the cap; beyond +-2^20 blocks; arguments
    assert _box(hip, 0.01, T, 1280, 720, K720, truncation_distance=0.03, max_depth_m=60.0)[0] == -1
    far = np.array(T, np.float32)
    far[4] = np.float32(1.6 * (2 ** 20 - 1))
    assert _box(hip, dr.VOXEL, far, dr.W, dr.H, K, **dr.BASE)[0] == -5
    far[4] = np.float32(-1.6 * 2 ** 20)
    assert _box(hip, dr.VOXEL, far, dr.W, dr.H, K, **dr.BASE)[0] == -5
    bad = np.array(T, np.float32)
    bad[5] = np.nan
    assert _box(hip, dr.VOXEL, bad, dr.W, dr.H, K, **dr.BASE)[0] == -1
    assert _box(hip, dr.VOXEL, T, 0, dr.H, K, **dr.BASE)[0] == -1
    assert _box(hip, dr.VOXEL, T, dr.W, dr.H, np.array([0.0, 30, 20, 20], np.float32), **dr.BASE)[0] == -1
    assert _box(hip, dr.VOXEL, T, dr.W, dr.H, np.array([30, np.inf, 20, 20], np.float32), **dr.BASE)[0] == -1
    for cfg in (dict(interpolation_scheme=4), dict(interpolation_scheme=-1), dict(truncation_distance=dr.VOXEL), dict(min_depth_m=0.0), dict(max_depth_m=np.inf),
                dict(max_depth_m=-1.0), dict(truncation_distance=np.nan)):
        assert _box(hip, dr.VOXEL, T, dr.W, dr.H, K, **{**dr.BASE, **cfg})[0] == -1, cfg
    # a truncation of one voxel is fine without drop-off
    assert _box(hip, dr.VOXEL, T, dr.W, dr.H, K, **dict(dr.BASE, truncation_distance=dr.VOXEL, use_weight_dropoff=0))[0] == 0
