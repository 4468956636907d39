"""The collision checks' C ABI (include/coxgraph_hip_collide.h) and the test-side reference's hand-worked answers (rules S, L, T
and R of DESIGN.md section 7k) -- no GPU needed.

The hand-built layers are 0.1 m wall fields d = 4.0 - x; coordinates are binary fractions and sample_spacing is 0.25, so every
sample position is exact and every threshold is at least 1e-3 away from a sampled distance (asserted through min_margin)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import collide_ref as cr
from collide_ref import (C_CLEARED, C_DISTANCE, C_INVALID, C_OBSERVED, C_TRAVERSABLE, SEG_CLAMPED, SEG_FEASIBLE, SEG_GOAL, SEG_INVALID, SEG_TOO_LONG)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
Y = 0.75  # y = z of every sample: inside the one row of blocks, away from its faces
WALL = dict(collision_radius=0.5, sample_spacing=0.25, max_extension_range=0.0)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cr.build(tmp_path_factory.mktemp("collideref"))


@pytest.fixture(scope="module")
def wall(ref):
    idx, words = cr.wall_layer_arrays(3)
    return ref.layer(cr.VS, idx, words)


def _x(*xs):
    return np.array([[x, Y, Y] for x in xs], np.float32)


def _seg(L, xa, xb, **cfg):
    out = L.segments(_x(xa), _x(xb), **{**WALL, **cfg})
    assert out["min_margin"] >= 1e-3, out["min_margin"]
    return out["records"][0]


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "coxgraph_hip_collide.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cox_[a-z0-9_]+)\s*\(", text)))


def test_collide_header_symbols_are_exported(hip):
    syms = _declared_symbols()
    assert syms == ["cox_collide_config_default", "cox_collide_create", "cox_collide_destroy", "cox_collide_points", "cox_collide_points_dev",
                    "cox_collide_prune_dev", "cox_collide_segments", "cox_collide_segments_dev", "cox_collide_set_clearing_centre",
                    "cox_collide_set_group_size", "cox_collide_set_profiling", "cox_collide_stats", "cox_collide_trajectories",
                    "cox_collide_trajectories_dev", "cox_collide_tree", "cox_collide_tree_dev"]
    missing = [s for s in syms if not hasattr(hip.lib, s)]
    assert not missing, missing


def test_collide_defaults_are_the_planner_yaml(hip):
    from coxgraph_amd.capi import CollideConfig, collide_config
    c = collide_config(hip)
    assert C.sizeof(CollideConfig) == C.sizeof(cr.Config) == 48
    got = dict(collision_radius=c.collision_radius, collision_optimistic=c.collision_optimistic, clearing_radius=c.clearing_radius,
               clearing_centre=tuple(c.clearing_centre), sample_spacing=c.sample_spacing, max_samples=c.max_samples,
               max_extension_range=c.max_extension_range, crop=c.crop, crop_margin=c.crop_margin, crop_min_length=c.crop_min_length)
    exp = {k: (F(v) if isinstance(v, float) else v) for k, v in cr.DEFAULTS.items()}
    assert got == exp
    assert F(1.0) / F(20.0) == c.sample_spacing  # v_max / sampling_rate


def test_collide_entry_points_fail_cleanly(hip):
    """Without a GPU every call reports COX_ERR_NO_DEVICE before it looks at its arguments; with one, a NULL handle is
    COX_ERR_INVALID_ARG."""
    f = hip.fn
    want = -2 if hip.device_count() == 0 else -1
    h = C.c_void_p()
    n1, z = C.c_uint64(1), C.c_uint64(0)
    assert f("collide_create")(None, None, C.byref(h)) == want
    assert f("collide_set_clearing_centre")(None, None) == want
    assert f("collide_set_group_size")(None, C.c_int(7)) == want
    assert f("collide_set_profiling")(None, C.c_int(1)) == want
    assert f("collide_stats")(None, None, C.c_int(0)) == want
    assert f("collide_points")(None, None, n1, None, None) == want
    assert f("collide_points_dev")(None, None, n1, None, None, None) == want
    assert f("collide_segments")(None, None, None, n1, None) == want
    assert f("collide_segments_dev")(None, None, None, n1, None, None) == want
    assert f("collide_trajectories")(None, None, n1, None, z, None) == want
    assert f("collide_trajectories_dev")(None, None, n1, None, z, None, None) == want
    assert f("collide_prune_dev")(None, None, None, n1, n1, None, None) == want
    assert f("collide_tree")(None, None, None, n1, None, z, None, None) == want
    assert f("collide_tree_dev")(None, None, None, n1, None, z, None, None, None) == want
    f("collide_destroy", None)(None)


# ---- rule S ------------------------------------------------------------------------------------------------------------
def test_reference_sample_states_on_the_wall(wall):
    full = C_OBSERVED | C_DISTANCE
    q = np.concatenate([_x(1.125, 3.375, 3.625, 4.625, 0.02, 4.78, 4.85, -0.125),
                        np.array([[np.nan, Y, Y], [1.0, np.inf, Y], [1.0, Y, -np.inf], [3e6, Y, Y], [1.0, 0.02, Y]], np.float32)])
    exp = [full | C_TRAVERSABLE, full | C_TRAVERSABLE, full, full,
           C_OBSERVED,  # within half a voxel of the missing block -1: observed, no trilinear cell
           C_OBSERVED,  # ... of the missing block 3
           0, 0, C_INVALID, C_INVALID, C_INVALID, C_INVALID, C_OBSERVED]
    r = wall.points(q, **WALL)
    assert r["state"].tolist() == exp
    has = (r["state"] & C_DISTANCE) != 0
    assert np.isnan(r["distance"][~has]).all()
    assert np.max(np.abs(r["distance"][has] - (4.0 - q[has, 0].astype(np.float64)))) < 2e-6
    # unobserved samples: optimistic, and the clearing sphere (strictly inside)
    assert wall.points(q, **WALL, collision_optimistic=1)["state"].tolist()[6:8] == [C_TRAVERSABLE, C_TRAVERSABLE]
    c = wall.points(q, **WALL, clearing_radius=0.25, clearing_centre=(5.0, Y, Y))["state"].tolist()
    assert c[6] == (C_CLEARED | C_TRAVERSABLE) and c[7] == 0 and c[4] == C_OBSERVED
    edge = wall.points(_x(4.875), **WALL, clearing_radius=0.125, clearing_centre=(5.0, Y, Y), collision_optimistic=1)["state"].tolist()
    assert edge == [0]  # r == clearing_radius is outside; with a clearing sphere the optimistic flag is not consulted


def test_reference_removed_block_in_the_middle(ref):
    idx, words = cr.wall_layer_arrays(3)
    keep = [0, 2]
    L = ref.layer(cr.VS, idx[keep], words[keep])
    full = C_OBSERVED | C_DISTANCE | C_TRAVERSABLE
    r = L.points(_x(1.52, 1.58, 2.0, 3.22, 3.27), **WALL)
    assert r["state"].tolist() == [full, C_OBSERVED, 0, C_OBSERVED, full]
    # 1.125, 1.375 free; 1.625 lies in the removed block
    rec = _seg(L, 1.125, 3.125)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (8, 2, 0)
    assert _seg(L, 1.125, 3.125, collision_optimistic=1)["flags"] & SEG_FEASIBLE


# ---- rule L ------------------------------------------------------------------------------------------------------------
def test_reference_segment_through_free_blocked_and_unallocated_space(wall):
    # x_i = 1.125 + 0.25 i: d(3.375) = 0.625 is free, d(3.625) = 0.375 is blocked; 4.875 and 5.125 are unallocated
    for optimistic in (0, 1):
        rec = _seg(wall, 1.125, 5.125, collision_optimistic=optimistic)
        assert (rec["n_samples"], rec["first_blocked"]) == (16, 10)
        assert rec["flags"] == SEG_GOAL
        fl = F(4.0) * (F(9.0) / F(16.0)) - F(0.3)
        assert rec["free_length"] == fl and fl == F(2.25) - F(0.3)
        assert rec["goal"].tolist() == [F(1.125) + F(1.0) * fl, F(Y), F(Y)]
    # the segment starts in unallocated space: x_i = -0.875 + 0.25 i, observed from i = 4 on, free to its end
    rec = _seg(wall, -0.875, 3.125)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (16, 0, 0)
    assert rec["free_length"] == F(4.0) * (F(-1.0) / F(16.0)) - F(0.3) and np.isnan(rec["goal"]).all()
    rec = _seg(wall, -0.875, 3.125, collision_optimistic=1)
    assert (rec["first_blocked"], rec["flags"]) == (17, SEG_FEASIBLE | SEG_GOAL)
    assert rec["goal"].tolist() == [F(3.125), F(Y), F(Y)] and rec["free_length"] == F(4.0)
    # a clearing sphere about the start: distances 0, 0.25, 0.5, 0.75 -- 0.6 rescues three samples, 1.0 all four
    rec = _seg(wall, -0.875, 3.125, clearing_radius=0.6, clearing_centre=(-0.875, Y, Y))
    assert (rec["first_blocked"], rec["flags"]) == (3, 0)
    assert rec["free_length"] == F(4.0) * (F(2.0) / F(16.0)) - F(0.3)
    rec = _seg(wall, -0.875, 3.125, clearing_radius=1.0, clearing_centre=(-0.875, Y, Y))
    assert (rec["first_blocked"], rec["flags"]) == (17, SEG_FEASIBLE | SEG_GOAL)


def test_reference_crop_arithmetic(wall):
    # first_blocked = 0: the first term is negative
    rec = _seg(wall, 3.625, 2.625)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (4, 0, 0)
    assert rec["free_length"] == F(1.0) * (F(-1.0) / F(4.0)) - F(0.3)
    # first_blocked = 1: nothing but the margin
    rec = _seg(wall, 3.375, 4.375)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (4, 1, 0)
    assert rec["free_length"] == F(0.0) - F(0.3) and np.isnan(rec["goal"]).all()
    # free_length == crop_min_length: 4 * (3 / 16) - 0.25 = 0.5, and the comparison is strict
    rec = _seg(wall, 2.625, 6.625, crop_margin=0.25)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (16, 4, 0)
    assert rec["free_length"] == F(0.5) and np.isnan(rec["goal"]).all()
    rec = _seg(wall, 2.625, 6.625, crop_margin=0.25, crop_min_length=0.4375)
    assert rec["flags"] == SEG_GOAL and rec["goal"].tolist() == [F(3.125), F(Y), F(Y)]
    # against -x: the unit vector is -1
    rec = _seg(wall, 3.375, -0.625, crop_margin=0.25)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (16, 14, SEG_GOAL)  # x = -0.125 is unallocated
    assert rec["goal"].tolist() == [F(3.375) - (F(4.0) * (F(13.0) / F(16.0)) - F(0.25)), F(Y), F(Y)]
    # crop off: feasibility only
    rec = _seg(wall, 1.125, 5.125, crop=0)
    assert (rec["first_blocked"], rec["flags"]) == (10, 0) and np.isnan(rec["free_length"]) and np.isnan(rec["goal"]).all()
    rec = _seg(wall, 1.125, 3.125, crop=0)
    assert (rec["first_blocked"], rec["flags"]) == (9, SEG_FEASIBLE) and np.isnan(rec["goal"]).all()
    # a feasible segment shorter than crop_min_length gets no goal (the planner's early return)
    rec = _seg(wall, 1.125, 1.5)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (2, 3, SEG_FEASIBLE)
    assert rec["free_length"] == F(0.375) and np.isnan(rec["goal"]).all()


def test_reference_extension_clamp_zero_length_too_long_and_nan(wall):
    rec = _seg(wall, 1.0, 3.0, max_extension_range=1.5)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (6, 7, SEG_FEASIBLE | SEG_GOAL | SEG_CLAMPED)
    assert rec["goal"].tolist() == [F(2.5), F(Y), F(Y)] and rec["free_length"] == F(1.5)
    rec = _seg(wall, 1.0, 2.5, max_extension_range=1.5)  # len == range: not clamped
    assert rec["flags"] == SEG_FEASIBLE | SEG_GOAL
    # zero length: n = 1, two identical samples
    rec = _seg(wall, 1.0, 1.0)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (1, 2, SEG_FEASIBLE)
    assert rec["free_length"] == 0.0 and np.isnan(rec["goal"]).all()
    rec = _seg(wall, 3.625, 3.625)
    assert (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (1, 0, 0)
    # 16 intervals > max_samples 8: nothing is sampled
    out = wall.segments(_x(1.125), _x(5.125), **WALL, max_samples=8)
    rec = out["records"][0]
    assert out["n_samples"] == 0 and (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (16, 0, SEG_TOO_LONG)
    assert np.isnan(rec["free_length"]) and np.isnan(rec["goal"]).all()
    assert _seg(wall, 1.125, 5.125, max_samples=16)["first_blocked"] == 10
    for a, b in (([np.nan, Y, Y], [1.0, Y, Y]), ([1.0, Y, Y], [1.0, np.inf, Y]), ([-3e38, Y, Y], [3e38, Y, Y])):
        out = wall.segments(np.array([a], np.float32), np.array([b], np.float32), **WALL)
        rec = out["records"][0]
        assert out["n_samples"] == 0 and (rec["n_samples"], rec["first_blocked"], rec["flags"]) == (0, 0, SEG_INVALID)
        assert np.isnan(rec["free_length"]) and np.isnan(rec["goal"]).all()


# ---- rule T ------------------------------------------------------------------------------------------------------------
def test_reference_trajectories(wall):
    xyz = _x(1.0, 3.625, 1.0, 2.0, 3.0, 3.4, 3.7, 1.0)
    offsets = [0, 0, 1, 2, 2, 8]  # empty, one free point, one blocked point, empty, six points blocked at the fifth
    rec = wall.trajectories(offsets, xyz, **WALL)
    assert rec["n_samples"].tolist() == [0, 1, 1, 0, 6]
    assert rec["first_blocked"].tolist() == [0, 1, 0, 0, 4]
    assert rec["flags"].tolist() == [SEG_FEASIBLE, SEG_FEASIBLE, 0, SEG_FEASIBLE, 0]
    assert np.isnan(rec["free_length"]).all() and np.isnan(rec["goal"]).all()


# ---- rule R ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cr.TREES))
def test_reference_trees(ref, name):
    parent, feasible, keep = cr.TREES[name]
    assert ref.prune(parent, feasible).tolist() == keep
