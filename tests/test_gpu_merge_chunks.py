"""The bundle merge (k_bundle_merge) at the chunk edges of its software pipeline.

A wave walks a bundle in chunks of 64 points; while the chain of one chunk runs, the points of the next chunk and the sorted values
of the chunk behind it are in flight (coxgraph_amd/csrc/cox_raygen.hpp).  So the shapes that can go wrong are bundle sizes around
one, two, three chunks and beyond, bundles that stop early (clearing bundles use their first point only and drop what is in flight),
the bundle at the very end of the sorted array (nothing may be read behind it), and bundle sets that are used again.

Clouds are designed in VISITING order with the helpers of test_gpu_bundle_bounds.py: every bundle has a voxel of its own, `model()`
derives the bundles from the visit list and each case asserts on the model that the sizes are what it claims.  The fused layer and
the frame statistics are compared with the CPU oracle bit for bit.  Every case runs with the constant point weight (whole chunks of
weight 1 take the closed form of the running weight) and with the 1 / z^2 weight (the running weight is summed point by point), and
with COX_GRID_MERGE=1, where one workgroup takes all tasks in turn (what a task leaves behind would meet the next one).
"""
import numpy as np
import pytest

from test_gpu_bundle_bounds import CLEAR, NAN, NEAR, PLAIN, check, model

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 449, 577]


def visits(bundles, seed, last=None, tail=()):
    """Visit list (class, voxel id per visit) of bundles [(class, size)]: bundle j lives in voxel j, the visits are shuffled.  `last`:
    the visits of that bundle follow all others, so its head is the frame's latest.  `tail`: classes of invalid visits behind all."""
    cls = np.concatenate([np.full(n, c, np.int64) for c, n in bundles])
    vid = np.concatenate([np.full(n, j, np.int64) for j, (_, n) in enumerate(bundles)])
    perm = np.random.default_rng(seed).permutation(len(cls))
    cls, vid = cls[perm], vid[perm]
    if last is not None:
        order = np.argsort(vid == last, kind="stable")
        cls, vid = cls[order], vid[order]
    if len(tail):
        cls = np.concatenate([cls, np.asarray(tail, np.int64)])
        vid = np.concatenate([vid, np.arange(len(tail)) % 50])
    return cls, vid


def sizes_of(m, c):
    return sorted(m["sizes"][m["head_cls"] == c].tolist())


@pytest.fixture(params=[1, 0], ids=["const_weight", "z_weight"])
def weight(request):
    return dict(use_const_weight=request.param)


@pytest.fixture(params=[None, "1"], ids=["grid_default", "grid_1"])
def grid(request, monkeypatch):
    """(the switches are read when an integrator is created: the oracle's ignores them)"""
    if request.param is not None:
        monkeypatch.setenv("COX_GRID_MERGE", request.param)


def test_sizes_around_chunk_edges_plain_and_clearing(hip, oracle, weight, grid):
    """Every size once as a plain bundle and once as a clearing bundle, in one frame of 4 742 points."""
    cls, vid = visits([(PLAIN, n) for n in SIZES] + [(CLEAR, n) for n in SIZES], seed=1)
    m = model(cls, vid)
    assert sizes_of(m, PLAIN) == SIZES and sizes_of(m, CLEAR) == SIZES and m["n_valid"] == 2 * sum(SIZES)
    check(hip, oracle, [(cls, vid)], weight)


@pytest.mark.parametrize("c", [PLAIN, CLEAR], ids=["plain", "clearing"])
@pytest.mark.parametrize("invalid_behind", [False, True])
def test_largest_bundle_ends_the_sorted_array(hip, oracle, weight, grid, c, invalid_behind):
    """Bundles sort by (class, first visit), invalid points last.  The largest bundle has the frame's latest head (and the clearing
    class where there is one): its run ends the valid part of the sorted array -- which is the whole array (end == n_valid == n),
    or has NaN and too-near points behind it."""
    bundles = [(PLAIN, n) for n in SIZES[:-1]] + [(c, SIZES[-1])]
    tail = np.resize([NAN, NEAR], 90) if invalid_behind else ()
    cls, vid = visits(bundles, seed=2, last=len(bundles) - 1, tail=tail)
    m = model(cls, vid)
    assert m["sizes"][-1] == max(SIZES) == m["sizes"].max() and m["head_cls"][-1] == c and m["heads"][-1] == m["heads"].max()
    assert (m["head_cls"][:-1] == PLAIN).all()  # so the last bundle by head is the last one of the sorted array in either class
    assert m["n_valid"] == sum(SIZES) == len(cls) - len(tail)
    if invalid_behind:
        assert set(cls[m["n_valid"]:].tolist()) == {NAN, NEAR}
    check(hip, oracle, [(cls, vid)], weight)


def test_frame_without_a_valid_point(hip, oracle, weight, grid):
    """... then an ordinary frame on the same integrator."""
    none = (np.resize([NAN, NEAR], 300), np.arange(300) % 50)
    cls, vid = visits([(PLAIN, n) for n in SIZES[:8]] + [(CLEAR, 65)], seed=3)
    assert model(*none)["n_bundles"] == 0 and model(cls, vid)["n_bundles"] == 9
    check(hip, oracle, [none, (cls, vid)], weight)


def test_three_frames_in_a_row(hip, oracle, weight, grid):
    """Three different frames through one integrator, then the first again: every bundle set is used, and one of them twice.  The
    sizes move to other voxels and classes from frame to frame."""
    frames = []
    for k in range(3):
        s = SIZES[k:] + SIZES[:k]
        bundles = [(PLAIN if (j + k) % 2 else CLEAR, n) for j, n in enumerate(s)] + [(CLEAR if (j + k) % 2 else PLAIN, n) for j, n in enumerate(s[:6])]
        cls, vid = visits(bundles, seed=10 + k)
        m = model(cls, vid)
        assert sorted(m["sizes"].tolist()) == sorted(s + s[:6]) and {PLAIN, CLEAR} == set(m["head_cls"].tolist())
        frames.append((cls, vid))
    check(hip, oracle, frames + frames[:1], weight)
