"""The reference of the front-end tests (tests/frontend_ref.py) and their case generator (tests/frontend_cases.py), held to things they
were not derived from; no GPU needed.

  synth       on a synthetic frame with invalid pixels the reference returns synth's point list and colours bit for bit
  float64     the float32 formula is within three roundings of the same formula in float64
  order       mixed_sequence is a permutation and the inverse of voxblox's MixedThreadSafeIndex rule; pow2_above
  cases       the masks, values and sizes of the GPU tests are what their names say
  clean load  the library exports the two entries and they fail with COX_ERR_NO_DEVICE without a device
"""
import numpy as np
import pytest

from coxgraph_amd import synth

import frontend_cases as fc
import frontend_ref as fr


@pytest.fixture(scope="module")
def frame():
    T, pts, rgba, depth = synth.make_frame(2, nan_fraction=0.02)
    return pts, rgba, depth, fr.depth_to_points(depth, synth.frame_colors(), synth.INTRINSICS[(640, 480)])


def test_reference_is_synths_point_list_bit_for_bit(frame):
    pts, rgba, depth, (xyz, colours, tile_sums, n) = frame
    assert n == len(pts) < depth.size  # some pixels are invalid
    assert xyz.dtype == np.float32 and np.array_equal(xyz.view(np.uint32), pts.view(np.uint32))
    assert colours.dtype == np.uint8 and np.array_equal(colours, rgba)
    assert len(tile_sums) == 150 and int(tile_sums.sum()) == n and int(tile_sums.max()) <= 2048
    assert int(tile_sums[0]) == int(fr.depth_valid(depth.reshape(-1)[:2048]).sum())
    no_colour = fr.depth_to_points(depth, None, synth.INTRINSICS[(640, 480)])
    assert np.array_equal(no_colour[0], xyz) and no_colour[1].shape == (n, 4) and not no_colour[1].any()


def test_float32_formula_is_three_roundings_from_float64(frame):
    """(u - cx), / fx and d * xn round once each, by at most 2^-24 relative: (1 + e)^3 - 1 < 4 e."""
    _, _, depth, (xyz, _, _, _) = frame
    want = fr.depth_to_points_f64(depth, synth.INTRINSICS[(640, 480)])
    assert want.shape == xyz.shape
    assert np.all(np.abs(xyz.astype(np.float64) - want) <= 4 * 2.0 ** -24 * np.abs(want))
    assert np.array_equal(xyz[:, 2].astype(np.float64), want[:, 2])  # z is the depth itself


def voxblox_mixed_index(seq, n):
    """voxblox MixedThreadSafeIndex::getNextIndexImpl: groups of 1024 points are visited in turn, the remainder in order."""
    number_of_groups = n // 1024
    if number_of_groups * 1024 <= seq:
        return seq
    group_num, position_in_group = seq % number_of_groups, seq // number_of_groups
    return group_num * 1024 + position_in_group


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 5000])
def test_mixed_sequence_inverts_the_reference_index_rule(n):
    seq = fr.mixed_sequence(np.arange(n), n)
    assert sorted(seq.tolist()) == list(range(n))  # a permutation
    for s in range(n):
        assert int(seq[voxblox_mixed_index(s, n)]) == s
    assert np.array_equal(fr.mixed_sequence(np.arange(n), n), [int(fr.mixed_sequence(i, n)) for i in range(n)])


def test_pow2_above_and_host_segment():
    assert [fr.pow2_above(n) for n in (0, 1, 2, 3, 4, 4095, 4096, 4757, 8191, 8192)] == [1, 2, 4, 4, 8, 4096, 8192, 8192, 8192, 16384]
    assert fr.pow2_above(0x7FFFFFFF) == fr.pow2_above(0x80000000) == fr.pow2_above(0xFFFFFFFF) == 0x80000000
    assert fr.pow2_above(4757) == fr.pow2_above(4096) != fr.pow2_above(4095)  # what the valid counts of the GPU tests straddle
    for n in range(0, 64):
        n16, tail = fr.host_segment(4 * n)
        assert 16 * n16 + 4 * tail == 4 * n and 0 <= tail < 4
    assert fr.host_segment(12) == (0, 3) and fr.host_segment(16) == (1, 0) and fr.host_segment(12 * 4757) == (3567, 3)
    a = np.arange(5, dtype=np.uint32)
    b = fr.copy_words(a)
    assert np.array_equal(a, b) and b is not a and not np.shares_memory(a, b)


def test_depth_rule_on_the_edge_values():
    d = np.array([[np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e-40, 1e30, 1.5]], np.float32)
    assert fr.depth_valid(d).tolist() == [[False] * 6 + [True] * 3]
    assert d[0, 6] > 0 and d[0, 6] < np.finfo(np.float32).tiny  # the denormal survived the conversion to float32
    K = (2.0, 4.0, 0.5, 0.25)
    xyz, colours, tile_sums, n = fr.depth_to_points(d, np.arange(36, dtype=np.uint8).reshape(9, 4), K)
    assert n == 3 and tile_sums.tolist() == [3] and colours[:, 0].tolist() == [24, 28, 32]
    assert np.array_equal(xyz[2], np.array([1.5 * (8 - 0.5) / 2, 1.5 * (0 - 0.25) / 4, 1.5], np.float32))
    assert np.array_equal(xyz[:, 2], d[0, 6:])
    # row-major order: the pixel index is v * w + u
    xyz2, _, _, _ = fr.depth_to_points(np.full((3, 2), 2.0, np.float32), None, (1.0, 1.0, 0.0, 0.0))
    assert xyz2[:, 0].tolist() == [0, 2, 0, 2, 0, 2] and xyz2[:, 1].tolist() == [0, 0, 2, 2, 4, 4]


def test_cases_are_what_they_say():
    shapes = {w * h for w, h in fc.SHAPES}
    assert {1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048 + 1} <= shapes and max(shapes) == 6145
    assert sorted(shapes - {6145})[-1] <= 5000 and set(fc.STRIDED_SHAPES) <= set(fc.SHAPES)
    for w, h in fc.SHAPES:
        n = w * h
        K = fc.intrinsics(w, h)
        assert K[0] != K[1] and K[2] != np.floor(K[2]) and K[3] != np.floor(K[3])
        for pattern in fc.PATTERNS:
            m = fc.valid_mask(pattern, n)
            if m is None:
                assert (pattern == "tile_edge" and n <= 2048) or (pattern == "tile_hole" and n <= 3 * 2048)
                continue
            d = fc.depth_image(w, h, m)
            assert d.shape == (h, w) and d.dtype == np.float32 and np.array_equal(fr.depth_valid(d).reshape(-1), m)
            want = {"all": n, "none": 0, "first": 1, "last": 1, "tile_edge": 2, "tile_hole": n - 2048}.get(pattern)
            assert want is None or int(m.sum()) == want
            if pattern == "random" and n > 100:
                assert 0.4 * n < m.sum() < 0.6 * n
    d = fc.depth_image(6145, 1, fc.valid_mask("tile_hole", 6145)).reshape(-1)
    assert fr.depth_to_points(d.reshape(1, -1), None, fc.intrinsics(6145, 1))[2].tolist() == [2048, 0, 2048, 1]
    assert (d == fc.DENORMAL).any() and (d == fc.HUGE).any()
    bad = d[2048:4096]
    assert np.isnan(bad).any() and (bad == np.inf).any() and (bad == -np.inf).any() and (bad == -1).any()
    assert ((bad == 0) & ~np.signbit(bad)).any() and ((bad == 0) & np.signbit(bad)).any()
    words = fc.colour_image(67, 71).view(np.uint32).reshape(-1)
    assert not (words == 0).any() and not (words == fc.SENTINEL).any()
    for groups in fc.COPY_GROUPS:
        S = groups * 256
        n16 = {fr.host_segment(4 * n)[0] for n in fc.copy_sizes(groups)}
        assert {0, 1, S - 1, S, S + 1, 4 * S - 1, 4 * S, 4 * S + 1} <= n16
        for near in (S - 1, S, S + 1, 4 * S - 1, 4 * S, 4 * S + 1):  # every tail at every one of them
            assert {fr.host_segment(4 * n)[1] for n in fc.copy_sizes(groups) if fr.host_segment(4 * n)[0] == near} == {0, 1, 2, 3}
        for n in fc.copy_sizes(groups):
            absent, shorter, longer = fc.second_sizes(n, groups)
            assert absent is None and shorter <= n < longer and (shorter < n or n == 0)
    # the valid counts straddle np2, the mixed order's group count and the tiles, under a bound that does none of it
    w, h = fc.SCENE_WH
    assert w * h == 4757 and max(fc.VALID_COUNTS) < w * h
    assert {fr.pow2_above(v) for v in (4095, 4096)} == {4096, 8192} and fr.pow2_above(w * h) == 8192
    assert {v >> 10 for v in fc.VALID_COUNTS} == {0, 1, 2, 3, 4} and (w * h) >> 10 == 4
    for V in fc.VALID_COUNTS:
        assert int(fr.depth_valid(fc.with_valid_count(fc.scene_depth(w, h), V, seed=1)).sum()) == V
    assert {fr.host_segment(12 * n)[1] for n in fc.ASYNC_COUNTS} == {1, 2, 3} and fr.host_segment(12)[0] == 0
    assert {fr.host_segment(4 * n)[1] for n in fc.ASYNC_COUNTS} == {1, 2, 3} and fr.host_segment(4 * 3)[0] == 0


def test_selftest_entries_fail_cleanly_without_a_device(hip):
    for name in ("selftest_depth_points", "selftest_copy_from_host"):
        assert hip.has(name), name
    if hip.device_count() > 0:
        pytest.skip("GPU present")
    m = fc.valid_mask("random", 9)
    for rgba in (fc.colour_image(9, 1), None):
        assert fc.run_depth_points(hip, fc.depth_image(9, 1, m), rgba, fc.intrinsics(9, 1)).status == fc.NO_DEVICE
    words = fc.seeded_words(7, 1)
    assert fc.run_copy(hip, words, None, 8)[0] == fc.NO_DEVICE
    assert fc.run_copy(hip, words, words[:3], 1)[0] == fc.NO_DEVICE
