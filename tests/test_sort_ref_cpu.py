"""The reference of the sort and scan tests (tests/sort_ref.py), held to things it was not derived from; no GPU needed.

  layout      pass_layout against the layouts worked out in the comments of cox_sort.hpp
  simulation  a digit-by-digit LSD sort with that layout equals the stable argsort on the covered bits
  properties  the four-property check that replaces the argsort in the large GPU cases rejects hand-made wrong outputs
  clean load  the library exports the three self-test entries and they fail with COX_ERR_NO_DEVICE without a device
"""
import numpy as np
import pytest

import sort_cases as sc
import sort_ref as sr


def test_layouts_worked_in_the_header():
    assert sr.pass_layout(12, 23) == (2, 12)  # 12 + 12
    assert sr.pass_layout(11, 20) == (2, 10)  # 10 + 10
    assert sr.pass_layout(11, 1) == (1, 6)    # at least 6 bits per pass
    assert sr.pass_layout(11, 32) == (3, 11)
    assert sr.pass_layout(12, 32) == (3, 11)
    assert sr.pass_layout(12, 24) == (2, 12) and sr.pass_layout(12, 25) == (3, 9)
    assert sr.pass_layout(11, 0)[0] == 0 and sr.pass_layout(12, 0)[0] == 0  # no passes
    for rb in (11, 12):
        for nbits in range(1, 33):
            passes, width = sr.pass_layout(rb, nbits)
            assert 1 <= passes <= 4 and 6 <= width <= rb
            assert passes * width >= nbits  # the digits cover the key bits ...
            assert (passes - 1) * width < nbits  # ... and every pass has a bit of them: none is surplus
            assert sr.result_buffer(rb, nbits) == passes % 2


def test_every_layout_of_the_gpu_tests_is_inside_the_contract():
    lay = sc.layouts()
    assert len(lay) == len(set(lay)) and {b for _, _, b in lay} == set(sc.BASES)
    for rb, nbits, base in lay:
        assert base + nbits <= 32
    assert {(rb, nb) for rb, nb, b in lay if b == 0} == {(rb, nb) for rb in sc.WIDTHS for nb in (0,) + sc.WIDTHS[rb]}


@pytest.mark.parametrize("rb", [11, 12])
def test_lsd_simulation_is_the_stable_sort_on_the_covered_bits(rb):
    for r, nbits, base in sc.layouts():
        if r != rb:
            continue
        for pattern in ("random", "heavy", "all_ones_mixed", "top_digit"):
            keys = sc.make_keys(pattern, 300, rb, nbits, base, seed=5)
            want = sr.stable_order(keys, rb, nbits, base)
            assert np.array_equal(sr.lsd_order(keys, rb, nbits, base), want), (rb, nbits, base, pattern)
            if nbits == 0:
                assert np.array_equal(want, np.arange(300))  # nothing moves
            assert sr.sort_violations(keys, keys[want], want.astype(np.uint32), rb, nbits, base) == []


def test_key_patterns_are_what_they_say():
    rb, nbits, base = 11, 20, 9
    passes, width = sr.pass_layout(rb, nbits)
    n = 4099
    ck = {p: sr.covered_keys(sc.make_keys(p, n, rb, nbits, base, 1), rb, nbits, base) for p in sc.PATTERNS}
    assert len(np.unique(ck["equal"])) == 1
    assert len(np.unique(ck["sorted"])) == n and np.all(np.diff(ck["sorted"].astype(np.int64)) > 0)
    assert np.all(np.diff(ck["reversed"].astype(np.int64)) < 0)
    assert len(np.unique(ck["alternating"])) == 2 and np.all(ck["alternating"][:-2] == ck["alternating"][2:])
    assert np.all(ck["top_digit"] >> np.uint64((passes - 1) * width) == (1 << width) - 1)
    assert np.all(ck["high_pass_only"] & np.uint64((1 << (passes - 1) * width) - 1) == 0) and len(np.unique(ck["high_pass_only"])) > 100
    assert np.max(np.bincount(ck["heavy"].astype(np.int64))) > n // 16
    ones = sc.make_keys("all_ones_mixed", n, rb, nbits, base, 1) == sc.ALL_ONES
    assert n // 8 < ones.sum() < n // 2
    assert np.all(ck["random"] < (1 << nbits))
    low = sc.make_keys("random", n, rb, nbits, base, 1) & ((1 << base) - 1)
    assert len(np.unique(low)) > 100  # bits below base vary: the sort must ignore them


def test_property_check_rejects_wrong_outputs():
    rb, nbits = 11, 13
    keys = sc.make_keys("heavy", 500, rb, nbits, 0, seed=3)
    order = sr.stable_order(keys, rb, nbits)
    vals = order.astype(np.uint32)
    assert sr.sort_violations(keys, keys[order], vals, rb, nbits) == []
    ck = sr.covered_keys(keys[order], rb, nbits)
    # two neighbours with equal keys swapped: still sorted, still a permutation, pairs intact -- only stability sees it
    j = int(np.flatnonzero(ck[:-1] == ck[1:])[0])
    v = vals.copy()
    v[[j, j + 1]] = v[[j + 1, j]]
    assert sr.sort_violations(keys, keys[v], v, rb, nbits) == ["stable"]
    # a duplicated value (and so a missing one)
    v = vals.copy()
    v[7] = v[8]
    assert "permutation" in sr.sort_violations(keys, keys[order], v, rb, nbits)
    # one misplaced element: a pair moved from the front to the back, keys travelling with values
    o = np.concatenate((order[1:], order[:1]))
    assert ck[0] != ck[-1]
    assert "sorted" in sr.sort_violations(keys, keys[o], o.astype(np.uint32), rb, nbits)
    # a key that did not travel with its value
    k = keys[order].copy()
    k[j], k[-1] = k[-1], k[j]
    assert "pairs" in sr.sort_violations(keys, k, vals, rb, nbits)
    # a value out of range, an output of the wrong length
    v = vals.copy()
    v[0] = 500
    assert "permutation" in sr.sort_violations(keys, keys[order], v, rb, nbits)
    assert sr.sort_violations(keys, keys[order][:-1], vals[:-1], rb, nbits) != []
    # bits the passes do not cover are not sorted on: with base = 3 an order by the whole key is wrong, the covered order right
    keys = sc.make_keys("random", 400, rb, 7, 3, seed=4)
    whole = np.argsort(keys, kind="stable")
    assert sr.sort_violations(keys, keys[whole], whole.astype(np.uint32), rb, 7, 3) == ["stable"]


def test_scan_reference():
    out, total = sr.exclusive_scan(np.array([], np.uint32))
    assert len(out) == 0 and total == 0
    out, total = sr.exclusive_scan(np.array([5, 0, 7], np.uint32))
    assert out.tolist() == [0, 5, 5] and total == 12
    out, total = sr.exclusive_scan(np.full(5, 0xFFFFFFFF, np.uint32))  # wraps modulo 2^32: k * (2^32 - 1) = -k
    assert out.tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC] and total == 0xFFFFFFFB
    x = sc.scan_inputs(5000, 2)["small"]
    out, total = sr.exclusive_scan(x)
    for i in (0, 1, 2, 2047, 2048, 4999):
        assert int(out[i]) == int(x[:i].sum(dtype=np.uint64))
    assert total == int(x.sum(dtype=np.uint64))


def test_selftest_entries_fail_cleanly_without_a_device(hip):
    for name in ("selftest_sort", "selftest_scan", "selftest_scan_small"):
        assert hip.has(name), name
    if hip.device_count() > 0:
        pytest.skip("GPU present")
    keys = sc.make_keys("random", 100, 11, 20, 0, seed=1)
    for kw in (dict(), dict(device_bits=True, base=3), dict(aux=np.arange(100, dtype=np.uint32), extra=keys, d_n=50)):
        assert sc.run_sort(hip, keys, 11, 20, **kw).status == sc.NO_DEVICE
    assert sc.run_scan(hip, keys)[0] == sc.NO_DEVICE
    assert sc.run_scan_small(hip, keys, keys, 100, 100)[0] == sc.NO_DEVICE
