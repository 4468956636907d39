"""The radix sort and the scans of cox_sort.hpp / cox_frontend.hpp, called directly and compared exactly with tests/sort_ref.py.

Every frame-level test sits on these primitives; here they are held to the contracts their header states, at the sizes where a
tiled multi-pass sort and a tiled scan go wrong (lane, wave-tile, tile, grid-cap and tile-doubling edges):

  * the output is the stable order by the covered bits (sort_ref.covered_keys) of the first n = min(d_n, n_max) pairs; values are
    the input indices, so stability is visible; a second value array travels with its pair
  * the result is in buffer passes & 1; with device-side bits and nbits == 0 nothing moves; surplus passes do not flip the parity
  * [n, n_max) of both buffers is never written; the digit totals are all zero after every sort; a workspace of tiles_cap rows
    is enough at every size (the entry keeps a guard behind the counts matrix and reports writes into it)
  * any n_hint is correct; pass0_counted equals running k_rs_hist; the hook runs in the last pass only, once per wanted pair
  * the scans: exclusive prefix sums modulo 2^32, the tail beyond n untouched, in place or not, with or without a total

All comparisons are exact.  The entries are those of include/coxgraph_hip_selftest.h (bindings: tests/sort_cases.py).
"""
import numpy as np
import pytest

import sort_cases as sc
import sort_ref as sr
from sort_cases import SENTINEL, SMALL_SIZES, U32

pytestmark = pytest.mark.gpu

HIST_CAP = 1024 * 2048 + 1  # the histogram grid is capped at 1024 workgroups: one accumulates several tiles into `acc`
LAST_UNDOUBLED = 4096 * 2048  # 8 388 608
FIRST_DOUBLED = LAST_UNDOUBLED + 1  # the tile doubles to 4096 elements, 16 rounds per wave
STRIDED = 10 * 2048 + 5  # with n_hint = 1 one workgroup strides over all eleven tiles in all three kernels
ONE_TWO_THREE = {11: (11, 20, 32), 12: (12, 23, 32)}  # widths of one-, two- and three-pass sorts


def make_aux(n_max, seed):
    return np.random.default_rng([seed, n_max]).integers(0, 1 << 31, max(n_max, 1), dtype=np.uint64).astype(U32)


def check_sort(r, keys, rb, nbits, base=0, extra=None, aux=None, by_properties=False):
    """Everything the header promises about one sort, against the reference."""
    assert r.status == 0
    n, n_max = r.n, r.n_max
    passes = sr.pass_layout(rb, nbits)[0]
    buf = passes & 1
    assert r.result_buffer == buf
    assert r.totals_nonzero == 0
    assert r.guard_touched == 0  # the sort stayed inside a workspace of tiles_cap rows
    k_in = keys[:n]
    k_out, v_out = r.k[buf][:n], r.v[buf][:n]
    if by_properties:
        assert sr.sort_violations(k_in, k_out, v_out, rb, nbits, base) == []
    else:
        order = sr.stable_order(k_in, rb, nbits, base)
        assert np.array_equal(v_out, order)
        assert np.array_equal(k_out, k_in[order])
    if extra is not None:
        assert np.array_equal(r.x[buf][:n], extra[:n][v_out])
    arrays = [r.k, r.v] + ([r.x] if extra is not None else [])
    for pair in arrays:  # the tails of both ping-pong buffers were never written
        for b in (0, 1):
            assert bool(np.all(pair[b][n:] == SENTINEL))
    if passes == 0:  # nothing moves
        for pair in arrays:
            assert bool(np.all(pair[1] == SENTINEL))
    if passes <= 1:  # buffer 0 is only read
        assert np.array_equal(r.k[0][:n], k_in) and np.array_equal(r.v[0][:n], np.arange(n, dtype=U32))
    if aux is not None:  # the hook ran in the last pass only, exactly once per wanted pair
        want_pos = np.full(max(n_max, 1), SENTINEL, U32)
        want_aux = np.full(max(n_max, 1), SENTINEL, U32)
        want_count = np.zeros(max(n_max, 1), U32)
        if passes:
            where = np.empty(n, U32)
            where[v_out] = np.arange(n, dtype=U32)  # final position of the pair with value v
            wanted = np.arange(0, n, 3)
            want_pos[wanted] = where[wanted]
            want_aux[wanted] = aux[wanted]
            want_count[wanted] = 1
        assert np.array_equal(r.hook_pos, want_pos)
        assert np.array_equal(r.hook_aux, want_aux)
        assert np.array_equal(r.hook_count, want_count)


# ---------------------------------------------------------------------------------------------------------------------------
# the sort, small sizes: every width, every key pattern
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rb,nbits", [(rb, nb) for rb in sc.WIDTHS for nb in sc.WIDTHS[rb]])
def test_sort_host_bits(hip, rb, nbits):
    for n in SMALL_SIZES:
        for pattern in sc.PATTERNS:
            keys = sc.make_keys(pattern, n, rb, nbits, 0, seed=11)
            check_sort(sc.run_sort(hip, keys, rb, nbits), keys, rb, nbits)


@pytest.mark.parametrize("rb,nbits,base", sc.layouts())
def test_sort_device_bits(hip, rb, nbits, base):
    """SortInfo{nbits, parity = 0, base} on the device; max_passes zero, one and two above the passes needed (at most
    kRsMaxPasses = 4): the surplus launches must be no-ops and must not flip the parity.  nbits == 0: nothing moves."""
    needed = sr.pass_layout(rb, nbits)[0]
    turn = 0
    for n in SMALL_SIZES:
        for pattern in sc.PATTERNS:
            keys = sc.make_keys(pattern, n, rb, nbits, base, seed=12)
            max_passes = min(4, max(needed, 1) + turn % 3)
            turn += 1
            r = sc.run_sort(hip, keys, rb, nbits, device_bits=True, base=base, max_passes=max_passes)
            check_sort(r, keys, rb, nbits, base)


@pytest.mark.parametrize("rb", [11, 12])
@pytest.mark.parametrize("device_bits", [False, True])
def test_sort_second_value_array(hip, rb, device_bits):
    """x0/x1 travel with the pairs; with and without them the key and value buffers are the same."""
    base = 9 if device_bits else 0
    for nbits in ONE_TWO_THREE[rb]:
        if base + nbits > 32:
            base = 0
        for n in SMALL_SIZES:
            for pattern in ("heavy", "all_ones_mixed", "random"):
                keys = sc.make_keys(pattern, n, rb, nbits, base, seed=13)
                extra = np.random.default_rng([13, n]).integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
                kw = dict(device_bits=device_bits, base=base, max_passes=4 if device_bits else None)
                r = sc.run_sort(hip, keys, rb, nbits, extra=extra, **kw)
                check_sort(r, keys, rb, nbits, base, extra=extra)
                plain = sc.run_sort(hip, keys, rb, nbits, **kw)
                check_sort(plain, keys, rb, nbits, base)
                for b in (0, 1):
                    assert np.array_equal(r.k[b], plain.k[b]) and np.array_equal(r.v[b], plain.v[b])


@pytest.mark.parametrize("rb", [11, 12])
@pytest.mark.parametrize("device_bits", [False, True])
def test_sort_pass0_counted_equals_hist(hip, rb, device_bits):
    """The counts and totals of pass 0 left in the workspace beforehand, the sort's own histogram launch skipped: the same buffers."""
    base = 1 if device_bits else 0
    sizes = SMALL_SIZES + (STRIDED,)
    for nbits in (7,) + ONE_TWO_THREE[rb] if rb == 11 else ONE_TWO_THREE[rb]:
        if base + nbits > 32:
            base = 0
        for n in sizes:
            for pattern in ("alternating", "heavy", "random"):
                keys = sc.make_keys(pattern, n, rb, nbits, base, seed=14)
                kw = dict(device_bits=device_bits, base=base, n_hint=1 if n == STRIDED else None)
                on = sc.run_sort(hip, keys, rb, nbits, pass0_counted=True, **kw)
                off = sc.run_sort(hip, keys, rb, nbits, **kw)
                check_sort(on, keys, rb, nbits, base)
                check_sort(off, keys, rb, nbits, base)
                for b in (0, 1):
                    assert np.array_equal(on.k[b], off.k[b]) and np.array_equal(on.v[b], off.v[b])
    # with a device-side count below the capacity as well
    keys = sc.make_keys("random", 3 * 2048 + 1, rb, 20, 0, seed=14)
    r = sc.run_sort(hip, keys, rb, 20, d_n=2049, pass0_counted=True, device_bits=device_bits)
    check_sort(r, keys, rb, 20)


@pytest.mark.parametrize("rb", [11, 12])
@pytest.mark.parametrize("device_bits", [False, True])
@pytest.mark.parametrize("n_passes", [1, 2, 3])
def test_sort_hook(hip, rb, device_bits, n_passes):
    """The test hook (wants every third value, records aux[val] and the position) on both paths, in one-, two- and three-pass
    sorts: hook_pos[v] is where the pair with value v ended up, hook_aux[v] == aux[v], everything else still the sentinel."""
    nbits = ONE_TWO_THREE[rb][n_passes - 1]
    assert sr.pass_layout(rb, nbits)[0] == n_passes
    base = 12 if device_bits and nbits + 12 <= 32 else 0
    for n in SMALL_SIZES + (STRIDED,):
        aux = make_aux(n, 15)
        for pattern in ("equal", "reversed", "heavy", "all_ones_mixed", "random"):
            keys = sc.make_keys(pattern, n, rb, nbits, base, seed=15)
            r = sc.run_sort(hip, keys, rb, nbits, aux=aux, device_bits=device_bits, base=base, max_passes=4 if device_bits else None,
                            n_hint=1 if n == STRIDED else None)
            check_sort(r, keys, rb, nbits, base, aux=aux)
    # a count below the capacity: values at and above n are never wanted; nbits == 0 on the device: the hook never runs
    keys = sc.make_keys("random", 2049, rb, nbits, base, seed=15)
    aux = make_aux(2049, 16)
    r = sc.run_sort(hip, keys, rb, nbits, aux=aux, d_n=683, device_bits=device_bits, base=base)
    check_sort(r, keys, rb, nbits, base, aux=aux)
    if device_bits:
        r = sc.run_sort(hip, keys, rb, 0, aux=aux, device_bits=True, base=base, max_passes=3)
        check_sort(r, keys, rb, 0, base, aux=aux)


# ---------------------------------------------------------------------------------------------------------------------------
# counts and hints
# ---------------------------------------------------------------------------------------------------------------------------
def count_variants(n_max):
    """d_n: absent, the capacity, one below, a third, zero, five above (clamps)."""
    return [None, n_max, max(n_max - 1, 0), n_max // 3, 0, n_max + 5]


@pytest.mark.parametrize("rb", [11, 12])
@pytest.mark.parametrize("device_bits", [False, True])
def test_sort_counts_and_hints(hip, rb, device_bits):
    """n = min(*d_n, n_max) wherever the count lives, and any hint is correct: n_hint = 1 (one workgroup strides over all tiles in
    all three kernels, eleven of them at 10 * 2048 + 5), n, and 1 << 21 (far more workgroups than tiles)."""
    nbits = 20 if rb == 11 else 23
    base = 9 if device_bits else 0
    for n_max in SMALL_SIZES + (STRIDED,):
        keys = sc.make_keys("heavy" if n_max % 2 else "random", n_max, rb, nbits, base, seed=17)
        for d_n in count_variants(n_max):
            n = n_max if d_n is None else min(d_n, n_max)
            for n_hint in (1, n, 1 << 21):
                r = sc.run_sort(hip, keys, rb, nbits, d_n=d_n, n_hint=n_hint, device_bits=device_bits, base=base)
                assert r.n == n
                check_sort(r, keys, rb, nbits, base)


@pytest.mark.parametrize("rb", [11, 12])
@pytest.mark.parametrize("device_bits", [False, True])
@pytest.mark.parametrize("widths", [(32, 7, 7), (32, 7, 32), (7, 32, 13)])
def test_sort_repeats_on_one_workspace(hip, rb, device_bits, widths):
    """Three sorts on one workspace whose totals were zeroed once, the width changing in between: a sort that left a digit total
    behind would shift the next one's output; the totals are zero at the end."""
    for n in SMALL_SIZES + (STRIDED,):
        keys = sc.make_keys("random", n, 11, 32, 0, seed=18)  # all 32 bits vary, whatever the last width is
        r = sc.run_sort(hip, keys, rb, widths[-1], repeat_nbits=widths, device_bits=device_bits, max_passes=4 if device_bits else None)
        check_sort(r, keys, rb, widths[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# the sort, large sizes: the histogram grid cap, the last undoubled size, the first doubled one
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large_keys():
    """[8 388 609] uniform 32-bit keys, shared and never written."""
    keys = np.random.default_rng(19).integers(0, 1 << 32, FIRST_DOUBLED, dtype=np.uint64).astype(U32)
    keys.setflags(write=False)
    return keys


@pytest.fixture(scope="module")
def large_aux():
    aux = make_aux(FIRST_DOUBLED, 19)
    aux.setflags(write=False)
    return aux


@pytest.mark.parametrize("device_bits", [False, True], ids=["host_bits", "device_bits"])
@pytest.mark.parametrize("rb", [11, 12])
@pytest.mark.parametrize("n", [HIST_CAP, LAST_UNDOUBLED, FIRST_DOUBLED])
def test_sort_large(hip, large_keys, large_aux, n, rb, device_bits):
    """RB = 11 sorts all 32 bits (three passes of 11); RB = 12 sorts 24 bits (two passes of the full 4096 digits), from bit 8 on the
    device path.  The keys are uniform over 32 bits, so with 24 bits they break "below 2^nbits" and the covered-bits rule decides.
    The hook is on at 8 388 609: its path for the rounds of a doubled tile (r >= kRsRounds) is reached nowhere else.  Verified by
    the four properties of sort_ref.sort_violations, not a host argsort."""
    nbits = 32 if rb == 11 else 24
    base = 8 if device_bits and rb == 12 else 0
    keys = large_keys[:n]
    aux = large_aux[:n] if n == FIRST_DOUBLED else None
    r = sc.run_sort(hip, keys, rb, nbits, aux=aux, device_bits=device_bits, base=base, max_passes=4 if device_bits else None)
    check_sort(r, keys, rb, nbits, base, aux=aux, by_properties=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the three-launch scan
# ---------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 1024 * 2048, 1024 * 2048 + 1, 4096 * 2048 + 1)  # the last three: the carry loop of
# k_scan_sums (more than 1024 tile sums) and the grid cap of 4096
FAR_HINT = 1 << 24


def check_scan(hip, x, *, d_n=None, n_hint=None, in_place=False, want_total=True):
    st, out, total = sc.run_scan(hip, x, d_n=d_n, n_hint=n_hint, in_place=in_place, want_total=want_total)
    assert st == 0
    n = len(x) if d_n is None else min(d_n, len(x))
    want, want_total_value = sr.exclusive_scan(x[:n])
    assert np.array_equal(out[:n], want)
    assert np.array_equal(out[n:], x[n:] if in_place else np.full(len(x) - n, SENTINEL, U32))  # the tail is untouched
    assert total == (want_total_value if want_total else SENTINEL)  # n == 0 writes a total of 0


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sizes(hip, n):
    inputs = sc.scan_inputs(n, 21)
    big = n >= 1024 * 2048
    for name in ("small", "wrap") if big else inputs:
        x = inputs[name]
        for n_hint in (1, n, FAR_HINT):
            for in_place, want_total in ((False, True), (True, False)) if big else ((False, True), (True, True), (False, False), (True, False)):
                check_scan(hip, x, n_hint=n_hint, in_place=in_place, want_total=want_total)


@pytest.mark.parametrize("n_max", SCAN_SIZES)
def test_scan_counts(hip, n_max):
    x = sc.scan_inputs(n_max, 22)["small"]
    for d_n in count_variants(n_max):
        for n_hint, in_place in ((None, False), (1, True)):
            check_scan(hip, x, d_n=d_n, n_hint=n_hint, in_place=in_place)


@pytest.mark.parametrize("n", [2049, 3 * 2048 + 1, 1024 * 2048 + 1, 4096 * 2048 + 1])
def test_scan_single_nonzero_at_tile_edges(hip, n):
    """One nonzero word right before, at and after a tile edge, at the edges of the carry loop and the grid cap, and last."""
    edges = (0, 1, 2047, 2048, 2049, 2 * 2048 - 1, 2 * 2048, 1024 * 2048 - 1, 1024 * 2048, 4096 * 2048 - 1, 4096 * 2048, n - 2, n - 1)
    for pos in sorted({p for p in edges if 0 <= p < n}):
        check_scan(hip, sc.single_nonzero(n, pos), n_hint=n if pos % 2 else 1, in_place=bool(pos % 3 == 0))


# ---------------------------------------------------------------------------------------------------------------------------
# the one-workgroup scans
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 1])
def test_scan_small(hip, n):
    """k_scan_small and k_scan_small2 over n = min(d_n, n_max) elements with n reached through d_n (n_max above it) and through
    n_max (d_n above it): both halves of k_scan_small2 equal two k_scan_small runs, and both equal the reference."""
    length = n + 9
    fam_a, fam_b = sc.scan_inputs(length, 23), sc.scan_inputs(length, 24)
    cases = [(fam_a[name], fam_b[other]) for name, other in (("zeros", "ones"), ("ones", "small"), ("small", "wrap"), ("wrap", "small"))]
    for pos in sorted({p for p in (0, 3, 4, 4095, 4096, n - 1) if 0 <= p < n}):
        cases.append((sc.single_nonzero(length, pos), sc.single_nonzero(length, n - 1 - pos, 7)))
    for a, b in cases:
        for n_max, d_n in ((n + 9, n), (n, n + 9), (n, n)):
            st, outs, totals = sc.run_scan_small(hip, a, b, n_max, d_n)
            assert st == 0
            for x, small, small2, t1, t2 in ((a, outs[0], outs[2], totals[0], totals[2]), (b, outs[1], outs[3], totals[1], totals[3])):
                want, want_total = sr.exclusive_scan(x[:n])
                assert np.array_equal(small[:n], want) and t1 == want_total
                assert np.array_equal(small2, small) and t2 == t1
                assert bool(np.all(small[n:] == SENTINEL))  # the tail is untouched
