"""Exact integer references for the primitives of coxgraph_amd/csrc/cox_sort.hpp and the one-workgroup scans of cox_frontend.hpp.

Pure numpy, integers only: every comparison made with these is exact.

The sort.  radix_sort_pairs<RB> splits the nbits key bits over `passes` digits of `width` bits (pass_layout), starting at bit `base`
of the key (0 on the host-bits path).  Each pass is a stable counting sort on one digit, so what the passes produce is the STABLE
order of the first n pairs by

    (key >> base) & (2^(passes * width) - 1)                                                       (covered_keys)

-- the bits the passes actually cover, which may reach above nbits.  That statement is exact for keys that keep the engine's rule
("below 2^nbits or all ones") and for keys that break it, so the tests need no special case for either.  A shift never reaches
32 (a pass runs only when pass * width < nbits and base + nbits <= 32), so a digit that sticks out above bit 31 reads zeros there,
exactly as the uint64 arithmetic below does.

The scans.  Exclusive prefix sums of u32 words modulo 2^32; the total is the full sum modulo 2^32.
"""
import numpy as np

U32 = np.uint32
MASK32 = 0xFFFFFFFF


def pass_layout(rb, nbits):
    """(passes, width) of a sort of nbits key bits with RB = rb: passes = ceil(nbits / rb) digits of equal width
    ceil(nbits / passes), at least 6 bits wide.  No passes at nbits == 0."""
    if nbits == 0:
        return 0, 0
    passes = -(-nbits // rb)
    width = max(6, -(-nbits // passes))
    return passes, width


def covered_keys(keys, rb, nbits, base=0):
    """What the sort orders by: the passes * width bits of the key from bit `base` up, as uint64."""
    passes, width = pass_layout(rb, nbits)
    k = np.asarray(keys).astype(np.uint64)
    return (k >> np.uint64(base)) & np.uint64((1 << (passes * width)) - 1)


def result_buffer(rb, nbits):
    """The ping-pong buffer that holds the result: every pass that runs flips it."""
    return pass_layout(rb, nbits)[0] & 1


def stable_order(keys, rb, nbits, base=0):
    """Input indices in output order (host argsort; for the small cases)."""
    return np.argsort(covered_keys(keys, rb, nbits, base), kind="stable")


def lsd_order(keys, rb, nbits, base=0):
    """The sort as the kernels run it: digit by digit from the lowest, one stable counting pass each (histogram, exclusive
    prefix, placement in input order).  Returns input indices in output order."""
    passes, width = pass_layout(rb, nbits)
    keys = np.asarray(keys).astype(np.uint64)
    order = np.arange(len(keys), dtype=np.int64)
    for p in range(passes):
        digit = ((keys[order] >> np.uint64(base + p * width)) & np.uint64((1 << width) - 1)).astype(np.int64)
        counts = np.bincount(digit, minlength=1 << width)
        start = np.concatenate(([0], np.cumsum(counts)[:-1]))
        placed = np.empty_like(order)
        seen = np.zeros(1 << width, np.int64)
        for i, d in enumerate(digit):  # input order: the pass is stable
            placed[start[d] + seen[d]] = order[i]
            seen[d] += 1
        order = placed
    return order


def sort_violations(keys_in, keys_out, vals_out, rb, nbits, base=0):
    """The four properties that together say "keys_out / vals_out is the stable sort of keys_in with values arange(n)", without a
    host argsort.  Returns the list of the properties that do NOT hold (empty: the output is right).

      sorted       covered keys of the output are non-decreasing
      permutation  vals_out is a permutation of 0..n-1 (values are input indices)
      pairs        keys_out == keys_in[vals_out]: every key travelled with its value
      stable       inside every run of equal covered keys, vals_out increases

    Equivalence with np.argsort(kind="stable"): `permutation` and `pairs` make the output a reordering of the input pairs;
    `sorted` makes it an ordering by covered key; among the orderings by covered key the stable one is the only one in which
    equal keys appear by increasing input index, which is `stable`.  Conversely the stable argsort has all four."""
    keys_in, keys_out, vals_out = np.asarray(keys_in), np.asarray(keys_out), np.asarray(vals_out)
    n = len(keys_in)
    bad = []
    if len(keys_out) != n or len(vals_out) != n:
        return ["permutation"]
    ck = covered_keys(keys_out, rb, nbits, base)
    if n > 1 and not bool(np.all(ck[:-1] <= ck[1:])):
        bad.append("sorted")
    v = vals_out.astype(np.int64)
    is_perm = n == 0 or (int(v.max()) < n and bool(np.all(np.bincount(v, minlength=n) == 1)))
    if not is_perm:
        bad.append("permutation")
    elif not np.array_equal(keys_out, keys_in[v]):
        bad.append("pairs")
    if n > 1:
        same = ck[:-1] == ck[1:]
        if not bool(np.all(v[1:][same] > v[:-1][same])):
            bad.append("stable")
    return bad


def exclusive_scan(x):
    """(exclusive prefix sums, total) of u32 words modulo 2^32."""
    x = np.asarray(x, U32)
    inc = np.cumsum(x.astype(np.uint64), dtype=np.uint64) & np.uint64(MASK32)
    out = np.zeros(len(x), U32)
    out[1:] = inc[:-1].astype(U32)
    total = int(inc[-1]) if len(x) else 0
    return out, total
