"""Bindings of the self-test entries (include/coxgraph_hip_selftest.h) and the seeded inputs of the sort and scan tests.
Shared by tests/test_sort_ref_cpu.py (no GPU) and tests/test_gpu_sort_scan.py."""
import ctypes as C

import numpy as np

from sort_ref import pass_layout

U32 = np.uint32
SENTINEL = 0xDEADBEEF  # above every position, every aux word (< 2^31) and every value the tests use
ALL_ONES = 0xFFFFFFFF
NO_DEVICE = -2

SMALL_SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 1)  # lane, wave-tile and tile edges
WIDTHS = {11: (1, 6, 7, 11, 12, 13, 20, 22, 23, 32), 12: (12, 13, 23, 24, 25, 32)}
BASES = (0, 1, 9, 12)  # device-bits path only
PATTERNS = ("equal", "sorted", "reversed", "alternating", "top_digit", "high_pass_only", "heavy", "all_ones_mixed", "random")


def layouts():
    """Every (rb, nbits, base) the GPU tests sort with: base > 0 only where base + nbits <= 32, plus nbits == 0."""
    out = []
    for rb, widths in WIDTHS.items():
        for nbits in (0,) + widths:
            for base in BASES:
                if base + nbits <= 32:
                    out.append((rb, nbits, base))
    return out


class SortArgs(C.Structure):
    P = C.POINTER(C.c_uint32)
    _fields_ = [("rb", C.c_int32), ("n_max", C.c_uint32), ("use_d_n", C.c_int32), ("d_n", C.c_uint32), ("n_hint", C.c_uint32),
                ("bits_on_device", C.c_int32), ("nbits", C.c_uint32), ("base", C.c_uint32), ("max_passes", C.c_int32),
                ("pass0_counted", C.c_int32), ("hook", C.c_int32), ("repeat", C.c_int32), ("repeat_nbits", P),
                ("sentinel", C.c_uint32), ("pad0", C.c_uint32),
                ("keys", P), ("vals", P), ("extra", P), ("aux", P),
                ("k0", P), ("v0", P), ("x0", P), ("k1", P), ("v1", P), ("x1", P), ("hook_pos", P), ("hook_aux", P), ("hook_count", P),
                ("result_buffer", C.c_int32), ("totals_nonzero", C.c_uint32), ("guard_touched", C.c_uint32), ("pad1", C.c_uint32)]


def _ptr(a):
    return a.ctypes.data_as(SortArgs.P)


class SortResult:
    """Both ping-pong buffers in full, the buffer that holds the result, the hook's outputs, nonzero words left in totals, words
    written behind the counts matrix."""

    def __init__(self, status):
        self.status = status


def run_sort(hip, keys, rb, nbits, *, vals=None, extra=None, d_n=None, n_hint=None, device_bits=False, base=0, max_passes=None,
             pass0_counted=False, aux=None, repeat_nbits=None, device=0):
    """One cox_selftest_sort call.  keys: [n_max] u32; values default to the input indices.  d_n None: no device-side count.
    aux not None: the hook is on.  repeat_nbits: the widths of successive sorts on one workspace (the last one is returned)."""
    keys = np.ascontiguousarray(keys, U32)
    n_max = len(keys)
    vals = np.arange(n_max, dtype=U32) if vals is None else np.ascontiguousarray(vals, U32)
    a = SortArgs()
    a.rb, a.n_max = rb, n_max
    a.use_d_n, a.d_n = (0, 0) if d_n is None else (1, int(d_n))
    n = n_max if d_n is None else min(int(d_n), n_max)
    a.n_hint = n if n_hint is None else int(n_hint)
    a.bits_on_device, a.nbits, a.base = int(device_bits), nbits, base
    a.max_passes = (max(1, pass_layout(rb, nbits)[0]) if max_passes is None else max_passes) if device_bits else 0
    a.pass0_counted, a.hook, a.sentinel = int(pass0_counted), int(aux is not None), SENTINEL
    keep = [keys, vals]
    if repeat_nbits is not None:
        rn = np.ascontiguousarray(repeat_nbits, U32)
        keep.append(rn)
        a.repeat, a.repeat_nbits = len(rn), _ptr(rn)
    else:
        a.repeat = 1
    a.keys, a.vals = _ptr(keys), _ptr(vals)
    r = SortResult(0)
    r.n, r.n_max = n, n_max
    r.k, r.v, r.x = [np.zeros(n_max, U32) for _ in range(2)], [np.zeros(n_max, U32) for _ in range(2)], None
    a.k0, a.k1, a.v0, a.v1 = _ptr(r.k[0]), _ptr(r.k[1]), _ptr(r.v[0]), _ptr(r.v[1])
    if extra is not None:
        extra = np.ascontiguousarray(extra, U32)
        keep.append(extra)
        r.x = [np.zeros(n_max, U32) for _ in range(2)]
        a.extra, a.x0, a.x1 = _ptr(extra), _ptr(r.x[0]), _ptr(r.x[1])
    if aux is not None:
        aux = np.ascontiguousarray(aux, U32)
        assert len(aux) >= max(n_max, 1)
        keep.append(aux)
        r.hook_pos, r.hook_aux, r.hook_count = (np.zeros(max(n_max, 1), U32) for _ in range(3))
        a.aux, a.hook_pos, a.hook_aux, a.hook_count = _ptr(aux), _ptr(r.hook_pos), _ptr(r.hook_aux), _ptr(r.hook_count)
    r.status = hip.fn("selftest_sort")(C.c_int(device), C.byref(a))
    r.result_buffer, r.totals_nonzero, r.guard_touched = int(a.result_buffer), int(a.totals_nonzero), int(a.guard_touched)
    return r


def run_scan(hip, x, *, d_n=None, n_hint=None, in_place=False, want_total=True, device=0):
    """(status, out [n_max], total) of one cox_selftest_scan call."""
    x = np.ascontiguousarray(x, U32)
    n_max = len(x)
    n = n_max if d_n is None else min(int(d_n), n_max)
    out = np.zeros(n_max, U32)
    total = C.c_uint32(0)
    st = hip.fn("selftest_scan")(C.c_int(device), _ptr(x), C.c_uint32(n_max), C.c_int(d_n is not None), C.c_uint32(0 if d_n is None else int(d_n)),
                                 C.c_uint32(n if n_hint is None else int(n_hint)), C.c_int(in_place), C.c_int(want_total), C.c_uint32(SENTINEL),
                                 _ptr(out), C.byref(total))
    return st, out, int(total.value)


def run_scan_small(hip, a, b, n_max, d_n, device=0):
    """(status, [small a, small b, small2 a, small2 b], totals[4]) of one cox_selftest_scan_small call."""
    a, b = np.ascontiguousarray(a, U32), np.ascontiguousarray(b, U32)
    assert len(a) == len(b)
    outs = [np.zeros(len(a), U32) for _ in range(4)]
    totals = np.zeros(4, U32)
    st = hip.fn("selftest_scan_small")(C.c_int(device), _ptr(a), _ptr(b), C.c_uint32(len(a)), C.c_uint32(n_max), C.c_uint32(d_n), C.c_uint32(SENTINEL),
                                       *[_ptr(o) for o in outs], _ptr(totals))
    return st, outs, [int(t) for t in totals]


def make_keys(pattern, n, rb, nbits, base, seed):
    """n seeded u32 keys: a field of the sort's bits at bit `base`, random bits below `base` that the sort must ignore stably.
    Fields stay below 2^nbits except in `top_digit` (the whole top digit set, which may reach above nbits: the covered-bits
    rule) and `all_ones_mixed` (the engine's invalid marker, the whole key all ones)."""
    rng = np.random.default_rng([seed, n, rb, nbits, base, PATTERNS.index(pattern)])
    passes, width = pass_layout(rb, nbits)
    span = 1 << nbits  # fields are below this
    top_shift = (passes - 1) * width if passes else 0
    i = np.arange(n, dtype=np.uint64)
    if nbits == 0:
        field = np.zeros(n, np.uint64)
    elif pattern == "equal":
        field = np.full(n, int(rng.integers(0, span)), np.uint64)
    elif pattern in ("sorted", "reversed"):  # all distinct where 2^nbits >= n
        field = (i * np.uint64(span)) // np.uint64(max(n, 1))
        if pattern == "reversed":
            field = field[::-1].copy()
    elif pattern == "alternating":  # two digits, lane by lane
        a, b = (int(t) for t in rng.integers(0, span, 2))
        field = np.where(i & np.uint64(1), np.uint64(a), np.uint64(b))
    elif pattern == "top_digit":
        field = np.uint64(((1 << width) - 1) << top_shift) | rng.integers(0, 1 << top_shift, n, dtype=np.uint64)
    elif pattern == "high_pass_only":
        field = rng.integers(0, span >> top_shift, n, dtype=np.uint64) << np.uint64(top_shift)
    elif pattern == "heavy":  # a few heavy duplicates among random keys
        heavy = rng.integers(0, span, 3, dtype=np.uint64)
        pick = rng.integers(0, 8, n)
        field = np.where(pick < 3, heavy[np.minimum(pick, 2)], rng.integers(0, span, n, dtype=np.uint64))
    else:  # "random", "all_ones_mixed"
        field = rng.integers(0, span, n, dtype=np.uint64)
    low = rng.integers(0, 1 << base, n, dtype=np.uint64)
    keys = ((field << np.uint64(base)) | low) & np.uint64(ALL_ONES)
    if pattern == "all_ones_mixed":
        keys[rng.integers(0, 4, n) == 0] = ALL_ONES
    return keys.astype(U32)


def scan_inputs(n, seed):
    """name -> [n] u32 for the scan tests: zeros, ones, random small values, all 0xFFFFFFFF (wraps mod 2^32)."""
    rng = np.random.default_rng([seed, n])
    return {"zeros": np.zeros(n, U32), "ones": np.ones(n, U32), "small": rng.integers(0, 1000, n, dtype=np.uint64).astype(U32),
            "wrap": np.full(n, ALL_ONES, U32)}


def single_nonzero(n, pos, value=0x80000001):
    x = np.zeros(n, U32)
    x[pos] = value
    return x
