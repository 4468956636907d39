"""The core of the ctypes binding (coxgraph_amd/capi.py): the status table, the handle base class and its liveness guard, and the
argument helpers.  No GPU: the libraries are only asked for symbols, and the guard is tested against a stub engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from coxgraph_amd import capi
from coxgraph_amd.capi import CoxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "coxgraph_hip.h")).read(), flags=re.S)
IDENT = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)


def test_status_table_is_the_header_enum():
    body = re.search(r"typedef enum cox_status \{(.*?)\} cox_status;", HEADER, flags=re.S).group(1)
    enum = {int(v): k for k, v in re.findall(r"(COX_\w+)\s*=\s*(-?\d+)", body)}
    assert len(enum) >= 10
    assert capi.STATUS == enum
    assert str(CoxError(-9, "comm_init_rank")) == "comm_init_rank: COX_ERR_COMM"


# ---- handle classes -------------------------------------------------------------------------------------------------------------
HANDLE_CLASSES = sorted((c for c in vars(capi).values() if isinstance(c, type) and hasattr(c, "close") and c is not capi._Handle),
                        key=lambda c: c.__name__)


def test_every_class_that_closes_is_found():
    assert len(HANDLE_CLASSES) >= 16  # the 15 owners of a handle and the borrowed layer
    assert {capi.Layer, capi.Integrator, capi.Comm, capi.StereoMatcher, capi._BorrowedLayer} <= set(HANDLE_CLASSES)


@pytest.mark.parametrize("cls", HANDLE_CLASSES, ids=lambda c: c.__name__)
def test_handle_class(cls, hip, oracle):
    assert issubclass(cls, capi._Handle)
    assert hip.has(cls._destroy), cls._destroy
    # the checker mirrors what include/coxgraph_hip.h itself declares, without the communicator (tests/test_capi_symbols.py)
    if re.search(r"\bcox_%s\s*\(" % cls._destroy, HEADER) and cls is not capi.Comm:
        assert oracle.has(cls._destroy), cls._destroy
    # no class writes close() or __del__ out again, except to do more than destroy
    assert cls.__dict__.get("__del__") is None
    assert ("close" in cls.__dict__) == (cls in (capi.EsdfIntegrator, capi.StereoMatcher, capi._BorrowedLayer))
    obj = cls.__new__(cls)  # as after a constructor that raised before the create call
    obj.close()
    obj.close()


def test_the_checker_has_the_destroy_symbols_of_the_classes_parity_tests_build(oracle):
    for cls in (capi.Layer, capi.Integrator, capi.RegPoints, capi.Registration, capi.MeshConverter):
        assert re.search(r"\bcox_%s\s*\(" % cls._destroy, HEADER) and oracle.has(cls._destroy), cls._destroy


class StubEngine:
    """Records every way to reach a C function; whatever it hands out answers COX_OK."""

    def __init__(self):
        self.seen = []

    def fn(self, name, restype=C.c_int):
        self.seen.append(("fn", name))
        return lambda *args: 0

    def call(self, name, *args):
        self.seen.append(("call", name))

    def check(self, status, what):
        assert status == 0

    def has(self, name):
        return True


def test_close_destroys_once_and_is_idempotent():
    eng = StubEngine()
    layer = capi.Layer._adopt(eng, C.c_void_p(0x10), voxel_size=0.1)
    assert layer.eng is eng and layer.h.value == 0x10 and layer.voxel_size == 0.1
    layer.close()
    layer.close()
    assert eng.seen == [("fn", "layer_destroy")] and not layer.h
    m = capi.StereoMatcher._adopt(eng, C.c_void_p(0x20), h=48)  # its handle is h_; h is the image height
    assert m.h_.value == 0x20 and m.h == 48
    m.close()
    m.close()
    assert eng.seen[1:] == [("fn", "stereo_destroy")] and not m.h_ and m.h == 48
    borrowed = capi._BorrowedLayer(eng, 0.1, C.c_void_p(0x30))
    borrowed.close()
    assert not borrowed.h and len(eng.seen) == 2  # forgotten, not destroyed


# ---- the liveness guard ---------------------------------------------------------------------------------------------------------
PTS = np.zeros((1, 3), np.float32)
GUARDED = [(capi.Integrator, ("layer",)), (capi.Tracker, ("layer",)), (capi.ViewGain, ("layer",)), (capi.CollisionChecker, ("layer",)),
           (capi.DepthIntegrator, ("layer",)), (capi.EsdfIntegrator, ("tsdf",)), (capi.Registration, ("ref", "reading"))]
# a few ordinary methods of each: plain calls, a two-call download, a function that returns a value, the batch over many handles
CALLS = {
    capi.Integrator: lambda o: [o.sync, o.last_stats, lambda: o.integrate_points_dev(IDENT, 0x1000, 0, 1)],
    capi.Tracker: lambda o: [lambda: o.refine(IDENT, PTS), lambda: o.refine_dev(IDENT, 0x1000, n=1)],
    capi.ViewGain: lambda o: [o.view_bytes, lambda: o.visible(IDENT), lambda: o.evaluate(IDENT)],
    capi.CollisionChecker: lambda o: [o.stats, lambda: o.points(PTS)],
    capi.DepthIntegrator: lambda o: [o.sync, o.last_stats, o.pool_order],
    capi.EsdfIntegrator: lambda o: [o.update, o.invalidate],
    capi.Registration: lambda o: [o.get_samples, o.kernel_time, lambda: o.draw_samples(4, 1),
                                  lambda: capi.Registration.normal_eq_batch([o], np.zeros(4), np.zeros(4))],
}


def test_the_guarded_classes_are_those_that_name_an_owner():
    assert {c for c in HANDLE_CLASSES if c._borrows} == {c for c, _ in GUARDED}
    for cls, owners in GUARDED:
        assert cls._borrows == owners


@pytest.mark.parametrize("cls,owners", GUARDED, ids=lambda v: getattr(v, "__name__", None))
def test_a_call_after_the_owner_is_closed_never_reaches_c(cls, owners):
    for closed in owners + (None,):  # None: every owner alive, the control
        eng = StubEngine()
        attrs = {a: capi.Layer._adopt(eng, C.c_void_p(0 if a == closed else 0x2000), voxel_size=0.1, n=4) for a in owners}
        obj = cls._adopt(eng, C.c_void_p(0x1000), **attrs)
        for call in CALLS[cls](obj):
            eng.seen.clear()
            if closed is None:
                call()
                assert eng.seen, "the control reached nothing"
                continue
            with pytest.raises(CoxError) as e:
                call()
            assert e.value.status == -1 and "closed" in str(e.value)
            assert eng.seen == [], (closed, eng.seen)
        # close() is not guarded: the handle is destroyed as ever
        eng.seen.clear()
        obj.close()
        assert eng.seen == [("fn", cls._destroy)]


# ---- helpers --------------------------------------------------------------------------------------------------------------------
class _Tensor:
    def data_ptr(self):
        return 0x7F00_0000_1000


class _Stream:
    cuda_stream = 0x5555_0000_2000


def test_ptr_and_stream():
    assert capi._ptr(None) is None
    assert capi._ptr(0x7F12_3456_7000).value == 0x7F12_3456_7000  # a pointer above 2^32 survives
    assert capi._ptr(_Tensor()).value == 0x7F00_0000_1000
    assert capi._ptr(0).value in (0, None)
    assert capi._stream(None).value in (0, None)
    assert capi._stream(_Stream()).value == 0x5555_0000_2000
    assert capi._stream(0x5555_0000_3000).value == 0x5555_0000_3000
    assert capi._opt(None) is None
    a = np.zeros(3, np.float32)
    assert capi._opt(a).value == a.ctypes.data == capi._fp(a).value


def test_pose_and_intrinsics():
    from coxgraph_amd import synth
    T = capi._pose([1, 0, 0, 0, 1, 2, 3])
    assert T.dtype == np.float32 and T.shape == (7,) and T.flags.c_contiguous
    assert capi._pose(np.arange(14, dtype=np.float64)[::2]).flags.c_contiguous
    for bad in (np.zeros((1, 7)), np.zeros(6), np.zeros((7, 1))):
        with pytest.raises(AssertionError):
            capi._pose(bad)
    assert np.array_equal(capi._intrinsics(640, 480, None), np.asarray(synth.INTRINSICS[(640, 480)], np.float32))
    assert capi._intrinsics(3, 2, (1, 2, 3, 4)).tolist() == [1, 2, 3, 4]
    with pytest.raises(AssertionError):
        capi._intrinsics(3, 2, (1, 2, 3))


def test_config(hip):
    for make in (hip.default_config, lambda **k: capi.track_config(hip, **k), lambda **k: capi.viewgain_config(hip, **k),
                 lambda **k: capi.collide_config(hip, **k), lambda **k: capi.depthfuse_config(hip, **k), lambda **k: capi.stereo_config(hip, **k)):
        with pytest.raises(AttributeError):
            make(no_such_field=1)
    vg = capi.viewgain_config(hip, K=(1, 2, 3, 4), box_min=(0, 0, 0), box_max=np.array([1.5, 2.5, 3.5], np.float32), w=7)
    assert list(vg.K) == [1, 2, 3, 4] and list(vg.box_min) == [0, 0, 0] and list(vg.box_max) == [1.5, 2.5, 3.5] and vg.w == 7
    assert list(capi.collide_config(hip, clearing_centre=(1, 2, 3)).clearing_centre) == [1, 2, 3]
    assert capi.track_config(hip, max_iterations=3).max_iterations == 3
    base = capi.viewgain_config(hip)
    assert vg.ray_length == base.ray_length  # what is not overridden is the library's default


def test_esdf_config_default_distance_follows_max_distance(hip):
    base = capi._esdf_config(hip)
    only_max = capi._esdf_config(hip, max_distance_m=1.25)
    assert only_max.max_distance_m == 1.25 and only_max.default_distance_m == 1.25 and only_max.min_distance_m == base.min_distance_m
    both = capi._esdf_config(hip, max_distance_m=1.25, default_distance_m=3.0, min_weight=0.5)
    assert both.default_distance_m == 3.0 and both.min_weight == 0.5
    assert capi._esdf_config(hip, min_distance_m=0.5).default_distance_m == base.default_distance_m
