"""ctypes binding of the C ABI declared in include/coxgraph_hip.h.

The binding is generic over (shared library, symbol prefix): the product engine is
``coxgraph_amd/lib/libcoxgraph_hip.so`` with prefix ``cox_``; the test suite loads its CPU checker
(built from ``oracle/``, its own symbol prefix) through the same classes so parity tests read the
same on both sides.  Nothing in this package loads that checker.

The core comes first: ``Engine.call`` (look up, call, raise on a status), the argument helpers (``_ptr``, ``_stream``, ``_pose``,
``_intrinsics``, ``_config`` ...) and ``_Handle``, the base of every class that owns an opaque C handle.  The classes after it
only say which symbols they call with which arguments.
"""
import ctypes as C
import os
import numpy as np

COX_OK = 0
STATUS = {
    0: "COX_OK", -1: "COX_ERR_INVALID_ARG", -2: "COX_ERR_NO_DEVICE", -3: "COX_ERR_OUT_OF_MEMORY",
    -4: "COX_ERR_POOL_EXHAUSTED", -5: "COX_ERR_INDEX_RANGE", -6: "COX_ERR_UNSUPPORTED",
    -7: "COX_ERR_BUFFER_TOO_SMALL", -8: "COX_ERR_INTERNAL", -9: "COX_ERR_COMM",
}
METHODS = {"simple": 0, "merged": 1, "fast": 2, "projective": 3}
QUERY_MODES = {"nearest": 0, "interpolate": 1, "adaptive": 2}  # cox_query_mode (include/coxgraph_hip_map.h)
Q_VALUE, Q_TRILINEAR, Q_GRADIENT = 1, 2, 4
R_HIT, R_NORMAL, R_COLOR, R_BUDGET = 1, 2, 4, 8  # status bits of a rendered pixel (include/coxgraph_hip_render.h)
VOXELS_PER_BLOCK = 4096


class CoxError(RuntimeError):
    def __init__(self, status, what):
        super().__init__(f"{what}: {STATUS.get(status, status)}")
        self.status = status


class TsdfConfig(C.Structure):
    """cox_tsdf_config (voxblox TsdfIntegratorBase::Config)."""
    _fields_ = [
        ("default_truncation_distance", C.c_float), ("max_weight", C.c_float),
        ("voxel_carving_enabled", C.c_int32), ("min_ray_length_m", C.c_float),
        ("max_ray_length_m", C.c_float), ("use_const_weight", C.c_int32), ("allow_clear", C.c_int32),
        ("use_weight_dropoff", C.c_int32), ("use_sparsity_compensation_factor", C.c_int32),
        ("sparsity_compensation_factor", C.c_float), ("integrator_threads", C.c_int32),
        ("integration_order_mode", C.c_int32), ("enable_anti_grazing", C.c_int32),
        ("start_voxel_subsampling_factor", C.c_float), ("max_consecutive_ray_collisions", C.c_int32),
        ("clear_checks_every_n_frames", C.c_int32), ("max_integration_time_s", C.c_float),
        ("merged_bundle_order", C.c_int32), ("fast_exact_sets", C.c_int32),
        ("sensor_horizontal_resolution", C.c_int32), ("sensor_vertical_resolution", C.c_int32),
        ("sensor_vertical_field_of_view_degrees", C.c_float), ("projective_interpolation_scheme", C.c_int32),
        ("projective_adaptive_gap_m", C.c_float),
    ]


class FrameStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_points", "n_valid", "n_rays", "n_updates", "n_touched_voxels",
                                          "n_touched_blocks", "n_new_blocks", "max_bundle_points", "max_voxel_updates")]

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class EsdfConfig(C.Structure):
    """cox_esdf_config (voxblox EsdfIntegrator::Config)."""
    _fields_ = [("max_distance_m", C.c_float), ("min_distance_m", C.c_float), ("default_distance_m", C.c_float), ("min_weight", C.c_float)]


class RenderConfig(C.Structure):
    """cox_render_config."""
    _fields_ = [("min_depth", C.c_float), ("max_depth", C.c_float), ("step_scale", C.c_float), ("min_step_voxels", C.c_float),
                ("max_samples", C.c_uint32)]


class RenderStats(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("n_samples", C.c_uint64), ("n_block_skips", C.c_uint64), ("n_budget", C.c_uint64), ("kernel_ms", C.c_double)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RegConfig(C.Structure):
    _fields_ = [("no_correspondence_cost", C.c_double)]


# ---- the core: argument helpers, the engine, the handle base ---------------------------------------
def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def _opt(a):
    """_fp of an optional host array."""
    return None if a is None else _fp(a)


def _ptr(t):
    """A device buffer as c_void_p: a torch tensor (anything with data_ptr()), a raw address (int), or None."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def _stream(s):
    """A torch stream, a raw hipStream_t or None (the null stream) as c_void_p."""
    return C.c_void_p(getattr(s, "cuda_stream", s) or 0)


def _pose(T):
    """A pose qw qx qy qz tx ty tz as contiguous float32 (7,)."""
    T = np.ascontiguousarray(T, np.float32)
    assert T.shape == (7,)
    return T


def _intrinsics(w, h, K):
    """K = (fx, fy, cx, cy) as float32 (4,); None: synth.INTRINSICS[(w, h)]."""
    if K is None:
        from . import synth
        K = synth.INTRINSICS[(w, h)]
    K = np.ascontiguousarray(K, np.float32)
    assert K.shape == (4,)
    return K


def _config(eng, Struct, default_symbol, overrides):
    """Struct as default_symbol fills it, then the overrides: an unknown key raises AttributeError, a field that is an array
    takes a sequence."""
    c = Struct()
    eng.fn(default_symbol, None)(C.byref(c))
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        if isinstance(getattr(c, k), C.Array):
            v = type(getattr(c, k))(*np.asarray(v).ravel().tolist())
        setattr(c, k, v)
    return c


def _esdf_config(eng, max_distance_m=None, min_distance_m=None, default_distance_m=None, min_weight=None):
    """cox_esdf_config_default with the fields given; default_distance_m follows max_distance_m when only that is given."""
    if max_distance_m is not None and default_distance_m is None:
        default_distance_m = max_distance_m
    given = dict(max_distance_m=max_distance_m, min_distance_m=min_distance_m, default_distance_m=default_distance_m, min_weight=min_weight)
    return _config(eng, EsdfConfig, "esdf_config_default", {k: v for k, v in given.items() if v is not None})


class Engine:
    """One loaded implementation of the C ABI."""

    def __init__(self, lib_path, prefix):
        if not os.path.exists(lib_path):
            raise FileNotFoundError(lib_path)
        self.lib = C.CDLL(lib_path)
        self.prefix = prefix
        self.path = lib_path
        self._status_fns = {}  # name -> bound function that returns a cox_status (call())

    def fn(self, name, restype=C.c_int):
        f = getattr(self.lib, self.prefix + name)
        f.restype = restype
        return f

    def has(self, name):
        return hasattr(self.lib, self.prefix + name)

    def check(self, status, what):
        if status != COX_OK:
            raise CoxError(status, what)

    def call(self, name, *args):
        """Look the symbol up, call it, raise CoxError(status, name) unless it returns COX_OK.  The bound function is kept: this is
        the path of every per-frame call."""
        try:
            f = self._status_fns[name]
        except KeyError:
            f = self._status_fns[name] = self.lib[self.prefix + name]  # (an object of its own: fn() may set another restype on the shared one)
            f.restype = C.c_int
        status = f(*args)
        if status != COX_OK:
            raise CoxError(status, name)

    def default_config(self, **overrides):
        return _config(self, TsdfConfig, "tsdf_config_default", overrides)

    def device_count(self):
        return int(self.fn("device_count")()) if self.has("device_count") else 0


class _Handle:
    """What every owner of an opaque C handle shares: the engine, the handle, one idempotent close() and the guard in front of
    every call.  The class-level defaults make close() and __del__ no-ops on an object whose constructor never reached the create
    call."""
    _destroy = None  # the symbol that frees the handle
    _hattr = "h"     # the attribute that holds it
    _borrows = ()    # attributes (layers, point sets) whose C objects the handle keeps raw pointers into
    eng = None
    h = None

    @classmethod
    def _adopt(cls, eng, handle, **attrs):
        """An object around an existing handle, without running __init__."""
        self = cls.__new__(cls)
        self.eng = eng
        setattr(self, cls._hattr, handle)
        for k, v in attrs.items():
            setattr(self, k, v)
        return self

    def _guard(self, name):
        """The handle, unless an object it points into was closed first: the C side would read freed memory."""
        for a in self._borrows:
            if not getattr(self, a).h:
                raise CoxError(-1, name + " (the layer is closed)")
        return getattr(self, self._hattr)

    def _call(self, name, *args):
        self.eng.call(name, self._guard(name), *args)

    def _download(self, name, shapes, place=lambda arrays, cap: (*arrays, cap), query=None, also_ok=()):
        """The two-call download: the first call, with no arrays and a capacity of 0, asks for the count n; the second fills one
        zeroed array [n, *shape] per (shape, dtype) of `shapes`.  `place` puts the arrays and the capacity where the symbol takes them
        between the handle and the count; `query` labels an error of the first call, `also_ok` are statuses it may return."""
        h, f, n = self._guard(name), self.eng.fn(name), C.c_uint64()
        status = f(h, *place([None] * len(shapes), C.c_uint64(0)), C.byref(n))
        if status not in also_ok:
            self.eng.check(status, query or name)
        out = tuple(np.zeros((int(n.value), *shape), dtype) for shape, dtype in shapes)
        if n.value:
            self.eng.check(f(h, *place([_fp(a) for a in out], C.c_uint64(n.value)), C.byref(n)), name)
        return out

    def close(self):
        h = getattr(self, self._hattr)
        if h:
            self.eng.fn(self._destroy, None)(h)
            setattr(self, self._hattr, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Layer(_Handle):
    """voxblox::Layer<TsdfVoxel> (cox_layer_t)."""
    _destroy = "layer_destroy"

    def __init__(self, eng, voxel_size, voxels_per_side=16, device=0, capacity_blocks=0):
        self.eng = eng
        self.voxel_size = float(voxel_size)
        self.h = C.c_void_p()
        eng.call("layer_create", C.c_float(voxel_size), C.c_int(voxels_per_side), C.c_int(device), C.c_uint64(capacity_blocks), C.byref(self.h))

    def clear(self):  # removeAllBlocks
        self._call("layer_clear")

    def stats(self):
        n, b = C.c_uint64(), C.c_uint64()
        self._call("layer_stats", C.byref(n), C.byref(b))
        return int(n.value), int(b.value)

    def download(self):
        """serializeLayerAsMsg: (block_idx int32[n,3], words uint32[n,4096,3]) sorted by (z,y,x)."""
        return self._download("layer_download", (((3,), np.int32), ((VOXELS_PER_BLOCK, 3), np.uint32)), query="layer_download(query)")

    def merge_from(self, other, T_B_A=None):
        """mergeLayerAintoLayerB(other, [T_B_A,] self)."""
        self.eng.call("layer_merge", other.h, None if T_B_A is None else _fp(_pose(T_B_A)), self.h)

    def registration_points(self, min_voxel_weight=1.0, max_voxel_distance=0.3):
        """finishSubmap()'s relevant voxels: float32 [n,5] = x, y, z, distance, weight."""
        return self._download("layer_registration_points", (((5,), np.float32),),
                              lambda a, cap: (C.c_float(min_voxel_weight), C.c_float(max_voxel_distance), *a, cap))[0]

    def surface_obb(self):
        """getSubmapFrameSurfaceObb -> (min[3], max[3], n_surface_voxels)."""
        mn, mx, n = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_uint64()
        self._call("layer_surface_obb", _fp(mn), _fp(mx), C.byref(n))
        return mn, mx, int(n.value)

    def esdf(self, max_distance_m=None, min_distance_m=None, default_distance_m=None, min_weight=None):
        """generateEsdf(): a new layer (TSDF wire layout: distance = ESDF distance, weight = observed, colour word = fixed)."""
        cfg = _esdf_config(self.eng, max_distance_m, min_distance_m, default_distance_m, min_weight)
        out = Layer._adopt(self.eng, C.c_void_p(), voxel_size=self.voxel_size)
        self._call("esdf_from_tsdf", C.byref(cfg), C.byref(out.h))
        return out

    def reserve(self, capacity_blocks):
        self._call("layer_reserve", C.c_uint64(capacity_blocks))

    def capacity(self):
        n = C.c_uint64()
        self._call("layer_capacity", C.byref(n))
        return int(n.value)

    def set_auto_grow(self, on):
        self._call("layer_set_auto_grow", C.c_int(int(on)))

    def clone_to_device(self, device, capacity_blocks=0):
        """Submap hand-over inside one process: block array + keys copied GPU to GPU, hash rebuilt on `device`."""
        out = Layer._adopt(self.eng, C.c_void_p(), voxel_size=self.voxel_size)
        self._call("layer_clone_to_device", C.c_int(device), C.c_uint64(capacity_blocks), C.byref(out.h))
        return out

    def n_blocks(self):
        return self.stats()[0]

    def export_dev(self, idx_ptr, vox_ptr, cap_blocks):
        """serializeLayerAsMsg into device buffers (pointers as ints); returns the block count."""
        n = C.c_uint64()
        self._call("layer_export_dev", C.c_void_p(idx_ptr), C.c_void_p(vox_ptr), C.c_uint64(cap_blocks), C.byref(n))
        return int(n.value)

    def upload_dev(self, idx_ptr, vox_ptr, n_blocks, action=0):
        """deserializeMsgToLayer from device buffers (pointers as ints)."""
        self._call("layer_upload_dev", C.c_void_p(idx_ptr), C.c_void_p(vox_ptr), C.c_uint64(n_blocks), C.c_int(action))

    def upload(self, idx, vox, action=0):
        idx = np.ascontiguousarray(idx, np.int32)
        vox = np.ascontiguousarray(vox, np.uint32)
        assert vox.shape == (idx.shape[0], VOXELS_PER_BLOCK, 3)
        self._call("layer_upload", _fp(idx), _fp(vox), C.c_uint64(idx.shape[0]), C.c_int(action))

    def compare(self, other, T=None, ignore="all", sample="nearest", **cfg):
        """This layer as the test layer against `other` as the reference: the records of LayerComparer(...).run(T, ignore, sample)."""
        cmp = LayerComparer(self.eng, self, other, **cfg)
        try:
            return cmp.run(T, ignore, sample)
        finally:
            cmp.close()

    # ---- map queries (include/coxgraph_hip_map.h) ----
    def query(self, xyz, mode="interpolate", gradient=False):
        """voxblox Interpolator / EsdfMap batch queries at float32 points [n,3] in the layer's frame (cox_layer_query):
        dict(distance[n], weight[n], [gradient[n,3],] status[n] uint8 of Q_VALUE | Q_TRILINEAR | Q_GRADIENT); NaN where the
        matching status bit is clear."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        out = dict(distance=np.empty(n, np.float32), weight=np.empty(n, np.float32), status=np.empty(n, np.uint8))
        if gradient:
            out["gradient"] = np.empty((n, 3), np.float32)
        self._call("layer_query", _fp(xyz), C.c_uint64(n), C.c_int(QUERY_MODES[mode]), C.c_int(int(gradient)),
                   _fp(out["distance"]), _fp(out["weight"]), _opt(out.get("gradient")), _fp(out["status"]))
        return out

    def query_dev(self, xyz, n=None, mode="interpolate", gradient=False, distance=None, weight=None, grad=None, status=None, stream=None):
        """cox_layer_query_dev: torch tensors on the layer's GPU or raw device pointers (ints; then n is required), enqueued on
        `stream` (a torch stream, a raw hipStream_t or None = the null stream), not waited for.  Outputs left as they were
        where a status bit is clear."""
        if n is None:
            n = xyz.numel() // 3
        self._call("layer_query_dev", _ptr(xyz), C.c_uint64(n), C.c_int(QUERY_MODES[mode]), C.c_int(int(gradient)), _ptr(distance),
                   _ptr(weight), _ptr(grad), _ptr(status), _stream(stream))

    # ---- rendering (include/coxgraph_hip_render.h) ----
    def _render_args(self, T_G_C, w, h, K, cfg):
        return _pose(T_G_C), _intrinsics(w, h, K), _config(self.eng, RenderConfig, "render_config_default", cfg)

    def render(self, T_G_C, w, h, K=None, **cfg):
        """Depth, normal and colour images of the layer seen from T_G_C through a w x h pinhole camera K = (fx, fy, cx, cy)
        (cox_layer_render; K None: synth.INTRINSICS[(w, h)]; cfg: fields of cox_render_config): dict(depth[h,w] z-depth,
        normal[h,w,3], rgba[h,w,4], status[h,w] uint8 of R_HIT | R_NORMAL | R_COLOR | R_BUDGET, stats); NaN / 0 where the
        matching status bit is clear."""
        T, K, c = self._render_args(T_G_C, w, h, K, cfg)
        out = dict(depth=np.empty((h, w), np.float32), normal=np.empty((h, w, 3), np.float32), rgba=np.empty((h, w, 4), np.uint8),
                   status=np.empty((h, w), np.uint8))
        st = RenderStats()
        self._call("layer_render", _fp(T), C.c_int(w), C.c_int(h), _fp(K), C.byref(c), _fp(out["depth"]), _fp(out["normal"]),
                   _fp(out["rgba"]), _fp(out["status"]), C.byref(st))
        out["stats"] = st.asdict()
        return out

    def render_dev(self, T_G_C, w, h, K=None, depth=None, normal=None, rgba=None, status=None, stream=None, **cfg):
        """cox_layer_render_dev: outputs are torch tensors on the layer's GPU or raw device pointers (ints), any of them None;
        enqueued on `stream` (a torch stream, a raw hipStream_t or None = the null stream), not waited for.  Every pixel of
        every buffer given is written."""
        T, K, c = self._render_args(T_G_C, w, h, K, cfg)
        self._call("layer_render_dev", _fp(T), C.c_int(w), C.c_int(h), _fp(K), C.byref(c), _ptr(depth), _ptr(normal), _ptr(rgba),
                   _ptr(status), _stream(stream))

    # ---- view gain (include/coxgraph_hip_gain.h) ----
    def view_gain(self, poses, **cfg):
        """ViewGain(self, **cfg).evaluate(poses) with a throw-away evaluator: the gain records of candidate poses [n,7]."""
        vg = ViewGain(self.eng, self, **cfg)
        try:
            return vg.evaluate(poses)
        finally:
            vg.close()

    # ---- collision checks (include/coxgraph_hip_collide.h) ----
    def check_segments(self, a, b, **cfg):
        """CollisionChecker(self, **cfg).segments(a, b) with a throw-away checker: one record per straight segment a -> b."""
        cc = CollisionChecker(self.eng, self, **cfg)
        try:
            return cc.segments(a, b)
        finally:
            cc.close()

    # ---- incremental ESDF (include/coxgraph_hip_esdf.h) ----
    def esdf_integrator(self, **cfg):
        """EsdfIntegrator(self.eng, self, **cfg): an ESDF that follows this layer (keywords as esdf())."""
        return EsdfIntegrator(self.eng, self, **cfg)

    # ---- pinhole depth fusion (include/coxgraph_hip_depthfuse.h) ----
    def depth_integrator(self, **cfg):
        """DepthIntegrator(self.eng, self, **cfg): fuses depth and colour images of a pinhole camera into this layer."""
        return DepthIntegrator(self.eng, self, **cfg)

    def free_points(self, min_distance):
        """createFreePointcloudFromEsdfLayer: (xyz float32[n,3] voxel centres, intensity float32[n] distances), blocks in download
        order, voxels in linear index order."""
        return self._download("layer_free_points", (((3,), np.float32), ((), np.float32)), lambda a, cap: (C.c_float(min_distance), *a, cap),
                              query="layer_free_points(query)")


class Integrator(_Handle):
    """voxblox::TsdfIntegratorBase (cox_integrator_t)."""
    _destroy = "integrator_destroy"
    _borrows = ("layer",)

    def __init__(self, eng, layer, cfg, method):
        self.eng, self.layer = eng, layer
        self.h = C.c_void_p()
        m = METHODS[method] if isinstance(method, str) else int(method)
        eng.call("integrator_create", layer.h, C.byref(cfg), C.c_int(m), C.byref(self.h))

    def integrate_points(self, T_G_C, xyz, rgba=None, freespace=False):
        """integratePointCloud(T_G_C, points_C, colors, freespace_points) with host buffers."""
        T = _pose(T_G_C)
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] == 3
        n = xyz.shape[0]
        if rgba is not None:
            rgba = np.ascontiguousarray(rgba, np.uint8)
            assert rgba.shape == (n, 4)
        self._call("integrate_points", _fp(T), _fp(xyz), _opt(rgba), C.c_uint64(n), C.c_int(int(freespace)))

    def deintegrate_points(self, T_G_C, xyz):
        """integratePointCloud(..., deintegrate = true): projective integrator only."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        self._call("integrate_points_ex", _fp(_pose(T_G_C)), _fp(xyz), None, C.c_uint64(xyz.shape[0]), C.c_int(0), C.c_int(1))

    def integrate_points_dev(self, T_G_C, xyz_ptr, rgba_ptr, n, freespace=False):
        self._call("integrate_points_dev", _fp(_pose(T_G_C)), C.c_void_p(xyz_ptr), C.c_void_p(rgba_ptr or 0),
                   C.c_uint64(n), C.c_int(int(freespace)))

    def integrate_points_async(self, T_G_C, xyz_ptr, rgba_ptr, n, freespace=False):
        """Host buffers (addresses), frame not waited for; pinned buffers must stay untouched until wait_inputs() / sync()."""
        self._call("integrate_points_async", _fp(_pose(T_G_C)), C.c_void_p(xyz_ptr), C.c_void_p(rgba_ptr or 0),
                   C.c_uint64(n), C.c_int(int(freespace)))

    def wait_inputs(self):
        self._call("integrator_wait_inputs")

    def integrate_depth_dev(self, T_G_C, depth_ptr, rgba_ptr, w, h, K):
        K = np.ascontiguousarray(K, np.float32)
        self._call("integrate_depth_dev", _fp(_pose(T_G_C)), C.c_void_p(depth_ptr), C.c_void_p(rgba_ptr or 0),
                   C.c_int(w), C.c_int(h), _fp(K))

    def integrate_depth_async(self, T_G_C, depth_ptr, rgba_ptr, w, h, K):
        """Host depth / colour images (addresses), frame not waited for."""
        K = np.ascontiguousarray(K, np.float32)
        self._call("integrate_depth_async", _fp(_pose(T_G_C)), C.c_void_p(depth_ptr), C.c_void_p(rgba_ptr or 0),
                   C.c_int(w), C.c_int(h), _fp(K))

    def set_input_stream(self, stream_ptr, enable=True):
        """Order *_dev calls against the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream)."""
        self._call("integrator_set_input_stream", _stream(stream_ptr), C.c_int(int(enable)))

    def attach_history(self, obs):
        """cox_integrator_attach_history: every cloud fused from now on is also recorded in `obs` (an ObservationHistory) under
        its current frame id; None detaches."""
        self._call("integrator_attach_history", obs.h if obs is not None else None)
        self.history = obs  # (keeps the record alive while it is attached)

    def sync(self):
        self._call("integrator_sync")

    def last_stats(self):
        s = FrameStats()
        self._call("integrator_last_stats", C.byref(s))
        return s.asdict()

    def set_profiling(self, on=True):
        """0 / False = off, n >= 1 = HIP-event timing of the merge and apply kernels of every n-th frame."""
        self._call("integrator_set_profiling", C.c_int(int(on)))

    def stage_times(self, reset=False):
        """{'merge': (ms, launches), 'apply': (ms, launches)} measured with HIP events on the kernels' own streams."""
        ms, n = (C.c_double * 2)(), (C.c_uint64 * 2)()
        self._call("integrator_stage_times", ms, n, C.c_int(int(reset)))
        return {"merge": (float(ms[0]), int(n[0])), "apply": (float(ms[1]), int(n[1]))}

    KERNEL_CLASSES = ("merge", "apply", "bundle_hash", "point_sort", "touch_emit", "record_sort", "fast_start", "fast_visits", "fast_sweeps", "fast_round1")

    def class_times(self, reset=False):
        """{class: (ms, regions)} for every kernel class of a frame (cox_kernel_class), HIP events on the kernels' own streams."""
        k = len(self.KERNEL_CLASSES)
        ms, n = (C.c_double * k)(), (C.c_uint64 * k)()
        self._call("integrator_class_times", ms, n, C.c_int(int(reset)))
        return {name: (float(ms[i]), int(n[i])) for i, name in enumerate(self.KERNEL_CLASSES)}

    def fast_stats(self):
        """method 'fast': run totals of the observed-set relaxation (cox_integrator_fast_stats)."""
        out = (C.c_uint64 * 10)()
        self._call("integrator_fast_stats", out)
        return dict(sequential_frames=int(out[0]), round1_frames=int(out[1]), passes_round0=int(out[2]), passes_later_rounds=int(out[3]),
                    frames=int(out[4]), sequential_frames_list_outgrown=int(out[5]), sequential_frames_barrier_gave_up=int(out[6]), frames_with_three_rounds_or_more=int(out[7]), relax_work_ns=int(out[8]), relax_barrier_wait_ns=int(out[9]))

    def update_stats(self):
        """last frame: tiles whose classification was split over the chip, and their chunks (cox_integrator_update_stats)."""
        out = (C.c_uint64 * 2)()
        self._call("integrator_update_stats", out)
        return dict(split_tiles=int(out[0]), chunks=int(out[1]))

    def host_time(self, reset=False):
        """(ms, frames): host time spent inside the integrate calls (enqueueing; cox_integrator_host_time)."""
        ms, n = C.c_double(), C.c_uint64()
        self._call("integrator_host_time", C.byref(ms), C.byref(n), C.c_int(int(reset)))
        return float(ms.value), int(n.value)

    def kernel_time(self, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        self._call("integrator_kernel_time", C.byref(ms), C.byref(n), C.c_int(int(reset)))
        return float(ms.value), int(n.value)


class ObservationHistory(_Handle):
    """Which frames saw which part of a submap (cox_obs_t, include/coxgraph_hip_history.h): per 16^3 block 64 cells of 4x4x4
    voxels, per cell a 256-bit mask of frame ids."""
    _destroy = "obs_destroy"
    CELLS, WORDS = 64, 8

    def __init__(self, eng, layer, capacity_blocks=0):
        self.eng, self.voxel_size = eng, layer.voxel_size
        self.h = C.c_void_p()
        eng.call("obs_create", layer.h, C.c_uint64(capacity_blocks), C.byref(self.h))

    def clear(self):
        self._call("obs_clear")

    def set_auto_grow(self, on):
        self._call("obs_set_auto_grow", C.c_int(int(on)))

    def set_frame(self, frame_id):
        """The id (0..255) under which clouds are recorded until it is changed."""
        self._call("obs_set_frame", C.c_uint32(int(frame_id)))

    def record(self, T_G_C, xyz, min_ray, max_ray, freespace=False, allow_clear=True):
        """Record one host cloud (points in the sensor frame); returns when it is recorded."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._call("obs_record", _fp(_pose(T_G_C)), _fp(xyz), C.c_uint64(len(xyz)), C.c_int(int(freespace)), C.c_float(min_ray),
                   C.c_float(max_ray), C.c_int(int(allow_clear)))

    def record_dev(self, T_G_C, xyz, min_ray, max_ray, n=None, freespace=False, allow_clear=True, stream=None):
        """cox_obs_record_dev: xyz a torch tensor on the record's GPU or a raw device pointer (int; then n is required), ordered
        against `stream` (a torch stream, a raw hipStream_t or None = the null stream); not waited for."""
        if n is None:
            n = xyz.numel() // 3
        self._call("obs_record_dev", _fp(_pose(T_G_C)), _ptr(xyz), C.c_uint64(n), C.c_int(int(freespace)), C.c_float(min_ray),
                   C.c_float(max_ray), C.c_int(int(allow_clear)), _stream(stream))

    def sync(self):
        """Wait for the records; raises CoxError (COX_ERR_POOL_EXHAUSTED ...) when marks were lost since the last call."""
        self._call("obs_sync")

    def stats(self):
        """dict(blocks, marked_cells, bytes)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("obs_stats", C.byref(a), C.byref(b), C.byref(c))
        return dict(blocks=int(a.value), marked_cells=int(b.value), bytes=int(c.value))

    def counts(self):
        """Running totals: (points that marked, atomic ORs left after the lanes of a wave that share a cell merged)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._call("obs_counts", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def download(self):
        """(block_index int32[n,3] in (z, y, x) order, masks uint32[n,64,8])."""
        return self._download("obs_download", (((3,), np.int32), ((self.CELLS, self.WORDS), np.uint32)), query="obs_download(query)")


class RegPoints(_Handle):
    _destroy = "regpoints_destroy"

    def __init__(self, eng, pts, device=0):
        self.eng = eng
        pts = np.ascontiguousarray(pts, np.float32)
        assert pts.ndim == 2 and pts.shape[1] == 5
        self.n = pts.shape[0]
        self.h = C.c_void_p()
        eng.call("regpoints_create", C.c_int(device), _fp(pts), C.c_uint64(self.n), C.byref(self.h))

    @classmethod
    def from_layer(cls, eng, layer, min_voxel_weight=1.0, max_voxel_distance=0.3):
        """finishSubmap()'s relevant-voxel set, built and kept on the engine's side (no host round trip)."""
        h = C.c_void_p()
        eng.call("regpoints_from_layer", layer.h, C.c_float(min_voxel_weight), C.c_float(max_voxel_distance), C.byref(h))
        return cls._wrap(eng, h)

    @classmethod
    def _wrap(cls, eng, h):
        self = cls._adopt(eng, h)
        n = C.c_uint64()
        self._call("regpoints_size", C.byref(n))
        self.n = int(n.value)
        return self

    @classmethod
    def from_device(cls, eng, ptr, n, device=0):
        """A set whose n*5 floats already sit in HBM (pointer as int)."""
        h = C.c_void_p()
        eng.call("regpoints_create_dev", C.c_int(device), C.c_void_p(ptr), C.c_uint64(n), C.byref(h))
        return cls._wrap(eng, h)

    @classmethod
    def from_isosurface(cls, eng, layer, min_weight=1.0, vertex_proximity_threshold=None):
        """finishSubmap()'s isosurface vertices (the "explicit" set), built and kept on the engine's side."""
        thr = 0.5 * layer.voxel_size if vertex_proximity_threshold is None else vertex_proximity_threshold
        h, nm, nc = C.c_void_p(), C.c_uint64(), C.c_uint64()
        eng.call("regpoints_from_isosurface", layer.h, C.c_float(min_weight), C.c_float(thr), C.byref(h), C.byref(nm), C.byref(nc))
        self = cls._wrap(eng, h)
        self.n_mesh_vertices, self.n_connected_vertices = int(nm.value), int(nc.value)
        return self

    def clone_to_device(self, device):
        h = C.c_void_p()
        self._call("regpoints_clone_to_device", C.c_int(device), C.byref(h))
        return RegPoints._wrap(self.eng, h)

    def data_ptr(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._call("regpoints_data_dev", C.byref(p), C.byref(n))
        return int(p.value or 0), int(n.value)

    def download(self):
        out = np.zeros((self.n, 5), np.float32)
        n = C.c_uint64()
        self._call("regpoints_download", _fp(out), C.c_uint64(self.n), C.byref(n))
        return out


class Registration(_Handle):
    """voxgraph::RegistrationCostFunction for one (reference points, reading layer) pair."""
    _destroy = "reg_destroy"
    _borrows = ("ref", "reading")

    def __init__(self, eng, ref_points, reading_layer, no_correspondence_cost=0.0):
        self.eng, self.ref, self.reading = eng, ref_points, reading_layer
        cfg = RegConfig(no_correspondence_cost)
        self.h = C.c_void_p()
        eng.call("reg_create", ref_points.h, reading_layer.h, C.byref(cfg), C.byref(self.h))

    def _args(self, pose_ref, pose_read, sample_idx):
        pr = np.ascontiguousarray(pose_ref, np.float64)
        pd = np.ascontiguousarray(pose_read, np.float64)
        assert pr.shape == (4,) and pd.shape == (4,)
        if sample_idx is None:
            stored = getattr(self, "stored_n", None)  # (0 is a stored set too: an empty one)
            return pr, pd, None, (self.ref.n if stored is None else stored)
        si = np.ascontiguousarray(sample_idx, np.uint32)
        return pr, pd, si, si.shape[0]

    def evaluate(self, pose_ref, pose_read, sample_idx=None, jacobians=True):
        """CostFunction::Evaluate -> (residuals[n], J_ref[n,4], J_read[n,4])."""
        pr, pd, si, n = self._args(pose_ref, pose_read, sample_idx)
        r = np.zeros(n, np.float64)
        jf = np.zeros((n, 4), np.float64) if jacobians else None
        jr = np.zeros((n, 4), np.float64) if jacobians else None
        self._call("reg_evaluate", _fp(pr), _fp(pd), _opt(si), C.c_uint64(n), _fp(r), _opt(jf), _opt(jr))
        return r, jf, jr

    def normal_eq(self, pose_ref, pose_read, sample_idx=None):
        pr, pd, si, n = self._args(pose_ref, pose_read, sample_idx)
        H = np.zeros((8, 8), np.float64)
        b = np.zeros(8, np.float64)
        cost, nc = C.c_double(), C.c_uint64()
        self._call("reg_normal_eq", _fp(pr), _fp(pd), _opt(si), C.c_uint64(n), _fp(H), _fp(b), C.byref(cost), C.byref(nc))
        return H, b, float(cost.value), int(nc.value)

    def set_samples(self, sample_idx):
        """Keep the sample indices on the engine's side; later calls pass sample_idx=None and use them."""
        if sample_idx is None:
            self._call("reg_set_samples", None, C.c_uint64(0))
            self.stored_n = None
            return
        si = np.ascontiguousarray(sample_idx, np.uint32)
        self._call("reg_set_samples", _fp(si), C.c_uint64(si.shape[0]))
        self.stored_n = int(si.shape[0])

    def draw_samples(self, n_res, seed):
        """The weighted sampler's draws for one evaluation, made on the engine's side; they become the stored set."""
        self._call("reg_draw_samples", C.c_uint64(n_res), C.c_uint64(seed))
        self.stored_n = int(n_res)

    def get_samples(self):
        return self._download("reg_get_samples", (((), np.uint32),))[0]

    def normal_eq_begin(self, pose_ref, pose_read, sample_idx=None):
        pr, pd, si, n = self._args(pose_ref, pose_read, sample_idx)
        self._call("reg_normal_eq_begin", _fp(pr), _fp(pd), _opt(si), C.c_uint64(n))

    def normal_eq_finish(self):
        H = np.zeros((8, 8), np.float64)
        b = np.zeros(8, np.float64)
        cost, nc = C.c_double(), C.c_uint64()
        self._call("reg_normal_eq_finish", _fp(H), _fp(b), C.byref(cost), C.byref(nc))
        return H, b, float(cost.value), int(nc.value)

    def kernel_time(self, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        self._call("reg_kernel_time", C.byref(ms), C.byref(n), C.c_int(int(reset)))
        return float(ms.value), int(n.value)

    @staticmethod
    def normal_eq_batch(regs, poses_ref, poses_read):
        """cox_reg_normal_eq_batch: all the constraints of one pose-graph evaluation in ONE launch (every handle with its stored
        samples, or all its points).  -> [(H 8x8, b 8, cost, n_corr)] in the order of `regs`."""
        n = len(regs)
        eng = regs[0].eng
        handles = (C.c_void_p * n)(*[r._guard("reg_normal_eq_batch") for r in regs])
        pr = np.ascontiguousarray(poses_ref, np.float64).reshape(n, 4)
        pd = np.ascontiguousarray(poses_read, np.float64).reshape(n, 4)
        H = np.zeros((n, 8, 8), np.float64)
        b = np.zeros((n, 8), np.float64)
        cost = np.zeros(n, np.float64)
        nc = np.zeros(n, np.uint64)
        eng.call("reg_normal_eq_batch", handles, C.c_uint64(n), _fp(pr), _fp(pd), _fp(H), _fp(b), _fp(cost), _fp(nc))
        return [(H[c], b[c], float(cost[c]), int(nc[c])) for c in range(n)]


class Comm(_Handle):
    """cox_comm_t: RCCL behind the C ABI (one rank = one process = one GPU) -- the collectives the C++ host uses."""
    _destroy = "comm_destroy"
    ID_BYTES = 128

    @staticmethod
    def unique_id(eng):
        buf = (C.c_uint8 * Comm.ID_BYTES)()
        eng.call("comm_unique_id", buf)
        return bytes(buf)

    def __init__(self, eng, device, rank, world, unique_id):
        self.eng = eng
        self.h = C.c_void_p()
        buf = (C.c_uint8 * Comm.ID_BYTES).from_buffer_copy(unique_id)
        eng.call("comm_init_rank", C.c_int(device), C.c_int(rank), C.c_int(world), buf, C.byref(self.h))
        self.rank, self.world = rank, world

    def allreduce_f64(self, buf):
        """in-place sum over the ranks of a float64 numpy array (host in, host out)"""
        a = np.ascontiguousarray(buf, np.float64)
        self._call("comm_allreduce_f64", _fp(a), C.c_uint64(a.size))
        return a

    def allgather_dev(self, send_ptr, recv_ptr, bytes_per_rank, producer_stream=0):
        self._call("comm_allgather_dev_on", C.c_void_p(send_ptr), C.c_void_p(recv_ptr), C.c_uint64(bytes_per_rank), _stream(producer_stream))


class MeshMsgStruct(C.Structure):
    """cox_mesh_msg."""
    _fields_ = [
        ("block_edge_length", C.c_float), ("n_blocks", C.c_uint64), ("block_index", C.c_void_p), ("vertex_begin", C.c_void_p),
        ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("r", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p),
        ("block_has_history", C.c_void_p), ("history_begin", C.c_void_p), ("history", C.c_void_p),
        ("n_poses", C.c_uint64), ("stamp_sec", C.c_void_p), ("stamp_nsec", C.c_void_p), ("T_G_C", C.c_void_p),
    ]


class MeshMsg:
    """A voxblox_msgs/Mesh with history + trajectory, flattened into the arrays cox_mesh_msg points to.

    blocks: list of dict(index=(ix,iy,iz), x,y,z=uint16[nv], r,g,b=uint8[nv], history=None | list (one per triangle) of
    run-length lists [first0, last0, first1, last1, ...]); trajectory: list of (sec, nsec, T_G_C[7] float32).
    """

    def __init__(self, block_edge_length, blocks, trajectory):
        self.block_edge_length = float(block_edge_length)
        nb = len(blocks)
        self.block_index = np.array([b["index"] for b in blocks], np.int64).reshape(nb, 3)
        counts = [len(b["x"]) for b in blocks]
        self.vertex_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(b[k], dt) for b in blocks]) if nb else np.zeros(0, dt), dt)
        self.x, self.y, self.z = cat("x", np.uint16), cat("y", np.uint16), cat("z", np.uint16)
        self.r, self.g, self.b = cat("r", np.uint8), cat("g", np.uint8), cat("b", np.uint8)
        self.block_has_history = np.array([1 if b.get("history") else 0 for b in blocks], np.uint8)
        hb, hist = [0], []
        for b, cnt in zip(blocks, counts):
            runs = b.get("history") or [[] for _ in range(cnt // 3)]
            assert len(runs) == cnt // 3, "one ObsHistory per triangle"
            for r in runs:
                hist.extend(int(v) for v in r)
                hb.append(len(hist))
        self.history_begin = np.array(hb, np.uint64)
        self.history = np.array(hist, np.uint32)
        self.stamp_sec = np.array([p[0] for p in trajectory], np.uint32)
        self.stamp_nsec = np.array([p[1] for p in trajectory], np.uint32)
        self.T_G_C = np.ascontiguousarray(np.array([p[2] for p in trajectory], np.float32).reshape(len(trajectory), 7))
        self.n_blocks, self.n_poses = nb, len(trajectory)

    def struct(self):
        m = MeshMsgStruct()
        m.block_edge_length, m.n_blocks, m.n_poses = self.block_edge_length, self.n_blocks, self.n_poses
        for k in ("block_index", "vertex_begin", "x", "y", "z", "r", "g", "b", "block_has_history", "history_begin", "history", "stamp_sec",
                  "stamp_nsec", "T_G_C"):
            setattr(m, k, getattr(self, k).ctypes.data)
        return m


class MeshConverter(_Handle):
    """voxblox::MeshConverter (cox_meshconv_t): recover mode's mesh -> per-pose point clouds."""
    _destroy = "meshconv_destroy"

    def __init__(self, eng, interpolate_voxel_size=0.2, device=0):
        self.eng = eng
        self.h = C.c_void_p()
        eng.call("meshconv_create", C.c_int(device), C.c_float(interpolate_voxel_size), C.byref(self.h))

    def set_mesh(self, mesh):
        m = mesh.struct()
        self._call("meshconv_set_mesh", C.byref(m))

    def convert(self):
        """convertToPointCloud -> (converted?, recovered xyz float32[n,3], recovered rgb uint8[n,3])."""
        n, ok = C.c_uint64(), C.c_int()
        self._call("meshconv_convert", C.byref(n), C.byref(ok))
        return bool(ok.value), *self.recovered()

    def recovered(self):
        return self._download("meshconv_recovered", (((3,), np.float32), ((3,), np.uint8)), query="meshconv_recovered(query)")

    def pose_clouds(self):
        """The sequence getNextPointcloud yields: list of (T_G_C float32[7], points_C float32[n,3], colors uint8[n,4])."""
        out = []
        i = C.c_int32(0)
        T = np.zeros(7, np.float32)
        n, more = C.c_uint64(), C.c_int()
        while True:
            k = int(i.value)
            px, pc = C.c_void_p(), C.c_void_p()
            self._call("meshconv_next", C.byref(i), _fp(T), C.byref(px), C.byref(pc), C.byref(n), C.byref(more))
            if not more.value:
                break
            xyz = np.zeros((int(n.value), 3), np.float32)
            rgba = np.zeros((int(n.value), 4), np.uint8)
            if n.value:
                self._call("meshconv_download", C.c_int32(k), _fp(xyz), _fp(rgba), C.c_uint64(n.value), C.byref(n))
            out.append((T.copy(), xyz, rgba))
        return out

    def clear(self):
        self._call("meshconv_clear")

    def process_mesh(self, integrator, mesh):
        """TsdfRecover::processMesh up to the serialisation: -> (n_recovered_points, n_integratePointCloud_calls)."""
        m = mesh.struct()
        nr, ni = C.c_uint64(), C.c_uint64()
        self._call("recover_process_mesh", integrator._guard("recover_process_mesh"), C.byref(m), C.byref(nr), C.byref(ni))
        return int(nr.value), int(ni.value)


COLOR_MODES = {"color": 0, "normals": 1, "gray": 2, "lambert": 3, "lambert_color": 4}


class MeshLayer(_Handle):
    """voxblox::MeshLayer of a TSDF layer (cox_meshlayer_t, include/coxgraph_hip_mesh.h): per block with triangles its index and
    vertex range; per vertex position, face normal and colour; triangle t = vertices 3t, 3t+1, 3t+2."""
    _destroy = "meshlayer_destroy"

    def __init__(self, eng, h):
        self.eng, self.h = eng, h
        nb, nv, edge = C.c_uint64(), C.c_uint64(), C.c_float()
        self._call("meshlayer_size", C.byref(nb), C.byref(nv), C.byref(edge))
        self.n_blocks, self.n_vertices, self.block_edge_length = int(nb.value), int(nv.value), float(edge.value)
        self.n_triangles = self.n_vertices // 3

    @classmethod
    def from_layer(cls, eng, layer, min_weight=1e-4):
        """MeshIntegrator::generateMesh over the whole layer (corners valid when weight > min_weight)."""
        h = C.c_void_p()
        eng.call("meshlayer_from_layer", layer.h, C.c_float(min_weight), C.byref(h), None, None)
        return cls(eng, h)

    def stats(self):
        """(vertices whose colour voxel lay in no block, (count kernel ms, write kernel ms))."""
        n, ms = C.c_uint64(), np.zeros(2, np.float64)
        self._call("meshlayer_stats", C.byref(n), _fp(ms))
        return int(n.value), (float(ms[0]), float(ms[1]))

    def download(self):
        """dict(block_index int32[nb,3], vertex_begin uint64[nb+1], xyz float32[nv,3], normals float32[nv,3], rgb uint8[nv,3])."""
        nb, nv = self.n_blocks, self.n_vertices
        out = dict(block_index=np.zeros((nb, 3), np.int32), vertex_begin=np.zeros(nb + 1, np.uint64), xyz=np.zeros((nv, 3), np.float32),
                   normals=np.zeros((nv, 3), np.float32), rgb=np.zeros((nv, 3), np.uint8))
        self._call("meshlayer_download", *[_fp(out[k]) for k in ("block_index", "vertex_begin", "xyz", "normals", "rgb")],
                   C.c_uint64(nb), C.c_uint64(nv))
        return out

    def data_ptr(self):
        """(xyz, normals, rgb) device pointers as ints, and the vertex count."""
        p, q, r, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._call("meshlayer_data_dev", C.byref(p), C.byref(q), C.byref(r), C.byref(n))
        return int(p.value or 0), int(q.value or 0), int(r.value or 0), int(n.value)

    def transform(self, T):
        """In place: positions T p, normals R n (T = qw qx qy qz tx ty tz)."""
        self._call("meshlayer_transform", _fp(_pose(T)))

    def msg_arrays(self, color_mode="color"):
        """generateVoxbloxMeshMsg's per-vertex arrays: dict(x, y, z uint16[nv], r, g, b uint8[nv])."""
        nv = self.n_vertices
        out = {k: np.zeros(nv, np.uint16) for k in "xyz"}
        out.update({k: np.zeros(nv, np.uint8) for k in "rgb"})
        self._call("meshlayer_msg", C.c_int(COLOR_MODES[color_mode]), *[_fp(out[k]) for k in "xyzrgb"], C.c_uint64(nv))
        return out

    def history(self, obs, with_time=False):
        """cox_meshlayer_history against an ObservationHistory: dict(history_begin uint64[nt + 1], history uint32[...] of
        inclusive [first, last] frame-id runs, block_has_history uint8[nb]) in cox_mesh_msg's layout."""
        nt, nh, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        self._call("meshlayer_history_size", obs.h, C.byref(nt), C.byref(nh), C.byref(ms))
        nt, nh = int(nt.value), int(nh.value)
        out = dict(history_begin=np.zeros(nt + 1, np.uint64), history=np.zeros(nh, np.uint32), block_has_history=np.zeros(self.n_blocks, np.uint8))
        self._call("meshlayer_history", obs.h, _fp(out["history_begin"]), _fp(out["history"]), _fp(out["block_has_history"]),
                   C.c_uint64(nt), C.c_uint64(nh), C.c_uint64(self.n_blocks))
        if with_time:
            out["kernel_ms"] = float(ms.value)
        return out

    def to_msg(self, color_mode="color", history=None, trajectory=()):
        """A voxblox_msgs/Mesh in the dict form MeshMsg takes: MeshMsg(**mesh.to_msg(...)).  history: None, a callable
        (block index tuple, n_triangles) -> one run-length list per triangle (the caller's observation histories), or an
        ObservationHistory recorded while the layer was fused (a block none of whose triangles was seen goes without history)."""
        d = self.download()
        a = self.msg_arrays(color_mode)
        vb = d["vertex_begin"].astype(np.int64)
        if isinstance(history, ObservationHistory):
            h = self.history(history)
            hb, runs, has = h["history_begin"].astype(np.int64), h["history"], h["block_has_history"]
            order = {tuple(int(v) for v in d["block_index"][k]): k for k in range(self.n_blocks)}

            def history(idx, n, _hb=hb, _runs=runs, _has=has, _vb=vb, _order=order):
                k = _order[idx]
                if not _has[k]:
                    return None
                t0 = int(_vb[k]) // 3
                return [_runs[_hb[t]:_hb[t + 1]].tolist() for t in range(t0, t0 + n)]
        blocks = []
        for k in range(self.n_blocks):
            s, e = vb[k], vb[k + 1]
            idx = tuple(int(v) for v in d["block_index"][k])
            blk = dict(index=idx, **{c: a[c][s:e] for c in "xyzrgb"})
            if history is not None:
                blk["history"] = history(idx, int(e - s) // 3)
            blocks.append(blk)
        return dict(block_edge_length=self.block_edge_length, blocks=blocks, trajectory=list(trajectory))

    @staticmethod
    def connected(eng, parts, T_per_part=None, proximity_threshold=1e-4):
        """createConnectedMesh of several meshes, each moved by its T first: dict(xyz, normals, rgb, triangles uint32[nt,3])."""
        mesh = MeshLayer.connected_mesh(eng, parts, T_per_part, proximity_threshold)
        try:
            return mesh.download()
        finally:
            mesh.close()

    @staticmethod
    def connected_mesh(eng, parts, T_per_part=None, proximity_threshold=1e-4):
        """As connected(), but the welded mesh stays on the GPU: a ConnectedMesh to clean, smooth, cluster and download."""
        arr = (C.c_void_p * max(1, len(parts)))(*[p.h.value for p in parts])
        T = None if T_per_part is None else np.ascontiguousarray(np.asarray(T_per_part, np.float32).reshape(len(parts), 7))
        h = C.c_void_p()
        eng.call("meshlayer_connected", arr, _opt(T), C.c_uint64(len(parts)), C.c_float(proximity_threshold), C.byref(h), None, None)
        return ConnectedMesh(eng, h)


class ConnectedMesh(_Handle):
    """A connected mesh on the GPU (cox_meshconn_t) and its clean-up in place: DESIGN.md section 7h."""
    _destroy = "meshconn_destroy"

    def __init__(self, eng, h):
        self.eng, self.h = eng, h

    @classmethod
    def from_arrays(cls, eng, xyz, triangles, normals=None, rgb=None, device=0):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        tri = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        col = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        assert (nrm is None or len(nrm) == len(xyz)) and (col is None or len(col) == len(xyz))
        h = C.c_void_p()
        eng.call("meshconn_from_arrays", C.c_int(device), _fp(xyz), _opt(nrm), _opt(col), _fp(tri), C.c_uint64(len(xyz)), C.c_uint64(len(tri)),
                 C.byref(h))
        return cls(eng, h)

    @property
    def size(self):
        """(vertices, triangles)."""
        nv, nt = C.c_uint64(), C.c_uint64()
        self._call("meshconn_size", C.byref(nv), C.byref(nt))
        return int(nv.value), int(nt.value)

    def clean(self):
        """-> (degenerate triangles, duplicate triangles, unreferenced vertices) removed."""
        r = np.zeros(3, np.uint64)
        self._call("meshconn_clean", _fp(r))
        return tuple(int(v) for v in r)

    def smooth_taubin(self, iterations=100, lam=0.5, mu=-0.53):
        """-> HIP-event time of the 2 * iterations half-step launches, in ms."""
        ms = C.c_double()
        self._call("meshconn_smooth_taubin", C.c_int(iterations), C.c_float(lam), C.c_float(mu), C.byref(ms))
        return float(ms.value)

    def simplify_clustering(self, cell_size):
        """-> the new (vertices, triangles)."""
        nv, nt = C.c_uint64(), C.c_uint64()
        self._call("meshconn_simplify_clustering", C.c_float(cell_size), C.byref(nv), C.byref(nt))
        return int(nv.value), int(nt.value)

    def compute_normals(self):
        self._call("meshconn_compute_normals")

    def download(self):
        """dict(xyz, normals, rgb, triangles uint32[nt,3]), as MeshLayer.connected returns."""
        nv, nt = self.size
        out = dict(xyz=np.zeros((nv, 3), np.float32), normals=np.zeros((nv, 3), np.float32), rgb=np.zeros((nv, 3), np.uint8),
                   triangles=np.zeros((nt, 3), np.uint32))
        self._call("meshconn_download", *[_fp(out[k]) for k in ("xyz", "normals", "rgb", "triangles")], C.c_uint64(nv), C.c_uint64(nt))
        return out


# ---- scan-to-map registration (include/coxgraph_hip_track.h) ---------------------------------------
TRACK_STATUS = {0: "converged", 1: "max_iterations", 2: "lost", 3: "degenerate"}
TRACK_CONSIDERED, TRACK_USED = 1, 2  # status bits of Tracker.evaluate
TRACK_GRID_PASS = 65536              # COX_TRACK_GRID_PASS: candidates one pass of the kernel's grid covers


class TrackConfig(C.Structure):
    """cox_track_config."""
    _fields_ = [("dof", C.c_int32), ("max_iterations", C.c_uint32), ("stride", C.c_uint32), ("min_points", C.c_uint32),
                ("max_abs_distance", C.c_float), ("reserved", C.c_float), ("huber_delta", C.c_double), ("damping", C.c_double),
                ("translation_tolerance", C.c_double), ("rotation_tolerance", C.c_double), ("min_inlier_ratio", C.c_double)]


class TrackResult(C.Structure):
    """cox_track_result."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_uint32), ("first_n_used", C.c_uint64), ("first_n_considered", C.c_uint64),
                ("last_n_used", C.c_uint64), ("last_n_considered", C.c_uint64), ("first_cost", C.c_double), ("last_cost", C.c_double),
                ("last_step_translation", C.c_double), ("last_step_rotation", C.c_double), ("T_G_C", C.c_double * 7), ("kernel_ms", C.c_double)]

    def asdict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "T_G_C"}
        d["T"] = np.array(self.T_G_C[:], np.float64)
        d["status_name"] = TRACK_STATUS.get(self.status, str(self.status))
        return d


def track_config(eng, **cfg):
    return _config(eng, TrackConfig, "track_config_default", cfg)


class Tracker(_Handle):
    """Scan-to-map registration against a layer (cox_track_t): cfg are fields of cox_track_config."""
    _destroy = "track_destroy"
    _borrows = ("layer",)

    def __init__(self, eng, layer, **cfg):
        self.eng, self.layer = eng, layer  # (keeps the layer alive)
        self.cfg = track_config(eng, **cfg)
        self.h = C.c_void_p()
        eng.call("track_create", layer.h, C.byref(self.cfg), C.byref(self.h))

    def _result(self, res, T_refined):
        out = res.asdict()
        out["T_refined"] = T_refined
        return out

    def evaluate(self, T_G_C, xyz):
        """The per-point values of one iteration (cox_track_evaluate_dev) for host points [n,3]: dict(status uint8[n] of
        TRACK_CONSIDERED | TRACK_USED, pG[n,3], d[n], g[n,3]); NaN where the matching bit is clear."""
        import torch
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        dx = torch.from_numpy(xyz).cuda()
        vals = torch.empty((n, 7), dtype=torch.float32, device="cuda")
        st = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self._call("track_evaluate_dev", _fp(_pose(T_G_C)), _ptr(dx), C.c_uint64(n), _ptr(vals), _ptr(st))
        v = vals.cpu().numpy()
        return dict(status=st.cpu().numpy(), pG=v[:, 0:3].copy(), d=v[:, 3].copy(), g=v[:, 4:7].copy())

    def _normal_eq_out(self, name, *args):
        H, b, cost, counts = np.zeros(36, np.float64), np.zeros(6, np.float64), C.c_double(), (C.c_uint64 * 2)()
        self._call(name, *args, _fp(H), _fp(b), C.byref(cost), counts)
        dof = self.cfg.dof
        return dict(H=H.reshape(6, 6)[:dof, :dof].copy(), b=b[:dof].copy(), cost=cost.value, n_used=int(counts[0]), n_considered=int(counts[1]))

    def normal_eq(self, T_G_C, xyz, n=None):
        """One evaluation of the normal equations, no update (cox_track_normal_eq_dev): xyz a torch tensor on the layer's GPU, a raw
        device pointer (then n is required) or a host array.  dict(H[dof,dof], b[dof], cost, n_used, n_considered)."""
        xyz, n = self._dev_points(xyz, n)
        return self._normal_eq_out("track_normal_eq_dev", _fp(_pose(T_G_C)), _ptr(xyz), C.c_uint64(n))

    def normal_eq_depth_dev(self, T_G_C, depth, w, h, K=None):
        """normal_eq on a depth image on the device (cox_track_normal_eq_depth_dev)."""
        return self._normal_eq_out("track_normal_eq_depth_dev", _fp(_pose(T_G_C)), _ptr(depth), C.c_int(w), C.c_int(h), _fp(_intrinsics(w, h, K)))

    def _dev_points(self, xyz, n):
        if isinstance(xyz, np.ndarray):
            import torch
            xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)).cuda()
            torch.cuda.synchronize()
        if n is None:
            n = xyz.numel() // 3
        return xyz, n

    def refine(self, T_prior, xyz):
        """cox_track_refine with host points [n,3]: the fields of cox_track_result as a dict (T float64[7], status_name, ...)
        plus T_refined float32[7]."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        res, Tr = TrackResult(), np.zeros(7, np.float32)
        self._call("track_refine", _fp(_pose(T_prior)), _fp(xyz), C.c_uint64(len(xyz)), _fp(Tr), C.byref(res))
        return self._result(res, Tr)

    def refine_dev(self, T_prior, xyz, n=None):
        """cox_track_refine_dev: xyz a torch tensor on the layer's GPU or a raw device pointer (then n is required), complete
        when the call is made."""
        if n is None:
            n = xyz.numel() // 3
        res, Tr = TrackResult(), np.zeros(7, np.float32)
        self._call("track_refine_dev", _fp(_pose(T_prior)), _ptr(xyz), C.c_uint64(n), _fp(Tr), C.byref(res))
        return self._result(res, Tr)

    def refine_depth_dev(self, T_prior, depth, w, h, K=None):
        """cox_track_refine_depth_dev: depth a torch tensor [h,w] on the layer's GPU or a raw device pointer, in the layout of
        Integrator.integrate_depth_dev and Layer.render_dev; K None: synth.INTRINSICS[(w, h)]."""
        res, Tr = TrackResult(), np.zeros(7, np.float32)
        self._call("track_refine_depth_dev", _fp(_pose(T_prior)), _ptr(depth), C.c_int(w), C.c_int(h),
                   _fp(_intrinsics(w, h, K)), _fp(Tr), C.byref(res))
        return self._result(res, Tr)


# ---- view gain for exploration (include/coxgraph_hip_gain.h) ---------------------------------------
VG_FREE, VG_OCCUPIED, VG_UNKNOWN, VG_FRONTIER = 0, 1, 2, 3  # class of a visible voxel (ViewGain.visible)
VG_COUNTS = ("n_visible", "n_free", "n_occupied", "n_surface_counted", "n_unknown", "n_frontier")


class ViewGainConfig(C.Structure):
    """cox_viewgain_config."""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("K", C.c_float * 4), ("min_range", C.c_float), ("ray_length", C.c_float), ("ray_step", C.c_float),
                ("min_weight", C.c_float), ("surface_distance", C.c_float), ("frontier_voxel_weight", C.c_float), ("new_voxel_weight", C.c_float),
                ("min_impact_factor", C.c_float), ("ray_angle_x", C.c_float), ("ray_angle_y", C.c_float), ("accurate_frontiers", C.c_int32),
                ("surface_frontiers", C.c_int32), ("use_box", C.c_int32), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
                ("workspace_bytes", C.c_uint64)]


class ViewGainRecord(C.Structure):
    """cox_view_gain."""
    _fields_ = [("gain", C.c_double), ("surface_gain", C.c_double), ("surface_gain_q32", C.c_uint64)] + [(n, C.c_uint32) for n in VG_COUNTS]


VIEW_GAIN_DTYPE = np.dtype([("gain", np.float64), ("surface_gain", np.float64), ("surface_gain_q32", np.uint64)] + [(n, np.uint32) for n in VG_COUNTS])
assert VIEW_GAIN_DTYPE.itemsize == C.sizeof(ViewGainRecord) == 48


class ViewGainStats(C.Structure):
    _fields_ = [("n_samples", C.c_uint64), ("n_chunks", C.c_uint64), ("kernel_ms", C.c_double)]


def viewgain_config(eng, **cfg):
    """cox_viewgain_config_default with overrides; K, box_min and box_max take sequences."""
    return _config(eng, ViewGainConfig, "viewgain_config_default", cfg)


class ViewGain(_Handle):
    """Scores candidate views against a layer (cox_viewgain_t): cfg are fields of cox_viewgain_config."""
    _destroy = "viewgain_destroy"
    _borrows = ("layer",)

    def __init__(self, eng, layer, **cfg):
        self.eng, self.layer = eng, layer  # (keeps the layer alive)
        self.cfg = viewgain_config(eng, **cfg)
        self.h = C.c_void_p()
        eng.call("viewgain_create", layer.h, C.byref(self.cfg), C.byref(self.h))

    def view_bytes(self):
        """Workspace bytes one view takes (cox_viewgain_view_bytes)."""
        h = self._guard("viewgain_view_bytes")
        return int(self.eng.fn("viewgain_view_bytes", C.c_uint64)(h))

    def evaluate(self, poses):
        """cox_viewgain_evaluate for host poses [n,7] (qw qx qy qz tx ty tz): dict of numpy arrays over the views -- gain,
        surface_gain, surface_gain_q32 and the counts of cox_view_gain -- plus stats (n_samples, n_chunks, kernel_ms)."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        n = len(poses)
        rec = np.zeros(n, VIEW_GAIN_DTYPE)
        st = ViewGainStats()
        self._call("viewgain_evaluate", _fp(poses), C.c_uint64(n), _fp(rec), C.byref(st))
        out = {k: rec[k].copy() for k in VIEW_GAIN_DTYPE.names}
        out["stats"] = dict(n_samples=int(st.n_samples), n_chunks=int(st.n_chunks), kernel_ms=float(st.kernel_ms))
        return out

    def evaluate_dev(self, poses_dev, out_dev, stream=None, n=None):
        """cox_viewgain_evaluate_dev: poses_dev a float32 torch tensor [n,7] on the layer's GPU (or a raw device pointer; then n is
        required), out_dev a tensor of n * 48 bytes (view it with VIEW_GAIN_DTYPE once it is on the host) or a raw pointer; enqueued
        on `stream` (a torch stream, a raw hipStream_t or None = the null stream), not waited for."""
        if n is None:
            n = poses_dev.numel() // 7
        self._call("viewgain_evaluate_dev", _ptr(poses_dev), C.c_uint64(n), _ptr(out_dev), _stream(stream))

    def visible(self, pose):
        """The visible set of one view (cox_viewgain_visible): dict(voxel_xyz int32[n,3] global voxel indices, cls uint8[n] of
        VG_FREE | VG_OCCUPIED | VG_UNKNOWN | VG_FRONTIER, value float32[n]) in ascending (z, y, x) order."""
        pose = _pose(pose)
        out = self._download("viewgain_visible", (((3,), np.int32), ((), np.uint8), ((), np.float32)), lambda a, cap: (_fp(pose), cap, *a),
                             query="viewgain_visible(query)")
        return dict(zip(("voxel_xyz", "cls", "value"), out))


# ---- collision checks for a planner (include/coxgraph_hip_collide.h) --------------------------------
C_TRAVERSABLE, C_OBSERVED, C_DISTANCE, C_CLEARED, C_INVALID = 1, 2, 4, 8, 16  # state of a sample (CollisionChecker.points)
SEG_FEASIBLE, SEG_GOAL, SEG_CLAMPED, SEG_TOO_LONG, SEG_INVALID = 1, 2, 4, 8, 16  # flags of a record
TREE_KEEP, TREE_INVALID = 1, 2  # keep[] of a tree


class CollideConfig(C.Structure):
    """cox_collide_config."""
    _fields_ = [("collision_radius", C.c_float), ("collision_optimistic", C.c_int32), ("clearing_radius", C.c_float), ("clearing_centre", C.c_float * 3),
                ("sample_spacing", C.c_float), ("max_samples", C.c_uint32), ("max_extension_range", C.c_float), ("crop", C.c_int32),
                ("crop_margin", C.c_float), ("crop_min_length", C.c_float)]


class CollideStats(C.Structure):
    _fields_ = [("n_samples_evaluated", C.c_uint64), ("n_samples_skipped", C.c_uint64), ("n_launches", C.c_uint64), ("kernel_ms", C.c_double)]


COLLIDE_RECORD_DTYPE = np.dtype([("n_samples", np.uint32), ("first_blocked", np.uint32), ("flags", np.uint32), ("free_length", np.float32),
                                 ("goal", np.float32, 3), ("pad", np.uint32)])
assert COLLIDE_RECORD_DTYPE.itemsize == 32


def collide_config(eng, **cfg):
    """cox_collide_config_default with overrides; clearing_centre takes a sequence."""
    return _config(eng, CollideConfig, "collide_config_default", cfg)


class CollisionChecker(_Handle):
    """Checks planner paths against a layer (cox_collide_t): cfg are fields of cox_collide_config, group_size 32 or 64."""
    _destroy = "collide_destroy"
    _borrows = ("layer",)

    def __init__(self, eng, layer, group_size=None, **cfg):
        self.eng, self.layer = eng, layer  # (keeps the layer alive)
        self.cfg = collide_config(eng, **cfg)
        self.h = C.c_void_p()
        eng.call("collide_create", layer.h, C.byref(self.cfg), C.byref(self.h))
        if group_size is not None:
            self.set_group_size(group_size)

    def set_clearing_centre(self, centre):
        c = np.ascontiguousarray(centre, np.float32)
        assert c.shape == (3,)
        self._call("collide_set_clearing_centre", _fp(c))

    def set_group_size(self, lanes):
        self._call("collide_set_group_size", C.c_int(lanes))

    def set_profiling(self, on=True):
        self._call("collide_set_profiling", C.c_int(int(on)))

    def stats(self, reset=False):
        st = CollideStats()
        self._call("collide_stats", C.byref(st), C.c_int(int(reset)))
        return dict(n_samples_evaluated=int(st.n_samples_evaluated), n_samples_skipped=int(st.n_samples_skipped), n_launches=int(st.n_launches),
                    kernel_ms=float(st.kernel_ms))

    @staticmethod
    def _records(rec):
        return {k: rec[k].copy() for k in COLLIDE_RECORD_DTYPE.names if k != "pad"}

    def points(self, xyz):
        """cox_collide_points at float32 points [n,3]: dict(state[n] uint8 of C_*, distance[n], NaN without C_DISTANCE)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        out = dict(state=np.zeros(n, np.uint8), distance=np.full(n, np.nan, np.float32))
        self._call("collide_points", _fp(xyz), C.c_uint64(n), _fp(out["state"]), _fp(out["distance"]))
        return out

    def points_dev(self, xyz, state=None, distance=None, n=None, stream=None):
        """cox_collide_points_dev: torch tensors on the layer's GPU or raw device pointers (ints; then n is required), enqueued on
        `stream` (a torch stream, a raw hipStream_t or None = the null stream), not waited for."""
        if n is None:
            n = xyz.numel() // 3
        self._call("collide_points_dev", _ptr(xyz), C.c_uint64(n), _ptr(state), _ptr(distance), _stream(stream))

    def segments(self, a, b):
        """cox_collide_segments for straight segments a[n,3] -> b[n,3]: dict of numpy arrays over the segments -- n_samples,
        first_blocked, flags (SEG_*), free_length, goal[n,3]."""
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
        assert a.shape == b.shape
        rec = np.zeros(len(a), COLLIDE_RECORD_DTYPE)
        rec["free_length"] = rec["goal"] = np.nan
        self._call("collide_segments", _fp(a), _fp(b), C.c_uint64(len(a)), _fp(rec))
        return self._records(rec)

    def segments_dev(self, a, b, out, n=None, stream=None):
        """cox_collide_segments_dev: out a tensor of n * 32 bytes (view it with COLLIDE_RECORD_DTYPE on the host) or a raw pointer."""
        if n is None:
            n = a.numel() // 3
        self._call("collide_segments_dev", _ptr(a), _ptr(b), C.c_uint64(n), _ptr(out), _stream(stream))

    @staticmethod
    def _csr(offsets, xyz):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        assert offsets.ndim == 1 and len(offsets) >= 1
        return offsets, xyz

    def trajectories(self, offsets, xyz):
        """cox_collide_trajectories: trajectory t is xyz[offsets[t]:offsets[t + 1]]; dict as segments() (free_length and goal NaN)."""
        offsets, xyz = self._csr(offsets, xyz)
        rec = np.zeros(len(offsets) - 1, COLLIDE_RECORD_DTYPE)
        rec["free_length"] = rec["goal"] = np.nan
        self._call("collide_trajectories", _fp(offsets), C.c_uint64(len(offsets) - 1), _fp(xyz), C.c_uint64(len(xyz)), _fp(rec))
        return self._records(rec)

    def trajectories_dev(self, offsets, n_traj, xyz, n_points, out, stream=None):
        self._call("collide_trajectories_dev", _ptr(offsets), C.c_uint64(n_traj), _ptr(xyz), C.c_uint64(n_points), _ptr(out), _stream(stream))

    def prune_dev(self, parent, feasible, keep, n=None, feasible_stride=1, stream=None):
        """cox_collide_prune_dev: parent int32[n], feasible bytes (bit 0, feasible_stride bytes apart), keep uint8[n] of TREE_*."""
        if n is None:
            n = parent.numel()
        self._call("collide_prune_dev", _ptr(parent), _ptr(feasible), C.c_uint64(feasible_stride), C.c_uint64(n), _ptr(keep), _stream(stream))

    def prune(self, parent, feasible):
        """keep uint8[n] of a tree given on the host (staged through torch; the rule runs in cox_collide_prune_dev)."""
        import torch
        parent = np.ascontiguousarray(parent, np.int32)
        feasible = np.ascontiguousarray(feasible, np.uint8)
        assert parent.shape == feasible.shape and parent.ndim == 1
        if len(parent) == 0:
            return np.zeros(0, np.uint8)
        p, f = torch.from_numpy(parent).cuda(), torch.from_numpy(feasible).cuda()
        keep = torch.zeros(len(parent), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream()
        self.prune_dev(p, f, keep, stream=s)
        s.synchronize()
        return keep.cpu().numpy()

    def tree(self, offsets, parent, xyz):
        """cox_collide_tree: node i owns trajectory i; dict as trajectories() plus keep uint8[n] of TREE_*."""
        offsets, xyz = self._csr(offsets, xyz)
        parent = np.ascontiguousarray(parent, np.int32)
        n = len(offsets) - 1
        assert parent.shape == (n,)
        rec = np.zeros(n, COLLIDE_RECORD_DTYPE)
        rec["free_length"] = rec["goal"] = np.nan
        keep = np.zeros(n, np.uint8)
        self._call("collide_tree", _fp(offsets), _fp(parent), C.c_uint64(n), _fp(xyz), C.c_uint64(len(xyz)), _fp(rec), _fp(keep))
        out = self._records(rec)
        out["keep"] = keep
        return out

    def tree_dev(self, offsets, parent, n_nodes, xyz, n_points, out, keep, stream=None):
        self._call("collide_tree_dev", _ptr(offsets), _ptr(parent), C.c_uint64(n_nodes), _ptr(xyz), C.c_uint64(n_points), _ptr(out), _ptr(keep),
                   _stream(stream))


class EsdfUpdateStats(C.Structure):
    """cox_esdf_update_stats."""
    _fields_ = [(n, C.c_uint64) for n in ("n_blocks", "n_new_blocks", "n_dirty_blocks", "n_swept_blocks", "n_raise_sweeps", "n_lower_sweeps",
                                          "n_reset_voxels", "n_changed_voxels")] + [("rebuilt", C.c_uint32), ("pad", C.c_uint32), ("ms", C.c_double)]

    def asdict(self):
        return {n: (float(self.ms) if n == "ms" else int(getattr(self, n))) for n, _ in self._fields_ if n != "pad"}


class _BorrowedLayer(Layer):
    """A layer owned by another handle: closing it only forgets the pointer (every call on it then fails with INVALID_ARG)."""

    def __init__(self, eng, voxel_size, h):
        self.eng, self.voxel_size, self.h = eng, voxel_size, h

    def close(self):
        self.h = C.c_void_p()  # forgotten first: the owner destroys it, so nothing is left for the base to destroy
        super().close()


class EsdfIntegrator(_Handle):
    """voxblox EsdfIntegrator::updateFromTsdfLayer (cox_esdf_t): an ESDF bound to a TSDF layer; update() brings it to exactly what
    layer.esdf(**cfg) would return now.  Keywords as Layer.esdf (default_distance_m follows max_distance_m when only that is given)."""
    _destroy = "esdf_destroy"
    _borrows = ("tsdf",)
    layer = None

    def __init__(self, eng, layer, max_distance_m=None, min_distance_m=None, default_distance_m=None, min_weight=None):
        self.eng, self.tsdf = eng, layer  # (keeps the TSDF alive)
        self.cfg = _esdf_config(eng, max_distance_m, min_distance_m, default_distance_m, min_weight)
        self.h = C.c_void_p()
        eng.call("esdf_create", layer.h, C.byref(self.cfg), C.byref(self.h))
        lh = C.c_void_p()
        self._call("esdf_layer", C.byref(lh))
        self.layer = _BorrowedLayer(eng, layer.voxel_size, lh)

    def close(self):
        if self.layer is not None:
            self.layer.close()  # the borrowed layer dies with the handle: later use is refused
        super().close()

    def update(self):
        st = EsdfUpdateStats()
        self._call("esdf_update", C.byref(st))
        return st.asdict()

    def invalidate(self):
        self._call("esdf_invalidate")


class DepthFuseConfig(C.Structure):
    """cox_depthfuse_config."""
    _fields_ = [("truncation_distance", C.c_float), ("max_weight", C.c_float), ("min_depth_m", C.c_float), ("max_depth_m", C.c_float),
                ("voxel_carving_enabled", C.c_int32), ("use_const_weight", C.c_int32), ("use_weight_dropoff", C.c_int32),
                ("interpolation_scheme", C.c_int32), ("adaptive_gap_m", C.c_float), ("reserved", C.c_uint32)]


class DepthFuseStats(C.Structure):
    """cox_depthfuse_stats."""
    _fields_ = [(n, C.c_uint64) for n in ("n_valid_pixels", "n_candidate_blocks", "n_touched_blocks", "n_new_blocks", "n_updated_voxels",
                                          "n_coloured_voxels")] + [("kernel_ms", C.c_double)]

    def asdict(self):
        return {n: (float(self.kernel_ms) if n == "kernel_ms" else int(getattr(self, n))) for n, _ in self._fields_}


def depthfuse_config(eng, **cfg):
    """cox_depthfuse_config_default with fields overridden"""
    return _config(eng, DepthFuseConfig, "depthfuse_config_default", cfg)


class DepthIntegrator(_Handle):
    """The voxel-projective integrator of a pinhole depth camera (cox_depthfuse_t): cfg are fields of
    cox_depthfuse_config.  Images are [h, w] float32 z-depths (NaN, 0, negative: nothing there) and [h, w, 4] uint8 r, g, b, a;
    K = (fx, fy, cx, cy), None: synth.INTRINSICS[(w, h)]."""
    _destroy = "depthfuse_destroy"
    _borrows = ("layer",)

    def __init__(self, eng, layer, **cfg):
        self.eng, self.layer = eng, layer  # (keeps the layer alive)
        self.cfg = depthfuse_config(eng, **cfg)
        self.h = C.c_void_p()
        eng.call("depthfuse_create", layer.h, C.byref(self.cfg), C.byref(self.h))

    def integrate(self, T_G_C, depth, rgba=None, K=None):
        """cox_depthfuse_integrate: one frame from host images; the update is enqueued, not waited for (sync())."""
        depth =np.ascontiguousarray(depth, np.float32)
        assert depth.ndim == 2
        h, w = depth.shape
        T, K = _pose(T_G_C), _intrinsics(w, h, K)
        if rgba is not None:
            rgba = np.ascontiguousarray(rgba, np.uint8)
            assert rgba.shape == (h, w, 4)
        self._call("depthfuse_integrate", _fp(T), _fp(depth), _opt(rgba), C.c_int(w), C.c_int(h), _fp(K))

    def integrate_dev(self, T_G_C, depth, rgba, w, h, K=None, stream=None):
        """cox_depthfuse_integrate_dev: images are torch tensors on the layer's GPU or raw device pointers (ints), rgba may be
        None; ordered behind `stream` (a torch stream, a raw hipStream_t or None = the null stream), which then waits until the
        frame has read them."""
        self._call("depthfuse_integrate_dev", _fp(_pose(T_G_C)), _ptr(depth), _ptr(rgba), C.c_int(w), C.c_int(h), _fp(_intrinsics(w, h, K)),
                   _stream(stream))

    def sync(self):
        self._call("depthfuse_sync")

    def last_stats(self):
        st = DepthFuseStats()
        self._call("depthfuse_last_stats", C.byref(st))
        return st.asdict()

    def pool_order(self):
        """the layer's block indices int32[n, 3] in pool order"""
        return self._download("depthfuse_pool_order", (((3,), np.int32),), query="depthfuse_pool_order(query)",
                              also_ok=(-7,))[0]  # (the query may answer COX_ERR_BUFFER_TOO_SMALL)


# ---- dense stereo (include/coxgraph_hip_stereo.h) -------------------------------------------------
STEREO_BUFFERS = {"rect_left": 0, "rect_right": 1, "cost_sum": 2, "disparity": 3}  # cox_stereo_buffer
STEREO_INVALID = 0xFFFF


class StereoConfig(C.Structure):
    """cox_stereo_config."""
    _fields_ = [("n_disparities", C.c_int32), ("n_paths", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("uniqueness_percent", C.c_int32),
                ("lr_max_diff", C.c_int32), ("min_depth_m", C.c_float), ("max_depth_m", C.c_float), ("reserved", C.c_uint32)]


class StereoStats(C.Structure):
    """cox_stereo_stats."""
    _fields_ = [(n, C.c_uint64) for n in ("n_valid_pixels", "n_rejected_uniqueness", "n_rejected_lr", "n_rejected_depth")] + \
               [(n, C.c_double) for n in ("remap_ms", "census_ms", "paths_ms", "winner_ms", "depth_ms", "frame_ms")]

    def asdict(self):
        return {n: (float(getattr(self, n)) if t is C.c_double else int(getattr(self, n))) for n, t in self._fields_}


class StereoCamera(C.Structure):
    """cox_stereo_camera."""
    _fields_ = [("camera_model", C.c_int32), ("distortion_model", C.c_int32), ("intrinsics", C.c_double * 4), ("distortion_coeffs", C.c_double * 4)]


class StereoCalibration(C.Structure):
    """cox_stereo_calibration."""
    _fields_ = [("cam", StereoCamera * 2), ("T_cn_cnm1", C.c_double * 16)]


class StereoFilterConfig(C.Structure):
    """cox_stereo_filter_config (include/coxgraph_hip_stereo_filter.h)."""
    _fields_ = [("median_size", C.c_int32), ("speckle_window", C.c_int32), ("speckle_range16", C.c_int32), ("reserved", C.c_uint32)]


class StereoFilterStats(C.Structure):
    """cox_stereo_filter_stats."""
    _fields_ = [(n, C.c_uint64) for n in ("n_median_changed", "n_components", "n_speckle_components", "n_speckle_pixels")] + \
               [(n, C.c_double) for n in ("median_ms", "speckle_ms")]

    def asdict(self):
        return {n: (float(getattr(self, n)) if t is C.c_double else int(getattr(self, n))) for n, t in self._fields_}


STEREO_FILTER_BUFFERS = {"disparity_raw": 0, "disparity_median": 1, "labels": 2}  # cox_stereo_filter_buffer

CAMERA_MODELS = {"pinhole": 0, "omni": 1, "eucm": 2, "ds": 3}
DISTORTION_MODELS = {"radtan": 0, "equidistant": 1, "fov": 2, "none": 3}


def stereo_config(eng, **cfg):
    """cox_stereo_config_default with fields overridden"""
    return _config(eng, StereoConfig, "stereo_config_default", cfg)


def stereo_calibration(chain):
    """a kalibr camchain as a dict (cam0 / cam1 with camera_model, distortion_model, intrinsics, distortion_coeffs, and cam1's
    T_cn_cnm1 as 4 x 4) -> cox_stereo_calibration; a StereoCalibration passes through"""
    if isinstance(chain, StereoCalibration):
        return chain
    c = StereoCalibration()
    for i in (0, 1):
        cam = chain["cam%d" % i]
        c.cam[i].camera_model = CAMERA_MODELS.get(cam.get("camera_model", "pinhole"), -1)
        c.cam[i].distortion_model = DISTORTION_MODELS.get(cam.get("distortion_model", "radtan"), -1)
        c.cam[i].intrinsics[:] = [float(v) for v in cam["intrinsics"]]
        c.cam[i].distortion_coeffs[:] = [float(v) for v in cam["distortion_coeffs"]]
    T = np.asarray(chain["cam1"]["T_cn_cnm1"], np.float64)
    assert T.shape == (4, 4)
    c.T_cn_cnm1[:] = T.ravel().tolist()
    return c


def rectify_maps(eng, calibration, w, h, scale=1.0):
    """cox_stereo_rectify_maps (host only): -> map0, map1 float32 [h, w, 2], K_rect float32[4], the baseline in metres,
    T_c0_rect float32[7]"""
    calib = stereo_calibration(calibration)
    n = max(int(w), 0) * max(int(h), 0)
    map0, map1 = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    K, B, T = np.zeros(4, np.float32), C.c_float(), np.zeros(7, np.float32)
    eng.call("stereo_rectify_maps", C.byref(calib), C.c_int(w), C.c_int(h), C.c_double(scale), _fp(map0), _fp(map1), _fp(K), C.byref(B), _fp(T))
    return map0.reshape(h, w, 2), map1.reshape(h, w, 2), K, float(B.value), T


class StereoMatcher(_Handle):
    """Dense stereo of w x h 8-bit pairs (cox_stereo_t); cfg are fields of cox_stereo_config.  Either
    calibration (a camchain, rectified here with `scale`), or maps = (map0, map1) with K_rect and baseline_m, or neither of them
    with K_rect and baseline_m: the pairs are rectified already.  After a calibration, K_rect, baseline_m and T_c0_rect are its."""
    _destroy = "stereo_destroy"
    _hattr = "h_"  # (h is the image height)
    h_ = None

    def __init__(self, eng, w, h, calibration=None, maps=None, K_rect=None, baseline_m=None, scale=1.0, device=0, **cfg):
        self.eng, self.w, self.h = eng, int(w), int(h)
        self.cfg = stereo_config(eng, **cfg)
        self.T_c0_rect = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
        if calibration is not None:
            assert maps is None
            m0, m1, K_rect, baseline_m, self.T_c0_rect = rectify_maps(eng, calibration, w, h, scale)
            maps = (m0, m1)
        if maps is not None:
            maps = tuple(np.ascontiguousarray(m, np.float32) for m in maps)
            assert len(maps) == 2 and all(m.size == 2 * self.w * self.h for m in maps)
        self.K_rect = np.ascontiguousarray(K_rect, np.float32)
        assert self.K_rect.shape == (4,)
        self.baseline_m = float(baseline_m)
        self.h_ = C.c_void_p()
        eng.call("stereo_create", C.c_int(device), C.c_int(w), C.c_int(h), C.byref(self.cfg), None if maps is None else _fp(maps[0]),
                 None if maps is None else _fp(maps[1]), _fp(self.K_rect), C.c_float(self.baseline_m), C.byref(self.h_))
        self._keep = []  # host arrays of the frames in flight

    def close(self):
        super().close()
        self._keep = []

    def compute_async(self, left, right):
        """cox_stereo_compute without the wait: -> (depth, rgba, disparity), complete after sync()"""
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        assert left.shape == (self.h, self.w) and right.shape == (self.h, self.w)
        depth = np.empty((self.h, self.w), np.float32)
        rgba = np.empty((self.h, self.w, 4), np.uint8)
        disparity = np.empty((self.h, self.w), np.uint16)
        self._call("stereo_compute", _fp(left), _fp(right), _fp(depth), _fp(rgba), _fp(disparity))
        self._keep.append((left, right, depth, rgba, disparity))
        return depth, rgba, disparity

    def compute(self, left, right):
        """one pair of [h, w] uint8 images -> depth float32 [h, w] (NaN: nothing), rgba uint8 [h, w, 4], disparity uint16 [h, w]
        in 1/16 px (0xFFFF: invalid)"""
        out = self.compute_async(left, right)
        self.sync()
        return out

    def compute_dev(self, left, right, depth, rgba=None, disparity=None, stream=None):
        """cox_stereo_compute_dev: torch tensors on the matcher's GPU or raw device pointers (ints); ordered behind `stream` (a
        torch stream, a raw hipStream_t or None = the null stream), which then waits until the frame has read left and right.
        The outputs are complete after sync()."""
        self._call("stereo_compute_dev", _ptr(left), _ptr(right), _ptr(depth), _ptr(rgba), _ptr(disparity), _stream(stream))

    def stream(self):
        """the matcher's hipStream_t as an int"""
        return int(self.eng.fn("stereo_stream", C.c_void_p)(self.h_) or 0)

    def sync(self):
        self._call("stereo_sync")
        self._keep = []

    def last_stats(self):
        st = StereoStats()
        self._call("stereo_last_stats", C.byref(st))
        return st.asdict()

    def download(self, which):
        """an intermediate of the last frame: "rect_left" / "rect_right" uint8 [h, w], "cost_sum" uint16 [h, w, D], "disparity"
        uint16 [h, w]"""
        k = STEREO_BUFFERS[which] if isinstance(which, str) else int(which)
        shape, dt = {0: ((self.h, self.w), np.uint8), 1: ((self.h, self.w), np.uint8), 2: ((self.h, self.w, int(self.cfg.n_disparities)), np.uint16),
                     3: ((self.h, self.w), np.uint16)}[k]
        out = np.empty(shape, dt)
        self._call("stereo_download", C.c_int(k), _fp(out), C.c_uint64(out.nbytes))
        return out

    # the filters on the disparity (include/coxgraph_hip_stereo_filter.h); both are off at first
    def set_filters(self, median_size=0, speckle_window=0, speckle_range16=16):
        """cox_stereo_set_filters: a 3 x 3 median (median_size 3) and a speckle filter (components of at most speckle_window pixels,
        linked by differences of at most speckle_range16 sixteenths of a pixel); holds from the next frame"""
        c = StereoFilterConfig(int(median_size), int(speckle_window), int(speckle_range16), 0)
        self._call("stereo_set_filters", C.byref(c))

    @property
    def filters(self):
        """the setting as a StereoFilterConfig"""
        c = StereoFilterConfig()
        self._call("stereo_get_filters", C.byref(c))
        return c

    def filter_stats(self):
        """cox_stereo_filter_last_stats as a dict; zeros when the last frame ran unfiltered"""
        st = StereoFilterStats()
        self._call("stereo_filter_last_stats", C.byref(st))
        return st.asdict()

    def filter_download(self, which):
        """a filter stage of the last frame: "disparity_raw" (before 7a) / "disparity_median" (after 7a) uint16 [h, w], "labels"
        uint32 [h, w] (0xFFFFFFFF: invalid)"""
        k = STEREO_FILTER_BUFFERS[which] if isinstance(which, str) else int(which)
        out = np.empty((self.h, self.w), np.uint32 if k == 2 else np.uint16)
        self._call("stereo_filter_download", C.c_int(k), _fp(out), C.c_uint64(out.nbytes))
        return out


# ---- aligning two submaps without a prior (include/coxgraph_hip_align.h) -----
ALIGN_Q, ALIGN_MAX_CANDIDATES, ALIGN_MAX_KEEP, ALIGN_MAX_LEVELS = 1024, 1 << 20, 64, 16


class AlignConfig(C.Structure):
    """cox_align_config."""
    _fields_ = [("inlier_distance", C.c_float), ("pad", C.c_uint32), ("no_correspondence_cost", C.c_double)]


class AlignScore(C.Structure):
    """cox_align_score."""
    _fields_ = [("score", C.c_uint64), ("n_corr", C.c_uint32), ("n_inlier", C.c_uint32), ("cost", C.c_double)]


class AlignSearchConfig(C.Structure):
    """cox_align_search_config."""
    _fields_ = [("center", C.c_double * 4), ("half_extent", C.c_double * 4), ("step", C.c_double * 4), ("inlier_distance", C.c_float), ("tau_min", C.c_float),
                ("levels", C.c_uint32), ("keep", C.c_uint32), ("min_corr", C.c_uint32), ("pad", C.c_uint32)]


class AlignLevel(C.Structure):
    """cox_align_level."""
    _fields_ = [("n_candidates", C.c_uint64), ("step", C.c_double * 4), ("inlier_distance", C.c_float), ("n_kept", C.c_uint32),
                ("kept_index", C.c_uint32 * ALIGN_MAX_KEEP), ("kept_pose", C.c_double * (4 * ALIGN_MAX_KEEP)), ("kept_score", AlignScore * ALIGN_MAX_KEEP)]


ALIGN_SCORE_DTYPE = np.dtype([("score", np.uint64), ("n_corr", np.uint32), ("n_inlier", np.uint32), ("cost", np.float64)])
assert ALIGN_SCORE_DTYPE.itemsize == 24 == C.sizeof(AlignScore)


def align_config(eng, **cfg):
    """cox_align_config_default with overrides."""
    return _config(eng, AlignConfig, "align_config_default", cfg)


def _pose4(p):
    p = np.ascontiguousarray(p, np.float64)
    assert p.shape == (4,)
    return p


def align_grid(eng, center, half_extent, step):
    """cox_align_grid: float64 [n,4] poses x, y, z, yaw around center, x slowest and yaw fastest.  Needs no GPU."""
    c, h, s = _pose4(center), _pose4(half_extent), _pose4(step)
    n = C.c_uint64()
    eng.call("align_grid", _fp(c), _fp(h), _fp(s), None, C.c_uint64(0), C.byref(n))
    out = np.zeros((int(n.value), 4), np.float64)
    eng.call("align_grid", _fp(c), _fp(h), _fp(s), _fp(out), C.c_uint64(len(out)), C.byref(n))
    return out


def align_select(eng, scores, min_corr, keep):
    """cox_align_select on a structured array of ALIGN_SCORE_DTYPE: the kept indices (uint32), best first.  Needs no GPU."""
    scores = np.ascontiguousarray(scores, ALIGN_SCORE_DTYPE)
    idx, n = np.zeros(ALIGN_MAX_KEEP, np.uint32), C.c_uint32()
    eng.call("align_select", _fp(scores), C.c_uint64(len(scores)), C.c_uint32(min_corr), C.c_uint32(keep), _fp(idx), C.byref(n))
    return idx[:int(n.value)].copy()


class SubmapAligner(_Handle):
    """Scores candidate reference poses of one (reference points, reading layer) pair and searches them coarse to fine
    (cox_align_t): cfg are fields of cox_align_config."""
    _destroy = "align_destroy"

    def _guard(self, name):
        """As _Handle._guard with _borrows = ("ref", "reading")."""
        if not self.ref.h or not self.reading.h:
            raise CoxError(-1, name + " (the layer is closed)")
        return self.h

    def __init__(self, eng, ref_points, reading_layer, **cfg):
        self.eng, self.ref, self.reading = eng, ref_points, reading_layer
        self.cfg = align_config(eng, **cfg)
        self.samples = None
        self.h = C.c_void_p()
        eng.call("align_create", ref_points.h, reading_layer.h, C.byref(self.cfg), C.byref(self.h))

    def set_samples(self, sample_idx):
        """The points of a sweep as indices into the reference set (repeats allowed); None: all points in order."""
        if sample_idx is None:
            self._call("align_set_samples", None, C.c_uint64(0))
            self.samples = None
            return
        si = np.ascontiguousarray(sample_idx, np.uint32)
        self._call("align_set_samples", _fp(si), C.c_uint64(si.shape[0]))
        self.samples = si

    def sweep(self, poses_ref, pose_read=(0, 0, 0, 0), inlier_distance=None):
        """cox_align_sweep: one record of ALIGN_SCORE_DTYPE per candidate reference pose [M,4]."""
        pr = np.ascontiguousarray(poses_ref, np.float64).reshape(-1, 4)
        out = np.zeros(len(pr), ALIGN_SCORE_DTYPE)
        tau = self.cfg.inlier_distance if inlier_distance is None else inlier_distance
        self._call("align_sweep", _fp(_pose4(pose_read)), _fp(pr), C.c_uint64(len(pr)), C.c_float(tau), _fp(out))
        return out

    def search(self, center, half_extent, step, levels=4, keep=8, min_corr=0, tau_min=None, pose_read=(0, 0, 0, 0), inlier_distance=None, trace=False,
               refine=False):
        """cox_align_search: dict(poses [k,4] and scores [k] of the last level's kept candidates, best first; n_found; best = poses[0]
        or None).  trace=True adds levels = [dict(n_candidates, inlier_distance, step, kept_index, kept_pose, kept_score)].
        refine=True polishes the best pose with the registration cost (Registration.normal_eq under
        posegraph.trust_region_minimize, the reading pose fixed) and adds refined (pose), cost_before, cost_after."""
        tau = self.cfg.inlier_distance if inlier_distance is None else inlier_distance
        sc = AlignSearchConfig((C.c_double * 4)(*_pose4(center)), (C.c_double * 4)(*_pose4(half_extent)), (C.c_double * 4)(*_pose4(step)), tau,
                               tau / 4 if tau_min is None else tau_min, levels, keep, min_corr, 0)
        pose_read = _pose4(pose_read)
        k = max(1, min(int(keep), ALIGN_MAX_KEEP))
        poses, scores, n = np.zeros((k, 4), np.float64), np.zeros(k, ALIGN_SCORE_DTYPE), C.c_uint32()
        tr = (AlignLevel * (int(levels) + 1))() if trace and 0 <= levels <= ALIGN_MAX_LEVELS else None
        self._call("align_search", _fp(pose_read), C.byref(sc), _fp(poses), _fp(scores), C.byref(n), tr)
        n = int(n.value)
        out = dict(poses=poses[:n], scores=scores[:n], n_found=n, best=poses[0].copy() if n else None)
        if tr is not None:
            out["levels"] = []
            for t in tr:
                if t.n_candidates == 0:
                    break
                kk = int(t.n_kept)
                rec = np.frombuffer(t.kept_score, ALIGN_SCORE_DTYPE)[:kk].copy()
                out["levels"].append(dict(n_candidates=int(t.n_candidates), inlier_distance=float(t.inlier_distance), step=np.array(t.step[:]),
                                          kept_index=np.array(t.kept_index[:kk], np.uint32), kept_pose=np.array(t.kept_pose[:4 * kk]).reshape(kk, 4),
                                          kept_score=rec))
        if refine and n:
            out.update(self.refine(out["best"], pose_read))
        return out

    def refine(self, pose_ref, pose_read=(0, 0, 0, 0)):
        """The registration cost minimised over the reference pose from pose_ref: dict(refined, cost_before, cost_after).  The
        minimiser takes monotonic steps only, so cost_after <= cost_before."""
        from . import posegraph
        pose_read = _pose4(pose_read)
        reg = Registration(self.eng, self.ref, self.reading, self.cfg.no_correspondence_cost)
        try:
            def evaluate(x):
                H, b, cost, _ = reg.normal_eq(x, pose_read, self.samples)
                return cost, b[:4].copy(), H[:4, :4].copy()
            x, summary = posegraph.trust_region_minimize(evaluate, _pose4(pose_ref), lambda x, d: x + d)
        finally:
            reg.close()
        return dict(refined=x, cost_before=float(summary["initial_cost"]), cost_after=float(summary["final_cost"]))

    def kernel_time(self, reset=False):
        """(milliseconds of the sweeps' kernels, sweeps) since creation or the last reset."""
        ms, n = C.c_double(), C.c_uint64()
        self._call("align_kernel_time", C.byref(ms), C.byref(n), C.c_int(int(reset)))
        return float(ms.value), int(n.value)


# ---- comparing two layers (include/coxgraph_hip_compare.h) -----------------
COMPARE_MAX_TRANSFORMS, COMPARE_HIST_BINS, COMPARE_Q_PER_METRE, COMPARE_Q_SATURATED = 1024, 22, 65536, 1 << 20
COMPARE_IGNORE = {"all": 0, "behind_test": 1, "behind_gt": 2, "behind_all": 3}  # cox_compare_ignore (voxblox VoxelEvaluationMode)
COMPARE_SAMPLE = {"nearest": 0, "trilinear": 1}                                  # cox_compare_sample
COMPARE_COUNTS = ("n_a_observed", "n_overlap", "n_ignored", "n_evaluated", "sum_q", "sum_q2_lo", "sum_q2_hi", "n_near_a", "n_near_b",
                  "n_a_surface_in_b_free", "n_b_surface_in_a_free", "n_agree")
# classes in the colour word of an error layer
COMPARE_UNOBSERVED, COMPARE_NO_COUNTERPART, COMPARE_IGNORED, COMPARE_EVALUATED, COMPARE_A_IN_B_FREE, COMPARE_B_IN_A_FREE = 0, 1, 2, 3, 4, 8


class CompareConfig(C.Structure):
    """cox_compare_config."""
    _fields_ = [("surface_distance", C.c_float), ("free_distance", C.c_float), ("agree_distance", C.c_float), ("min_weight", C.c_float)]


class CompareStats(C.Structure):
    """cox_compare_stats."""
    _fields_ = [(n, C.c_uint64) for n in COMPARE_COUNTS] + [("hist", C.c_uint64 * COMPARE_HIST_BINS), ("min_q", C.c_uint32), ("max_q", C.c_uint32)]


COMPARE_STATS_DTYPE = np.dtype([(n, np.uint64) for n in COMPARE_COUNTS] + [("hist", np.uint64, (COMPARE_HIST_BINS,)), ("min_q", np.uint32), ("max_q", np.uint32)])
assert COMPARE_STATS_DTYPE.itemsize == 280 == C.sizeof(CompareStats)


def compare_config(eng, **cfg):
    """cox_compare_config_default with overrides (a distance of 0 stands for its default)."""
    return _config(eng, CompareConfig, "compare_config_default", cfg)


def compare_rmse(rec):
    """The root mean square of |e| in metres from one record: sqrt((hi * 2^20 + lo) / n_evaluated) / 65536, the sum in Python
    integers and the rest in float64.  NaN when nothing was evaluated."""
    n = int(rec["n_evaluated"])
    if n == 0:
        return float("nan")
    total = (int(rec["sum_q2_hi"]) << 20) + int(rec["sum_q2_lo"])
    return float(np.sqrt(np.float64(total) / np.float64(n)) / np.float64(COMPARE_Q_PER_METRE))


def compare_conflict_ratio(rec):
    """(n_a_surface_in_b_free + n_b_surface_in_a_free) / (n_near_a + n_near_b); NaN when no overlapping voxel is near a surface."""
    den = int(rec["n_near_a"]) + int(rec["n_near_b"])
    return (int(rec["n_a_surface_in_b_free"]) + int(rec["n_b_surface_in_a_free"])) / den if den else float("nan")


def _transforms(T):
    """None, one pose [7] or poses [n,7] as (contiguous float32 [n,7] or None, n)."""
    if T is None:
        return None, 1
    T = np.ascontiguousarray(T, np.float32)
    if T.ndim == 1:
        T = T.reshape(1, -1)
    assert T.ndim == 2 and T.shape[1] == 7
    return T, len(T)


class LayerComparer(_Handle):
    """Compares test layer A against reference layer B (cox_compare_t): cfg are fields of cox_compare_config."""
    _destroy = "compare_destroy"

    def _guard(self, name):
        """As _Handle._guard with _borrows = ("A", "B")."""
        if not self.A.h or not self.B.h:
            raise CoxError(-1, name + " (the layer is closed)")
        return self.h

    def __init__(self, eng, A, B, **cfg):
        self.eng, self.A, self.B = eng, A, B
        asked = compare_config(eng, **cfg)
        self.h = C.c_void_p()
        eng.call("compare_create", A.h, B.h, C.byref(asked), C.byref(self.h))
        self.cfg = CompareConfig()
        self._call("compare_get_config", C.byref(self.cfg))

    def run(self, T=None, ignore="all", sample="nearest"):
        """cox_compare_run: one record of COMPARE_STATS_DTYPE per transform T_B_A ([7] or [n,7]); None: the same-frame compare."""
        T, n = _transforms(T)
        out = np.zeros(n, COMPARE_STATS_DTYPE)
        self._call("compare_run", _opt(T), C.c_uint64(n), C.c_int(COMPARE_IGNORE[ignore]), C.c_int(COMPARE_SAMPLE[sample]), _fp(out))
        return out

    def error_layer(self, T=None, ignore="all", sample="nearest"):
        """cox_compare_error_layer: a new Layer with A's blocks: distance = e, weight = 1 where evaluated, colour word = class."""
        T, n = _transforms(T)
        assert n == 1
        out = Layer._adopt(self.eng, C.c_void_p(), voxel_size=self.A.voxel_size)
        self._call("compare_error_layer", _opt(T), C.c_int(COMPARE_IGNORE[ignore]), C.c_int(COMPARE_SAMPLE[sample]), C.byref(out.h))
        return out

    def kernel_time(self, reset=False):
        """(milliseconds of the compare kernels, calls that ran one) since creation or the last reset."""
        ms, n = C.c_double(), C.c_uint64()
        self._call("compare_kernel_time", C.byref(ms), C.byref(n), C.c_int(int(reset)))
        return float(ms.value), int(n.value)


# ---- wire-format helpers (voxblox_msgs/Block data words) -----------------------------------------
def words_to_fields(vox):
    """uint32[...,3] wire words -> (distance f32, weight f32, rgba u8[...,4])."""
    vox = np.ascontiguousarray(vox, np.uint32)
    d = vox[..., 0].copy().view(np.float32)
    w = vox[..., 1].copy().view(np.float32)
    c = vox[..., 2]
    rgba = np.stack([(c >> 24) & 255, (c >> 16) & 255, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8)
    return d, w, rgba
