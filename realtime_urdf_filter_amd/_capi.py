"""ctypes binding of the C ABI in include/rtuf.h (librtuf.so, built by csrc/build.sh).

This is the same binding a maintainer of the reference would write for a Python host
(INTEGRATION.md); the C++ facade binds the identical symbols.  The library is the product
path: if it is missing or no GPU is visible, construction fails loudly -- there is no CPU
fallback anywhere in this package.
"""
import ctypes
import os

import numpy as np

_LIB_PATH = os.environ.get("RTUF_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "librtuf.so")

RTUF_OK = 0
RTUF_ERR_NO_DEVICE = -2
OP_NONE, OP_SCALE, OP_TRANSLATE = 0, 1, 2
FLAG_TWO_KERNEL = 2
FLAG_STRICT_GRID = 4
ABI_VERSION = 6
# rtuf_batch_status_device: bits of a batch slot's device status word (0 = the planes are final)
STATUS_PENDING_MASK = 0xffff
STATUS_BIN_OVERFLOW, STATUS_CLIP_OVERFLOW, STATUS_LIST_OVERFLOW, STATUS_GRID_SHORT, STATUS_UNCOVERED = 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20

#: every symbol include/rtuf.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "rtuf_default_params", "rtuf_abi_version", "rtuf_create", "rtuf_destroy", "rtuf_last_error",
    "rtuf_set_params", "rtuf_add_model", "rtuf_add_link", "rtuf_add_draw", "rtuf_finalize_models",
    "rtuf_num_links", "rtuf_num_triangles", "rtuf_num_vertices", "rtuf_set_stream_models", "rtuf_set_camera",
    "rtuf_projection_from_intrinsics", "rtuf_set_link_poses", "rtuf_set_cameras", "rtuf_set_camera_shift", "rtuf_set_link_poses_batch", "rtuf_set_kinematics", "rtuf_set_joint_positions", "rtuf_debug_read_poses", "rtuf_filter_batch",
    "rtuf_filter_batch_device", "rtuf_filter_batch_u16", "rtuf_filter_batch_device_u16", "rtuf_filter", "rtuf_get_masked_depth", "rtuf_get_mask", "rtuf_sync",
    "rtuf_stream", "rtuf_get_stats", "rtuf_enable_timing", "rtuf_debug_read_zsurface",
    "rtuf_filter_batch_async", "rtuf_filter_batch_u16_async", "rtuf_wait_oldest", "rtuf_host_alloc", "rtuf_host_free",
    "rtuf_mask_bits_words", "rtuf_filter_batch_bits_async", "rtuf_filter_batch_bits_u16_async", "rtuf_filter_batch_device_bits",
    "rtuf_filter_batch_device_bits_u16", "rtuf_expand_mask_bits", "rtuf_order_stream_after_batches", "rtuf_batch_status_device",
    "rtuf_set_link_labels", "rtuf_filter_batch_device_labels", "rtuf_filter_batch_device_u16_labels", "rtuf_filter_batch_labels",
    "rtuf_filter_batch_u16_labels", "rtuf_set_link_thresholds", "rtuf_clear_link_thresholds",
    "rtuf_render_batch_device", "rtuf_render_batch_device_u16", "rtuf_render_batch", "rtuf_render_batch_u16",
    "rtuf_link_residuals_batch_device", "rtuf_link_residuals_batch_device_u16", "rtuf_link_residuals_batch", "rtuf_link_residuals_batch_u16",
    "rtuf_set_cloud_intrinsics", "rtuf_cloud_batch_device", "rtuf_cloud_batch_device_u16", "rtuf_cloud_compact_batch_device",
    "rtuf_cloud_compact_batch_device_u16", "rtuf_cloud_batch", "rtuf_cloud_batch_u16", "rtuf_cloud_compact_batch", "rtuf_cloud_compact_batch_u16",
    "rtuf_set_link_spheres", "rtuf_link_clearance_batch_device", "rtuf_link_clearance_batch_device_u16", "rtuf_link_clearance_batch",
    "rtuf_link_clearance_batch_u16", "rtuf_set_link_padding", "rtuf_clear_link_padding",
    "rtuf_set_scene_planes", "rtuf_set_scene_planes_device", "rtuf_get_scene_planes", "rtuf_get_scene_planes_device",
    "rtuf_set_scene_margins", "rtuf_clear_scene", "rtuf_learn_scene_batch", "rtuf_learn_scene_batch_u16",
    "rtuf_learn_scene_batch_device", "rtuf_learn_scene_batch_device_u16",
    "rtuf_set_point_transforms", "rtuf_points_batch_device", "rtuf_points_batch",
    "rtuf_set_voxel_grid", "rtuf_set_voxel_transforms", "rtuf_voxel_clear", "rtuf_voxel_insert_batch", "rtuf_voxel_insert_batch_u16",
    "rtuf_voxel_insert_batch_device", "rtuf_voxel_insert_batch_device_u16", "rtuf_voxel_insert_points_device", "rtuf_voxel_grid_device",
    "rtuf_get_voxel_grid",
    "rtuf_voxel_carve_batch_device", "rtuf_voxel_carve_batch_device_u16", "rtuf_voxel_carve_batch", "rtuf_voxel_carve_batch_u16",
    "rtuf_voxel_free_device", "rtuf_get_voxel_free",
]

# point list batches (include/rtuf.h, POINT LIST BATCHES): the verdict of a point, and the pixel of one that is not judged
POINT_KEPT, POINT_FILTERED, POINT_OUTSIDE = 0, 1, 2
POINT_NO_PIXEL = 0xFFFFFFFF

# rtuf_link_residuals (include/rtuf.h, LINK RESIDUAL TABLES): one 64-byte row per (stream, label)
LINK_RESIDUALS_DTYPE = np.dtype([("pixels", "<u8"), ("invalid", "<u8"), ("filtered", "<u8"), ("in_front", "<u8"), ("behind", "<u8"),
                                 ("agree", "<u8"), ("sum_residual", "<i8"), ("sum_abs_residual", "<u8")])
# rtuf_link_clearance (include/rtuf.h, LINK CLEARANCE TABLES): one 16-byte row per (stream, label)
LINK_CLEARANCE_DTYPE = np.dtype([("clearance", "<f4"), ("pixel", "<u4"), ("sphere", "<u4"), ("points_within", "<u4")])


class Params(ctypes.Structure):
    _fields_ = [("near_plane", ctypes.c_float), ("far_plane", ctypes.c_float),
                ("depth_distance_threshold", ctypes.c_float), ("filter_replace_value", ctypes.c_float),
                ("flags", ctypes.c_uint32), ("bin_capacity", ctypes.c_uint32),
                ("max_inflight_streams", ctypes.c_uint32), ("pipelines", ctypes.c_uint32),
                ("raster_lanes", ctypes.c_uint32), ("memory_limit_mb", ctypes.c_uint32),
                ("silhouette_dilation_px", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 1)]


class Stats(ctypes.Structure):
    _fields_ = [("triangles_submitted", ctypes.c_uint64), ("triangles_binned", ctypes.c_uint64),
                ("bin_entries", ctypes.c_uint64), ("triangles_clipped", ctypes.c_uint64),
                ("max_bin_fill", ctypes.c_uint32), ("bin_capacity", ctypes.c_uint32),
                ("regrowths", ctypes.c_uint32), ("max_fbin_fill", ctypes.c_uint32), ("fragments_binned", ctypes.c_uint64),
                ("ms_pose", ctypes.c_float), ("ms_setup", ctypes.c_float), ("ms_raster", ctypes.c_float),
                ("ms_compare", ctypes.c_float), ("ms_total", ctypes.c_float), ("ms_clip", ctypes.c_float),
                ("timed_batches", ctypes.c_uint64), ("sum_ms_pose", ctypes.c_double), ("sum_ms_setup", ctypes.c_double),
                ("sum_ms_raster", ctypes.c_double), ("sum_ms_compare", ctypes.c_double), ("sum_ms_total", ctypes.c_double),
                ("sum_ms_clip", ctypes.c_double),
                ("device_bytes", ctypes.c_uint64), ("occluded_entries", ctypes.c_uint64),
                ("cover_tiles", ctypes.c_uint32), ("exact_tiles", ctypes.c_uint32),
                ("work_items", ctypes.c_uint32), ("zero_survivor_items", ctypes.c_uint32),
                ("cover_pass", ctypes.c_uint32), ("counter_blocks", ctypes.c_uint32),
                ("raster_atomics", ctypes.c_uint64), ("drawn_pixels", ctypes.c_uint64),
                ("raster_lanes", ctypes.c_uint32), ("launch_group", ctypes.c_uint32), ("groups_last_batch", ctypes.c_uint32),
                ("graphs_enabled", ctypes.c_uint32), ("graph_hits", ctypes.c_uint64), ("graph_misses", ctypes.c_uint64),
                ("lanes_side_by_side", ctypes.c_uint32),
                ("batch_status", ctypes.c_uint32), ("batch_reruns", ctypes.c_uint32), ("over_memory_limit", ctypes.c_uint32),
                ("copy_streams_side_by_side", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class RtufError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("rtuf error %d: %s" % (code, message))
        self.code = code


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  A ROCm PyTorch wheel carries its own libamdhip64 / libhsa-runtime64 and
    loads them by path on `import torch`; librtuf.so is linked against the same soname (libamdhip64.so.7), so
    whichever of the two is loaded first decides which runtime librtuf binds to -- and if that is the system
    copy, torch later brings a second runtime into the process, which finds no GPU.  When such a wheel is
    installed and torch is not loaded yet, its runtime is mapped first (without importing torch), so both
    orders of use end up on the same runtime.  Without PyTorch the system runtime (/opt/rocm) is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        ctypes.CDLL(hip, mode=ctypes.RTLD_GLOBAL)


def load_library(path=None):
    """Loads librtuf.so (no GPU needed for loading; rtuf_create needs one)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or _LIB_PATH
    if not os.path.exists(p):
        raise RtufError(-100, "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)" % p)
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(p)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.rtuf_default_params.argtypes = [ctypes.POINTER(Params)]
    lib.rtuf_default_params.restype = None
    lib.rtuf_abi_version.restype = ci
    lib.rtuf_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci, ctypes.POINTER(Params)]
    lib.rtuf_destroy.argtypes = [vp]
    lib.rtuf_destroy.restype = None
    lib.rtuf_last_error.argtypes = [vp]
    lib.rtuf_last_error.restype = ctypes.c_char_p
    lib.rtuf_set_params.argtypes = [vp, ctypes.POINTER(Params)]
    lib.rtuf_add_model.argtypes = [vp]
    lib.rtuf_add_link.argtypes = [vp, ci]
    lib.rtuf_add_draw.argtypes = [vp, ci, ci, ci, vp, vp, ci, vp, ci]
    lib.rtuf_finalize_models.argtypes = [vp]
    lib.rtuf_num_links.argtypes = [vp, ci]
    lib.rtuf_num_triangles.argtypes = [vp]
    lib.rtuf_num_triangles.restype = ctypes.c_int64
    lib.rtuf_num_vertices.argtypes = [vp]
    lib.rtuf_num_vertices.restype = ctypes.c_int64
    lib.rtuf_set_stream_models.argtypes = [vp, ci, vp, ci]
    lib.rtuf_set_camera.argtypes = [vp, ci, vp, vp, vp]
    lib.rtuf_projection_from_intrinsics.argtypes = [cd, cd, cd, cd, cd, cd, ci, ci, cd, cd, vp, vp, vp]
    lib.rtuf_projection_from_intrinsics.restype = None
    lib.rtuf_set_link_poses.argtypes = [vp, ci, ci, vp, ci]
    lib.rtuf_set_cameras.argtypes = [vp, ci, ci, vp, vp, vp]
    lib.rtuf_set_link_poses_batch.argtypes = [vp, ci, ci, ci, vp, ci]
    lib.rtuf_set_camera_shift.argtypes = [vp, ci, ci, vp, vp]
    lib.rtuf_set_kinematics.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, ci]
    lib.rtuf_set_joint_positions.argtypes = [vp, ci, ci, ci, vp, vp, ci]
    lib.rtuf_debug_read_poses.argtypes = [vp, ci, vp, vp]
    lib.rtuf_filter_batch.argtypes = [vp, ci, vp, vp, vp]
    lib.rtuf_filter_batch_device.argtypes = [vp, ci, vp, vp, vp]
    lib.rtuf_filter_batch_u16.argtypes = [vp, ci, vp, vp, vp]
    lib.rtuf_filter_batch_device_u16.argtypes = [vp, ci, vp, vp, vp]
    lib.rtuf_filter.argtypes = [vp, vp, vp, ci, ci]
    lib.rtuf_get_masked_depth.argtypes = [vp]
    lib.rtuf_get_masked_depth.restype = ctypes.POINTER(ctypes.c_float)
    lib.rtuf_get_mask.argtypes = [vp]
    lib.rtuf_get_mask.restype = ctypes.POINTER(ctypes.c_uint8)
    lib.rtuf_sync.argtypes = [vp]
    lib.rtuf_stream.argtypes = [vp]
    lib.rtuf_stream.restype = vp
    lib.rtuf_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.rtuf_enable_timing.argtypes = [vp, ci]
    lib.rtuf_debug_read_zsurface.argtypes = [vp, ci, vp]
    lib.rtuf_filter_batch_async.argtypes = [vp, ci, vp, vp, vp]
    lib.rtuf_filter_batch_u16_async.argtypes = [vp, ci, vp, vp, vp]
    lib.rtuf_wait_oldest.argtypes = [vp]
    lib.rtuf_host_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.rtuf_host_free.argtypes = [vp, vp]
    lib.rtuf_mask_bits_words.argtypes = [ci, ci]
    lib.rtuf_mask_bits_words.restype = ctypes.c_size_t
    lib.rtuf_filter_batch_bits_async.argtypes = [vp, ci, vp, vp]
    lib.rtuf_filter_batch_bits_u16_async.argtypes = [vp, ci, vp, vp]
    lib.rtuf_filter_batch_device_bits.argtypes = [vp, ci, vp, vp]
    lib.rtuf_filter_batch_device_bits_u16.argtypes = [vp, ci, vp, vp]
    lib.rtuf_expand_mask_bits.argtypes = [vp, ci, vp, ci, ci, ctypes.c_float, vp, vp]
    lib.rtuf_order_stream_after_batches.argtypes = [vp, vp]
    lib.rtuf_batch_status_device.argtypes = [vp, ctypes.POINTER(vp)]
    lib.rtuf_set_link_labels.argtypes = [vp, ci, vp, ci]
    lib.rtuf_filter_batch_device_labels.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.rtuf_filter_batch_device_u16_labels.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.rtuf_filter_batch_labels.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.rtuf_filter_batch_u16_labels.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.rtuf_render_batch_device.argtypes = [vp, ci, vp, vp, ctypes.c_float]
    lib.rtuf_render_batch_device_u16.argtypes = [vp, ci, vp, vp, ctypes.c_float]
    lib.rtuf_render_batch.argtypes = [vp, ci, vp, vp, ctypes.c_float]
    lib.rtuf_render_batch_u16.argtypes = [vp, ci, vp, vp, ctypes.c_float]
    lib.rtuf_link_residuals_batch_device.argtypes = [vp, ci, vp, vp, ci]
    lib.rtuf_link_residuals_batch_device_u16.argtypes = [vp, ci, vp, vp, ci]
    lib.rtuf_link_residuals_batch.argtypes = [vp, ci, vp, vp, ci]
    lib.rtuf_link_residuals_batch_u16.argtypes = [vp, ci, vp, vp, ci]
    lib.rtuf_set_cloud_intrinsics.argtypes = [vp, ci, ci, vp]
    lib.rtuf_cloud_batch_device.argtypes = [vp, ci, vp, vp]
    lib.rtuf_cloud_batch_device_u16.argtypes = [vp, ci, vp, vp]
    lib.rtuf_cloud_compact_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, ci]
    lib.rtuf_cloud_compact_batch_device_u16.argtypes = [vp, ci, vp, vp, vp, vp, ci]
    lib.rtuf_cloud_batch.argtypes = [vp, ci, vp, vp]
    lib.rtuf_cloud_batch_u16.argtypes = [vp, ci, vp, vp]
    lib.rtuf_cloud_compact_batch.argtypes = [vp, ci, vp, vp, vp, vp, ci]
    lib.rtuf_cloud_compact_batch_u16.argtypes = [vp, ci, vp, vp, vp, vp, ci]
    lib.rtuf_set_link_spheres.argtypes = [vp, ci, vp, vp, ci]
    lib.rtuf_link_clearance_batch_device.argtypes = [vp, ci, vp, vp, ci, ctypes.c_float]
    lib.rtuf_link_clearance_batch_device_u16.argtypes = [vp, ci, vp, vp, ci, ctypes.c_float]
    lib.rtuf_link_clearance_batch.argtypes = [vp, ci, vp, vp, ci, ctypes.c_float]
    lib.rtuf_link_clearance_batch_u16.argtypes = [vp, ci, vp, vp, ci, ctypes.c_float]
    lib.rtuf_set_link_thresholds.argtypes = [vp, ci, vp, ci]
    lib.rtuf_clear_link_thresholds.argtypes = [vp, ci]
    lib.rtuf_set_link_padding.argtypes = [vp, ci, vp, ci]
    lib.rtuf_clear_link_padding.argtypes = [vp, ci]
    lib.rtuf_set_scene_planes.argtypes = [vp, ci, ci, vp]
    lib.rtuf_set_scene_planes_device.argtypes = [vp, ci, ci, vp]
    lib.rtuf_get_scene_planes.argtypes = [vp, ci, ci, vp]
    lib.rtuf_get_scene_planes_device.argtypes = [vp, ci, ci, vp]
    lib.rtuf_set_scene_margins.argtypes = [vp, ci, ci, vp]
    lib.rtuf_clear_scene.argtypes = [vp, ci, ci]
    lib.rtuf_learn_scene_batch.argtypes = [vp, ci, vp]
    lib.rtuf_learn_scene_batch_u16.argtypes = [vp, ci, vp]
    lib.rtuf_learn_scene_batch_device.argtypes = [vp, ci, vp]
    lib.rtuf_learn_scene_batch_device_u16.argtypes = [vp, ci, vp]
    lib.rtuf_set_point_transforms.argtypes = [vp, ci, ci, vp]
    lib.rtuf_points_batch_device.argtypes = [vp, ci, vp, vp, ci, ci, vp, vp, vp]
    lib.rtuf_points_batch.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp]
    lib.rtuf_set_voxel_grid.argtypes = [vp, vp, ctypes.c_double, vp, ci]
    lib.rtuf_set_voxel_transforms.argtypes = [vp, ci, ci, vp]
    lib.rtuf_voxel_clear.argtypes = [vp]
    lib.rtuf_voxel_insert_batch.argtypes = [vp, ci, vp, vp]
    lib.rtuf_voxel_insert_batch_u16.argtypes = [vp, ci, vp, vp]
    lib.rtuf_voxel_insert_batch_device.argtypes = [vp, ci, vp, vp]
    lib.rtuf_voxel_insert_batch_device_u16.argtypes = [vp, ci, vp, vp]
    lib.rtuf_voxel_insert_points_device.argtypes = [vp, ci, vp, vp, ci, vp, vp]
    lib.rtuf_voxel_grid_device.argtypes = [vp, vp, vp, vp]
    lib.rtuf_get_voxel_grid.argtypes = [vp, vp, vp]
    lib.rtuf_voxel_carve_batch_device.argtypes = [vp, ci, vp, ctypes.c_double, ci, vp]
    lib.rtuf_voxel_carve_batch_device_u16.argtypes = [vp, ci, vp, ctypes.c_double, ci, vp]
    lib.rtuf_voxel_carve_batch.argtypes = [vp, ci, vp, ctypes.c_double, ci, vp]
    lib.rtuf_voxel_carve_batch_u16.argtypes = [vp, ci, vp, ctypes.c_double, ci, vp]
    lib.rtuf_voxel_free_device.argtypes = [vp, vp, vp]
    lib.rtuf_get_voxel_free.argtypes = [vp, vp]
    if path is None:
        _lib = lib
    return lib


def default_params():
    p = Params()
    load_library().rtuf_default_params(ctypes.byref(p))
    return p


def projection_from_intrinsics(fx, fy, cx, cy, width, height, near=0.1, far=8.0, Tx=0.0, Ty=0.0):
    """getProjectionMatrix (reference src/urdf_filter.cpp:459-501). Returns (P[16], camera_tx, camera_ty)."""
    P = np.zeros(16, np.float64)
    tx, ty = ctypes.c_double(), ctypes.c_double()
    load_library().rtuf_projection_from_intrinsics(fx, fy, cx, cy, Tx, Ty, width, height, near, far,
                                                   P.ctypes.data, ctypes.byref(tx), ctypes.byref(ty))
    return P, tx.value, ty.value


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Context:
    """Thin object wrapper over an rtuf_context handle."""

    def __init__(self, width, height, max_streams=1, device=0, params=None):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        self.width, self.height, self.max_streams = width, height, max_streams
        p = params if params is not None else default_params()
        rc = self._lib.rtuf_create(ctypes.byref(self._h), device, width, height, max_streams, ctypes.byref(p))
        if rc != RTUF_OK:
            raise RtufError(rc, self._lib.rtuf_last_error(None).decode())
        self.params = p
        self._pinned = {}           # host_alloc() blocks: array address -> pointer

    def _check(self, rc):
        if rc < 0:
            raise RtufError(rc, self._lib.rtuf_last_error(self._h).decode())
        return rc

    def close(self):
        if self._h:
            self._lib.rtuf_destroy(self._h)          # also releases host_alloc() blocks still held
            self._h = ctypes.c_void_p()
            self._pinned = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # geometry
    def add_model(self):
        return self._check(self._lib.rtuf_add_model(self._h))

    def add_link(self, model):
        return self._check(self._lib.rtuf_add_link(self._h, model))

    def add_draw(self, model, link, verts, tris, pre_op=OP_NONE, op=(0.0, 0.0, 0.0)):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
        o = np.asarray(op, np.float32)
        return self._check(self._lib.rtuf_add_draw(self._h, model, link, pre_op, _ptr(o), _ptr(v), len(v), _ptr(t), len(t)))

    def finalize_models(self):
        self._check(self._lib.rtuf_finalize_models(self._h))

    def num_links(self, model):
        n = self._lib.rtuf_num_links(self._h, model)
        self._check(min(n, 0))
        return n

    def num_triangles(self):
        return int(self._lib.rtuf_num_triangles(self._h))

    def num_vertices(self):
        return int(self._lib.rtuf_num_vertices(self._h))

    def set_stream_models(self, stream, model_ids):
        m = np.ascontiguousarray(model_ids, np.int32)
        self._check(self._lib.rtuf_set_stream_models(self._h, stream, _ptr(m), len(m)))

    def set_params(self, params):
        self._check(self._lib.rtuf_set_params(self._h, ctypes.byref(params)))
        self.params = params

    # poses
    def set_camera(self, stream, projection=None, camera_offset_inv=None, camera_tf=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float64).reshape(16)
                for a in (projection, camera_offset_inv, camera_tf)]
        self._check(self._lib.rtuf_set_camera(self._h, stream, *[_ptr(a) for a in arrs]))

    def set_link_poses(self, stream, model, link_tf):
        a = np.ascontiguousarray(link_tf, np.float64).reshape(-1, 16)
        self._check(self._lib.rtuf_set_link_poses(self._h, stream, model, _ptr(a), len(a)))

    def set_cameras(self, first_stream, projections=None, camera_offset_inv=None, camera_tf=None):
        arrs = [None if a is None else np.ascontiguousarray(a, np.float64).reshape(-1, 16)
                for a in (projections, camera_offset_inv, camera_tf)]
        n = max(len(a) for a in arrs if a is not None)
        self._check(self._lib.rtuf_set_cameras(self._h, first_stream, n, *[_ptr(a) for a in arrs]))

    def set_camera_shift(self, first_stream, camera_tx, camera_ty):
        """camera_tx_/camera_ty_ (src/urdf_filter.cpp:607-611) for cameras posed by on-device forward kinematics."""
        tx = np.ascontiguousarray(camera_tx, np.float64).reshape(-1)
        ty = np.ascontiguousarray(camera_ty, np.float64).reshape(-1)
        assert len(tx) == len(ty)
        self._check(self._lib.rtuf_set_camera_shift(self._h, first_stream, len(tx), _ptr(tx), _ptr(ty)))

    def set_link_poses_batch(self, first_stream, model, link_tf):
        a = np.ascontiguousarray(link_tf, np.float64)
        n, nl = a.shape[0], a.shape[1]
        self._check(self._lib.rtuf_set_link_poses_batch(self._h, first_stream, n, model, _ptr(a), nl))

    def set_kinematics(self, model, parent, joint_type, joint_origin, joint_axis, link_frame, link_offset):
        """On-device FK tree of a model (see rtuf_set_kinematics)."""
        pa = np.ascontiguousarray(parent, np.int32)
        jt = np.ascontiguousarray(joint_type, np.int32)
        jo = np.ascontiguousarray(joint_origin, np.float64).reshape(-1, 16)
        ja = np.ascontiguousarray(joint_axis, np.float64).reshape(-1, 3)
        lf = np.ascontiguousarray(link_frame, np.int32)
        lo = np.ascontiguousarray(link_offset, np.float64).reshape(-1, 16)
        self._check(self._lib.rtuf_set_kinematics(self._h, model, len(pa), _ptr(pa), _ptr(jt), _ptr(jo), _ptr(ja), _ptr(lf), _ptr(lo), len(lf)))

    def set_joint_positions(self, first_stream, model, q, root_tf=None, camera_frame=-1):
        qa = np.ascontiguousarray(q, np.float64)
        rt = None if root_tf is None else np.ascontiguousarray(root_tf, np.float64).reshape(-1, 16)
        self._check(self._lib.rtuf_set_joint_positions(self._h, first_stream, qa.shape[0], model, _ptr(qa), _ptr(rt), camera_frame))

    def read_poses(self, n, n_links_total):
        tf = np.empty((n, max(n_links_total, 1), 16), np.float64)
        cam = np.empty((n, 16), np.float64)
        self._check(self._lib.rtuf_debug_read_poses(self._h, n, _ptr(tf), _ptr(cam)))
        return tf, cam

    # hot path
    def filter_batch(self, depth, want_mask=True):
        """depth: [n,H,W] float32 host array -> (masked [n,H,W] f32, mask [n,H,W] u8 or None)."""
        d = np.ascontiguousarray(depth, np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        masked = np.empty_like(d)
        mask = np.empty(d.shape, np.uint8) if want_mask else None
        PP = ctypes.c_void_p * n
        din = PP(*[d[i].ctypes.data for i in range(n)])
        mout = PP(*[masked[i].ctypes.data for i in range(n)])
        kout = PP(*[mask[i].ctypes.data for i in range(n)]) if want_mask else None
        self._check(self._lib.rtuf_filter_batch(self._h, n, din, mout, kout))
        return masked, mask

    def filter_batch_u16(self, depth_mm, want_mask=True):
        """16UC1: depth_mm [n,H,W] uint16 millimetres -> (masked uint16 [n,H,W], mask)."""
        d = np.ascontiguousarray(depth_mm, np.uint16).reshape(-1, self.height, self.width)
        n = d.shape[0]
        masked = np.empty_like(d)
        mask = np.empty(d.shape, np.uint8) if want_mask else None
        PP = ctypes.c_void_p * n
        din = PP(*[d[i].ctypes.data for i in range(n)])
        mout = PP(*[masked[i].ctypes.data for i in range(n)])
        kout = PP(*[mask[i].ctypes.data for i in range(n)]) if want_mask else None
        self._check(self._lib.rtuf_filter_batch_u16(self._h, n, din, mout, kout))
        return masked, mask

    # link labels (include/rtuf.h, LINK LABELS)
    def set_link_labels(self, model, labels):
        """Labels of model `model`'s links (one uint16 per link, in rtuf_add_link order)."""
        a = np.ascontiguousarray(labels, np.uint16).reshape(-1)
        self._check(self._lib.rtuf_set_link_labels(self._h, model, _ptr(a), len(a)))

    def filter_batch_labels(self, depth, want_mask=True):
        """Like filter_batch (float32 depth) or filter_batch_u16 (uint16 depth), plus the link label plane:
        -> (masked, mask or None, labels [n,H,W] uint16)."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        masked = np.empty_like(d)
        mask = np.empty(d.shape, np.uint8) if want_mask else None
        labels = np.empty(d.shape, np.uint16)
        PP = ctypes.c_void_p * n
        din = PP(*[d[i].ctypes.data for i in range(n)])
        mout = PP(*[masked[i].ctypes.data for i in range(n)])
        kout = PP(*[mask[i].ctypes.data for i in range(n)]) if want_mask else None
        lout = PP(*[labels[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_filter_batch_u16_labels if u16 else self._lib.rtuf_filter_batch_labels
        self._check(fn(self._h, n, din, mout, kout, lout))
        return masked, mask, labels

    def filter_batch_device_labels(self, n, d_depth, d_masked, d_mask, d_labels, u16=False):
        """Device pointers (ints; d_mask may be None): enqueue only; call sync()."""
        fn = self._lib.rtuf_filter_batch_device_u16_labels if u16 else self._lib.rtuf_filter_batch_device_labels
        self._check(fn(self._h, n, ctypes.c_void_p(d_depth), ctypes.c_void_p(d_masked), ctypes.c_void_p(d_mask) if d_mask else None,
                       ctypes.c_void_p(d_labels) if d_labels else None))

    # per-link depth thresholds (include/rtuf.h, PER-LINK DEPTH THRESHOLDS)
    def set_link_thresholds(self, model, thresholds):
        """Depth thresholds (metres, any float) of model `model`'s links, one per link in rtuf_add_link order."""
        a = np.ascontiguousarray(thresholds, np.float32).reshape(-1)
        self._check(self._lib.rtuf_set_link_thresholds(self._h, model, _ptr(a), len(a)))

    def clear_link_thresholds(self, model):
        """Model `model`'s links follow params.depth_distance_threshold again."""
        self._check(self._lib.rtuf_clear_link_thresholds(self._h, model))

    # link padding (include/rtuf.h, LINK PADDING)
    def set_link_padding(self, model, padding_m):
        """Margins in metres (finite, >= 0) around the silhouettes of model `model`'s links, one per link in rtuf_add_link order.
        The streams need their intrinsics (set_cloud_intrinsics): a margin is projected with max(fx, fy)."""
        a = np.ascontiguousarray(padding_m, np.float32).reshape(-1)
        self._check(self._lib.rtuf_set_link_padding(self._h, model, _ptr(a), len(a)))

    def clear_link_padding(self, model):
        """Model `model`'s links have no padding again."""
        self._check(self._lib.rtuf_clear_link_padding(self._h, model))

    # scene planes (include/rtuf.h, SCENE PLANES)
    def set_scene_planes(self, first_stream, planes):
        """The scene planes of streams first_stream ..: [n,H,W] float32 metres (any value; +inf and NaN mean unknown)."""
        a = np.ascontiguousarray(planes, np.float32).reshape(-1, self.height, self.width)
        PP = ctypes.c_void_p * max(len(a), 1)
        pin = PP(*[a[i].ctypes.data for i in range(len(a))])
        self._check(self._lib.rtuf_set_scene_planes(self._h, first_stream, len(a), pin))

    def set_scene_planes_device(self, first_stream, n, d_planes):
        """Device pointer (int): [n,H,W] float32, packed."""
        self._check(self._lib.rtuf_set_scene_planes_device(self._h, first_stream, n, ctypes.c_void_p(d_planes) if d_planes else None))

    def get_scene_planes(self, first_stream=0, n=None):
        """-> [n,H,W] float32: the scene planes of streams first_stream .. (all of them by default)."""
        n = self.max_streams - first_stream if n is None else n
        out = np.empty((max(n, 0), self.height, self.width), np.float32)
        PP = ctypes.c_void_p * max(n, 1)
        pout = PP(*[out[i].ctypes.data for i in range(max(n, 0))])
        self._check(self._lib.rtuf_get_scene_planes(self._h, first_stream, n, pout))
        return out

    def get_scene_planes_device(self, first_stream, n, d_out):
        self._check(self._lib.rtuf_get_scene_planes_device(self._h, first_stream, n, ctypes.c_void_p(d_out) if d_out else None))

    def set_scene_margins(self, first_stream, abs_rel, n=None):
        """abs_rel: [n,2] (or one row of 2) floats {abs_m >= 0, 0 <= rel < 1}: sets the margins and enables scene filtering for
        streams first_stream ..; abs_rel=None disables it for n streams and keeps their planes."""
        if abs_rel is None:
            self._check(self._lib.rtuf_set_scene_margins(self._h, first_stream, self.max_streams - first_stream if n is None else n, None))
            return
        a = np.ascontiguousarray(abs_rel, np.float32).reshape(-1, 2)
        self._check(self._lib.rtuf_set_scene_margins(self._h, first_stream, len(a), _ptr(a)))

    def clear_scene(self, first_stream=0, n=None):
        """Streams first_stream .. (all by default): filtering off, planes back to +inf, margins back to 0."""
        self._check(self._lib.rtuf_clear_scene(self._h, first_stream, self.max_streams - first_stream if n is None else n))

    def learn_scene_batch(self, depth):
        """Lowers the scene planes of streams 0 .. n-1 to the readings of every pixel the robot filter keeps: depth [n,H,W]
        float32 metres (or uint16 millimetres: the 16UC1 form).  Synchronous."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        PP = ctypes.c_void_p * max(n, 1)
        din = PP(*[d[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_learn_scene_batch_u16 if u16 else self._lib.rtuf_learn_scene_batch
        self._check(fn(self._h, n, din))

    def learn_scene_batch_u16(self, depth_mm):
        self.learn_scene_batch(np.ascontiguousarray(depth_mm, np.uint16))

    def learn_scene_batch_device(self, n, d_depth, u16=False):
        """Device pointer (int): d_depth [n,H,W] float32 (uint16 with u16).  Synchronous."""
        fn = self._lib.rtuf_learn_scene_batch_device_u16 if u16 else self._lib.rtuf_learn_scene_batch_device
        self._check(fn(self._h, n, ctypes.c_void_p(d_depth) if d_depth else None))

    # virtual depth (include/rtuf.h, VIRTUAL DEPTH)
    def render_batch(self, n, empty_value=0.0, labels=False, u16=False):
        """The robot's own depth image of streams 0 .. n-1, no sensor plane involved: -> (virtual [n,H,W] float32 metres, or
        uint16 millimetres with u16; labels [n,H,W] uint16 or None).  Pixels no link won hold empty_value."""
        virt = np.empty((n, self.height, self.width), np.uint16 if u16 else np.float32)
        lab = np.empty(virt.shape, np.uint16) if labels else None
        PP = ctypes.c_void_p * max(n, 1)
        vout = PP(*[virt[i].ctypes.data for i in range(n)])
        lout = PP(*[lab[i].ctypes.data for i in range(n)]) if labels else None
        fn = self._lib.rtuf_render_batch_u16 if u16 else self._lib.rtuf_render_batch
        self._check(fn(self._h, n, vout, lout, empty_value))
        return virt, lab

    def render_batch_device(self, n, d_virtual, d_labels=None, empty_value=0.0):
        """Device pointers (ints; d_labels may be None): enqueue only; call sync()."""
        self._check(self._lib.rtuf_render_batch_device(self._h, n, ctypes.c_void_p(d_virtual) if d_virtual else None,
                                                       ctypes.c_void_p(d_labels) if d_labels else None, empty_value))

    def render_batch_device_u16(self, n, d_virtual_mm, d_labels=None, empty_value=0.0):
        self._check(self._lib.rtuf_render_batch_device_u16(self._h, n, ctypes.c_void_p(d_virtual_mm) if d_virtual_mm else None,
                                                           ctypes.c_void_p(d_labels) if d_labels else None, empty_value))

    # link residual tables (include/rtuf.h, LINK RESIDUAL TABLES)
    def link_residuals_batch(self, depth, n_labels):
        """Per stream and label, how the sensor planes compare with the model: depth [n,H,W] float32 metres (or uint16
        millimetres: the 16UC1 form) -> table [n, n_labels] of LINK_RESIDUALS_DTYPE.  Synchronous."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        table = np.empty((n, max(int(n_labels), 0)), LINK_RESIDUALS_DTYPE)
        PP = ctypes.c_void_p * max(n, 1)
        din = PP(*[d[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_link_residuals_batch_u16 if u16 else self._lib.rtuf_link_residuals_batch
        self._check(fn(self._h, n, din, ctypes.c_void_p(table.ctypes.data), int(n_labels)))
        return table

    def link_residuals_batch_u16(self, depth_mm, n_labels):
        return self.link_residuals_batch(np.ascontiguousarray(depth_mm, np.uint16), n_labels)

    def link_residuals_batch_device(self, n, d_depth, d_table, n_labels):
        """Device pointers (ints): d_depth [n,H,W] float32, d_table [n, n_labels] rows of 64 bytes; enqueue only; call sync()."""
        self._check(self._lib.rtuf_link_residuals_batch_device(self._h, n, ctypes.c_void_p(d_depth) if d_depth else None,
                                                               ctypes.c_void_p(d_table) if d_table else None, int(n_labels)))

    def link_residuals_batch_device_u16(self, n, d_depth_mm, d_table, n_labels):
        self._check(self._lib.rtuf_link_residuals_batch_device_u16(self._h, n, ctypes.c_void_p(d_depth_mm) if d_depth_mm else None,
                                                                   ctypes.c_void_p(d_table) if d_table else None, int(n_labels)))

    # filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS)
    def set_cloud_intrinsics(self, first_stream, fx_fy_cx_cy):
        """fx, fy, cx, cy of streams first_stream ..: [n,4] (or one row of 4) doubles."""
        a = np.ascontiguousarray(fx_fy_cx_cy, np.float64).reshape(-1, 4)
        self._check(self._lib.rtuf_set_cloud_intrinsics(self._h, first_stream, len(a), _ptr(a)))

    def cloud_batch(self, depth):
        """The kept pixels as XYZ, organized: depth [n,H,W] float32 metres (or uint16 millimetres: the 16UC1 form) ->
        points [n,H,W,3] float32, NaN where the pixel is masked or holds no reading.  Synchronous."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        points = np.empty((n, self.height, self.width, 3), np.float32)
        PP = ctypes.c_void_p * max(n, 1)
        din = PP(*[d[i].ctypes.data for i in range(n)])
        pout = PP(*[points[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_cloud_batch_u16 if u16 else self._lib.rtuf_cloud_batch
        self._check(fn(self._h, n, din, pout))
        return points

    def cloud_batch_u16(self, depth_mm):
        return self.cloud_batch(np.ascontiguousarray(depth_mm, np.uint16))

    def cloud_compact_batch(self, depth, capacity, want_index=True):
        """The kept pixels as XYZ, compacted in row-major order: -> (points [n,capacity,3] float32, index [n,capacity] uint32
        (v * W + u) or None, counts [n] uint32).  counts is the full number of kept pixels; entries [min(count, capacity):] of a
        stream are unspecified.  Synchronous."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        cap = max(int(capacity), 0)
        points = np.empty((n, cap, 3), np.float32)
        index = np.empty((n, cap), np.uint32) if want_index else None
        counts = np.zeros(n, np.uint32)
        PP = ctypes.c_void_p * max(n, 1)
        din = PP(*[d[i].ctypes.data for i in range(n)])
        pout = PP(*[points[i].ctypes.data if cap else points.ctypes.data for i in range(n)])
        iout = PP(*[index[i].ctypes.data if cap else index.ctypes.data for i in range(n)]) if want_index else None
        fn = self._lib.rtuf_cloud_compact_batch_u16 if u16 else self._lib.rtuf_cloud_compact_batch
        self._check(fn(self._h, n, din, pout, iout, _ptr(counts), int(capacity)))
        return points, index, counts

    def cloud_compact_batch_u16(self, depth_mm, capacity, want_index=True):
        return self.cloud_compact_batch(np.ascontiguousarray(depth_mm, np.uint16), capacity, want_index)

    def cloud_batch_device(self, n, d_depth, d_points, u16=False):
        """Device pointers (ints): d_depth [n,H,W] float32 (uint16 with u16), d_points [n,H,W,3] float32; enqueue only; call sync()."""
        fn = self._lib.rtuf_cloud_batch_device_u16 if u16 else self._lib.rtuf_cloud_batch_device
        self._check(fn(self._h, n, ctypes.c_void_p(d_depth) if d_depth else None, ctypes.c_void_p(d_points) if d_points else None))

    def cloud_batch_device_u16(self, n, d_depth_mm, d_points):
        self.cloud_batch_device(n, d_depth_mm, d_points, u16=True)

    def cloud_compact_batch_device(self, n, d_depth, d_points, d_index, d_counts, capacity, u16=False):
        """Device pointers (ints; d_index may be None): d_points [n,capacity,3] float32, d_index [n,capacity] uint32, d_counts [n]
        uint32; enqueue only; call sync()."""
        fn = self._lib.rtuf_cloud_compact_batch_device_u16 if u16 else self._lib.rtuf_cloud_compact_batch_device
        self._check(fn(self._h, n, ctypes.c_void_p(d_depth) if d_depth else None, ctypes.c_void_p(d_points) if d_points else None,
                       ctypes.c_void_p(d_index) if d_index else None, ctypes.c_void_p(d_counts) if d_counts else None, int(capacity)))

    def cloud_compact_batch_device_u16(self, n, d_depth_mm, d_points, d_index, d_counts, capacity):
        self.cloud_compact_batch_device(n, d_depth_mm, d_points, d_index, d_counts, capacity, u16=True)

    # point list batches (include/rtuf.h, POINT LIST BATCHES)
    def set_point_transforms(self, first_stream, optical_from_points, n_streams=None):
        """optical_from_points: [n,16] (or one row of 16) doubles, column-major, for streams first_stream ..; None takes the
        transforms of n_streams streams (default: one) away again."""
        if optical_from_points is None:
            self._check(self._lib.rtuf_set_point_transforms(self._h, first_stream, 1 if n_streams is None else int(n_streams), None))
            return
        a = np.ascontiguousarray(optical_from_points, np.float64).reshape(-1, 16)
        self._check(self._lib.rtuf_set_point_transforms(self._h, first_stream, len(a), _ptr(a)))

    def points_batch(self, points, radius_px=0, want_pixel=True):
        """Point lists against the robot's virtual depth: points is a sequence of [count_s,3] float32 arrays, one per stream, in the
        stream's optical frame -> (verdicts: list of [count_s] uint8 -- 0 kept, 1 filtered, 2 outside --, pixels: list of [count_s]
        uint32 (v * W + u, 0xFFFFFFFF where the verdict is 2) or None, summary [n,4] uint32: kept, filtered, outside, count).
        Synchronous."""
        pts = [np.ascontiguousarray(p, np.float32).reshape(-1, 3) for p in points]
        n = len(pts)
        counts = np.array([len(p) for p in pts], np.uint32)
        verdict = [np.empty(len(p), np.uint8) for p in pts]
        pixel = [np.empty(len(p), np.uint32) for p in pts] if want_pixel else None
        summary = np.zeros((n, 4), np.uint32)
        PP = ctypes.c_void_p * max(n, 1)
        # (an empty list still hands a valid pointer over: nothing is read or written through it)
        at = lambda a: a.ctypes.data if a.size else summary.ctypes.data
        pin = PP(*[at(p) for p in pts])
        vout = PP(*[at(v) for v in verdict])
        xout = PP(*[at(x) for x in pixel]) if want_pixel else None
        self._check(self._lib.rtuf_points_batch(self._h, n, pin, _ptr(counts), int(radius_px), vout, xout, _ptr(summary)))
        return verdict, pixel, summary

    def points_batch_device(self, n, d_points, d_counts, capacity, radius_px, d_verdict, d_pixel=None, d_summary=None):
        """Device pointers (ints; d_pixel and d_summary may be None): d_points [n,capacity,3] float32, d_counts [n] uint32,
        d_verdict [n,capacity] uint8, d_pixel [n,capacity] uint32, d_summary [n,4] uint32; enqueue only; call sync()."""
        q = lambda v: ctypes.c_void_p(v) if v else None
        self._check(self._lib.rtuf_points_batch_device(self._h, n, q(d_points), q(d_counts), int(capacity), int(radius_px), q(d_verdict),
                                                       q(d_pixel), q(d_summary)))

    # voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS)
    def set_voxel_grid(self, origin, voxel_size, dims, with_counts=True):
        """One world grid for the kept points of all streams: origin [3] and voxel_size in metres, dims (nx, ny, nz).  Allocates
        and zeroes it (replacing the grid that is there); dims None frees it."""
        if dims is None:
            self._check(self._lib.rtuf_set_voxel_grid(self._h, None, 0.0, None, 0))
            self._voxel_dims = None
            return
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        d = np.ascontiguousarray(dims, np.int32).reshape(3)
        self._check(self._lib.rtuf_set_voxel_grid(self._h, _ptr(o), float(voxel_size), _ptr(d), 1 if with_counts else 0))
        self._voxel_dims = (tuple(int(q) for q in d), bool(with_counts))

    def set_voxel_transforms(self, first_stream, world_from_optical, n_streams=None):
        """world_from_optical: [n,16] (or one row of 16) doubles, column-major, for streams first_stream ..; None takes the
        transforms of n_streams streams (default: one) away again."""
        if world_from_optical is None:
            self._check(self._lib.rtuf_set_voxel_transforms(self._h, first_stream, 1 if n_streams is None else int(n_streams), None))
            return
        a = np.ascontiguousarray(world_from_optical, np.float64).reshape(-1, 16)
        self._check(self._lib.rtuf_set_voxel_transforms(self._h, first_stream, len(a), _ptr(a)))

    def voxel_clear(self):
        self._check(self._lib.rtuf_voxel_clear(self._h))

    def voxel_insert_batch(self, depth):
        """Inserts the kept pixels of depth [n,H,W] float32 metres (or uint16 millimetres: the 16UC1 form) into the grid ->
        summary [n,4] uint32: inserted, outside the grid, not kept, total.  Synchronous."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        summary = np.zeros((n, 4), np.uint32)
        PP = ctypes.c_void_p * max(n, 1)
        din = PP(*[d[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_voxel_insert_batch_u16 if u16 else self._lib.rtuf_voxel_insert_batch
        self._check(fn(self._h, n, din, _ptr(summary)))
        return summary

    def voxel_insert_batch_u16(self, depth_mm):
        return self.voxel_insert_batch(np.ascontiguousarray(depth_mm, np.uint16))

    def voxel_insert_batch_device(self, n, d_depth, d_summary=None, u16=False):
        """Device pointers (ints; d_summary may be None): d_depth [n,H,W] float32 (uint16 with u16), d_summary [n,4] uint32.
        Synchronous."""
        q = lambda v: ctypes.c_void_p(v) if v else None
        fn = self._lib.rtuf_voxel_insert_batch_device_u16 if u16 else self._lib.rtuf_voxel_insert_batch_device
        self._check(fn(self._h, n, q(d_depth), q(d_summary)))

    def voxel_insert_batch_device_u16(self, n, d_depth_mm, d_summary=None):
        self.voxel_insert_batch_device(n, d_depth_mm, d_summary, u16=True)

    def voxel_insert_points_device(self, n, d_points, d_counts, capacity, d_verdict=None, d_summary=None):
        """Device pointers (ints; d_verdict and d_summary may be None): d_points [n,capacity,3] float32, d_counts [n] uint32,
        d_verdict [n,capacity] uint8 (0 = taken), d_summary [n,4] uint32.  Synchronous."""
        q = lambda v: ctypes.c_void_p(v) if v else None
        self._check(self._lib.rtuf_voxel_insert_points_device(self._h, n, q(d_points), q(d_counts), int(capacity), q(d_verdict), q(d_summary)))

    def voxel_grid_device(self, want_counts=True):
        """-> (d_bits, d_counts or None, n_voxels): device pointers (ints) of the grid, valid until it is replaced or freed."""
        b, k, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._lib.rtuf_voxel_grid_device(self._h, ctypes.byref(b), ctypes.byref(k) if want_counts else None, ctypes.byref(n)))
        return b.value, (k.value if want_counts else None), int(n.value)

    def voxel_grid(self, want_counts=None):
        """-> (bits [ceil(n_voxels / 32)] uint32, counts [nz,ny,nx] uint32 or None): host copies of the grid.  want_counts
        defaults to whether the grid was made with counts."""
        _, _, n = self.voxel_grid_device(want_counts=False)
        dims, has = getattr(self, "_voxel_dims", None) or ((n, 1, 1), False)
        want = has if want_counts is None else bool(want_counts)
        bits = np.empty((n + 31) // 32, np.uint32)
        counts = np.empty(n, np.uint32) if want else None
        self._check(self._lib.rtuf_get_voxel_grid(self._h, _ptr(bits), _ptr(counts) if want else None))
        return bits, (counts.reshape(dims[2], dims[1], dims[0]) if want else None)

    # voxel free space (include/rtuf.h, VOXEL FREE SPACE)
    def voxel_carve_batch_device(self, n, d_depth, margin, radius_px=0, d_summary=None, u16=False):
        """Device pointers (ints; d_summary may be None): d_depth [n,H,W] float32 (uint16 with u16), d_summary [n,4] uint32 (free,
        not free, not seen, n_voxels).  Marks the voxels whose centre some stream sees in front of its reading by more than
        `margin` metres, at window radius radius_px (0 .. 4).  Synchronous."""
        q = lambda v: ctypes.c_void_p(v) if v else None
        fn = self._lib.rtuf_voxel_carve_batch_device_u16 if u16 else self._lib.rtuf_voxel_carve_batch_device
        self._check(fn(self._h, n, q(d_depth), float(margin), int(radius_px), q(d_summary)))

    def voxel_carve_batch(self, depth, margin, radius_px=0):
        """Carves from host planes depth [n,H,W] float32 metres (or uint16 millimetres: the 16UC1 form) -> summary [n,4] uint32:
        free, not free, not seen, n_voxels.  Synchronous."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        summary = np.zeros((n, 4), np.uint32)
        PP = ctypes.c_void_p * max(n, 1)
        din = PP(*[d[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_voxel_carve_batch_u16 if u16 else self._lib.rtuf_voxel_carve_batch
        self._check(fn(self._h, n, din, float(margin), int(radius_px), _ptr(summary)))
        return summary

    def voxel_free_device(self):
        """-> (d_free_bits, n_voxels): the device pointer (int) of the free words, valid until the grid is replaced or freed."""
        b, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._lib.rtuf_voxel_free_device(self._h, ctypes.byref(b), ctypes.byref(n)))
        return b.value, int(n.value)

    def voxel_free(self):
        """-> [ceil(n_voxels / 32)] uint32: a host copy of the free words (bit i & 31 of word i >> 5)."""
        _, n = self.voxel_free_device()
        free = np.empty((n + 31) // 32, np.uint32)
        self._check(self._lib.rtuf_get_voxel_free(self._h, _ptr(free)))
        return free

    # link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES)
    def set_link_spheres(self, model, link, xyzr):
        """The sphere list of model `model`: link [n] (index within the model) and xyzr [n,4] (centre in the link's frame -- a draw's
        pre_op applied to its vertices first -- and radius).  Replaces the model's list; empty arrays clear it."""
        li = np.ascontiguousarray(link, np.int32).reshape(-1)
        q = np.ascontiguousarray(xyzr, np.float32).reshape(-1, 4)
        if len(li) != len(q):
            raise ValueError("link and xyzr differ in length")
        self._check(self._lib.rtuf_set_link_spheres(self._h, model, _ptr(li) if len(li) else None, _ptr(q) if len(q) else None, len(li)))

    def link_clearance_batch(self, depth, n_labels, max_distance):
        """Per stream and label, the nearest kept point to the label's spheres: depth [n,H,W] float32 metres (or uint16
        millimetres: the 16UC1 form) -> table [n, n_labels] of LINK_CLEARANCE_DTYPE.  Synchronous."""
        u16 = np.asarray(depth).dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32).reshape(-1, self.height, self.width)
        n = d.shape[0]
        table = np.empty((n, max(int(n_labels), 0)), LINK_CLEARANCE_DTYPE)
        PP = ctypes.c_void_p * max(n, 1)
        din = PP(*[d[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_link_clearance_batch_u16 if u16 else self._lib.rtuf_link_clearance_batch
        self._check(fn(self._h, n, din, ctypes.c_void_p(table.ctypes.data), int(n_labels), float(max_distance)))
        return table

    def link_clearance_batch_u16(self, depth_mm, n_labels, max_distance):
        return self.link_clearance_batch(np.ascontiguousarray(depth_mm, np.uint16), n_labels, max_distance)

    def link_clearance_batch_device(self, n, d_depth, d_table, n_labels, max_distance, u16=False):
        """Device pointers (ints): d_depth [n,H,W] float32 (uint16 with u16), d_table [n, n_labels] rows of 16 bytes; enqueue only;
        call sync()."""
        fn = self._lib.rtuf_link_clearance_batch_device_u16 if u16 else self._lib.rtuf_link_clearance_batch_device
        self._check(fn(self._h, n, ctypes.c_void_p(d_depth) if d_depth else None, ctypes.c_void_p(d_table) if d_table else None, int(n_labels),
                       float(max_distance)))

    def link_clearance_batch_device_u16(self, n, d_depth_mm, d_table, n_labels, max_distance):
        self.link_clearance_batch_device(n, d_depth_mm, d_table, n_labels, max_distance, u16=True)

    # asynchronous host planes
    def host_alloc(self, shape, dtype):
        """Pinned host array (rtuf_host_alloc) for filter_batch_async; release with host_free()."""
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dt.itemsize
        p = ctypes.c_void_p()
        self._check(self._lib.rtuf_host_alloc(self._h, nbytes, ctypes.byref(p)))
        buf = (ctypes.c_char * nbytes).from_address(p.value)
        a = np.frombuffer(buf, dtype=dt).reshape(shape)
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a):
        p = self._pinned.pop(a.ctypes.data)
        self._check(self._lib.rtuf_host_free(self._h, ctypes.c_void_p(p)))

    def filter_batch_async(self, depth, masked, mask=None):
        """Enqueue only: depth / masked [n,H,W] float32 (or uint16 for 16UC1) host arrays, mask [n,H,W] u8 or
        None; the arrays must stay alive and untouched until wait_oldest() / sync() retires the batch."""
        n = depth.shape[0]
        u16 = depth.dtype == np.uint16
        assert depth.flags.c_contiguous and masked.flags.c_contiguous and masked.dtype == depth.dtype
        assert depth.dtype in (np.float32, np.uint16) and depth.shape == (n, self.height, self.width) == masked.shape
        assert mask is None or (mask.flags.c_contiguous and mask.dtype == np.uint8 and mask.shape == depth.shape)
        PP = ctypes.c_void_p * n
        din = PP(*[depth[i].ctypes.data for i in range(n)])
        mout = PP(*[masked[i].ctypes.data for i in range(n)])
        kout = PP(*[mask[i].ctypes.data for i in range(n)]) if mask is not None else None
        fn = self._lib.rtuf_filter_batch_u16_async if u16 else self._lib.rtuf_filter_batch_async
        self._check(fn(self._h, n, din, mout, kout))

    # mask-only output, one bit per pixel
    def mask_bits_words(self):
        return int(self._lib.rtuf_mask_bits_words(self.width, self.height))

    def filter_batch_bits_async(self, depth, bits):
        """Enqueue only: depth [n,H,W] float32 or uint16 host array, bits [n, mask_bits_words()] uint32 host array
        (pinned for overlap); retire with wait_oldest() / sync()."""
        n = depth.shape[0]
        u16 = depth.dtype == np.uint16
        assert depth.flags.c_contiguous and depth.dtype in (np.float32, np.uint16) and depth.shape == (n, self.height, self.width)
        assert bits.flags.c_contiguous and bits.dtype == np.uint32 and bits.shape == (n, self.mask_bits_words())
        PP = ctypes.c_void_p * n
        din = PP(*[depth[i].ctypes.data for i in range(n)])
        bout = PP(*[bits[i].ctypes.data for i in range(n)])
        fn = self._lib.rtuf_filter_batch_bits_u16_async if u16 else self._lib.rtuf_filter_batch_bits_async
        self._check(fn(self._h, n, din, bout))

    def filter_batch_device_bits(self, n, d_depth, d_bits, u16=False):
        fn = self._lib.rtuf_filter_batch_device_bits_u16 if u16 else self._lib.rtuf_filter_batch_device_bits
        self._check(fn(self._h, n, ctypes.c_void_p(d_depth), ctypes.c_void_p(d_bits)))

    def wait_oldest(self):
        self._check(self._lib.rtuf_wait_oldest(self._h))

    def filter_batch_device_u16(self, n, d_depth, d_masked, d_mask=None):
        self._check(self._lib.rtuf_filter_batch_device_u16(self._h, n, ctypes.c_void_p(d_depth), ctypes.c_void_p(d_masked),
                                                           ctypes.c_void_p(d_mask) if d_mask else None))

    def filter_batch_device(self, n, d_depth, d_masked, d_mask=None):
        """Device pointers (ints): enqueue only; call sync()."""
        self._check(self._lib.rtuf_filter_batch_device(self._h, n, ctypes.c_void_p(d_depth), ctypes.c_void_p(d_masked),
                                                       ctypes.c_void_p(d_mask) if d_mask else None))

    def filter(self, buffer, projection):
        """RealtimeURDFFilter::filter(buffer, glTf, w, h) + getMaskedDepth()/mask_."""
        b = np.ascontiguousarray(buffer, np.float32).reshape(self.height, self.width)
        P = np.ascontiguousarray(projection, np.float64).reshape(16)
        self._check(self._lib.rtuf_filter(self._h, _ptr(b), _ptr(P), self.width, self.height))
        n = self.width * self.height
        md = np.ctypeslib.as_array(self._lib.rtuf_get_masked_depth(self._h), shape=(n,)).reshape(self.height, self.width).copy()
        mk = np.ctypeslib.as_array(self._lib.rtuf_get_mask(self._h), shape=(n,)).reshape(self.height, self.width).copy()
        return md, mk

    def sync(self):
        self._check(self._lib.rtuf_sync(self._h))

    def stream_handle(self):
        """hipStream_t of a context with ONE raster lane and one pipeline; None for every other context (never hand that
        None to HIP as a stream: use order_stream_after_batches)."""
        return self._lib.rtuf_stream(self._h)

    def order_stream_after_batches(self, hip_stream=None):
        """Makes `hip_stream` (an int / c_void_p hipStream_t; None = the legacy default stream) wait on the device for every
        batch enqueued so far, whatever the number of lanes and pipelines."""
        self._check(self._lib.rtuf_order_stream_after_batches(self._h, ctypes.c_void_p(hip_stream) if hip_stream else None))

    def batch_status_device(self):
        """Device address (int) of the status word of the batch the last filter call enqueued: 0 there, read on a stream
        ordered behind the batch (order_stream_after_batches), means its planes are final; STATUS_* bits say why not."""
        p = ctypes.c_void_p()
        self._check(self._lib.rtuf_batch_status_device(self._h, ctypes.byref(p)))
        return p.value

    def enable_timing(self, on=True):
        # True/1: every stage; 2: only around the tile (and compare) kernel; False/0: off
        self._check(self._lib.rtuf_enable_timing(self._h, int(on)))

    def stats(self):
        s = Stats()
        self._check(self._lib.rtuf_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def read_zsurface(self, n):
        out = np.empty((n, self.height, self.width), np.float32)
        self._check(self._lib.rtuf_debug_read_zsurface(self._h, n, _ptr(out)))
        return out


def expand_mask_bits(depth, bits, replace_value, want_masked=True, want_mask=True):
    """Host helper rtuf_expand_mask_bits for one frame: depth [H,W] float32 or uint16, bits [mask_bits_words] uint32
    -> (masked like depth or None, mask u8 [H,W] or None)."""
    d = np.ascontiguousarray(depth)
    assert d.dtype in (np.float32, np.uint16) and d.ndim == 2
    H, W = d.shape
    b = np.ascontiguousarray(bits, np.uint32)
    masked = np.empty_like(d) if want_masked else None
    mask = np.empty((H, W), np.uint8) if want_mask else None
    rc = load_library().rtuf_expand_mask_bits(_ptr(d), 1 if d.dtype == np.uint16 else 0, _ptr(b), W, H, float(replace_value), _ptr(masked), _ptr(mask))
    if rc != RTUF_OK:
        raise RtufError(rc, "rtuf_expand_mask_bits failed")
    return masked, mask
