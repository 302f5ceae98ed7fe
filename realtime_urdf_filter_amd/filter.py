"""Host-side mirror of the reference's operator interface for the hot path, above the C ABI.

Same names, argument meaning and error behaviour as
  realtime_urdf_filter::RealtimeURDFFilter  include/realtime_urdf_filter/urdf_filter.h:51-143
  realtime_urdf_filter::URDFRenderer        include/realtime_urdf_filter/urdf_renderer.h:45-73
  realtime_urdf_filter::Renderable*         include/realtime_urdf_filter/renderable.h:54-143
with the ROS types replaced by plain Python ones: the private NodeHandle's parameters are a
`FilterParameters` object (+ a dict acting as the parameter server for robot descriptions),
tf::TransformListener is any object with `lookup_transform(target, source, stamp)`, and
sensor_msgs/CameraInfo is a `CameraInfo` tuple.  All per-pixel work happens in librtuf.so on
the GPU; this module only prepares matrices in double precision exactly like the reference's
host code does (tf::Transform algebra) and hands them to the C ABI.

The C++ facade (include/realtime_urdf_filter_amd/urdf_filter.hpp) exposes the same surface to
C++ hosts; both call the identical C entry points.
"""
import logging
from collections import namedtuple

import numpy as np

from . import _capi, geometry, urdf
from .urdf import Transform

log = logging.getLogger("realtime_urdf_filter")

CameraInfo = namedtuple("CameraInfo", "width height P")     # P: 12 doubles, row-major 3x4


class Renderable:
    """renderable.h:54-73."""

    def __init__(self):
        self.name = ""
        self.urdf_link = ""                   # the URDF link's own name (`name` carries the tf prefix): its label's key
        self.link_offset = Transform()
        self.link_to_fixed = Transform()
        self.draws = []

    def setLinkName(self, n):
        self.name = n

    def gl_matrix(self):
        """applyTransform (src/renderable.cpp:59-68): (link_to_fixed * link_offset).getOpenGLMatrix()."""
        return (self.link_to_fixed * self.link_offset).opengl_matrix()


class RenderableBox(Renderable):
    def __init__(self, dimx, dimy, dimz):
        super().__init__()
        self.dimx, self.dimy, self.dimz = np.float32(dimx), np.float32(dimy), np.float32(dimz)
        self.draws = geometry.box_draws(self.dimx, self.dimy, self.dimz)


class RenderableSphere(Renderable):
    def __init__(self, radius):
        super().__init__()
        self.radius = np.float32(radius)
        self.draws = geometry.sphere_draws(self.radius)


class RenderableCylinder(Renderable):
    def __init__(self, radius, length):
        super().__init__()
        self.radius, self.length = np.float32(radius), np.float32(length)
        self.draws = geometry.cylinder_draws(self.radius, self.length)


class RenderableMesh(Renderable):
    """src/renderable.cpp:306-322: a mesh that fails to load becomes a renderable with zero
    sub-meshes (draws nothing) and an error is logged (quirk Q15)."""

    def __init__(self, meshname, sx, sy, sz, mesh_loader=None):
        super().__init__()
        self.meshname = meshname
        try:
            if mesh_loader is None:
                # the reference resolves every URI through resource_retriever: package:// against ROS_PACKAGE_PATH
                mesh_loader = geometry.PackageResolver()
            v, t = mesh_loader(meshname)
            self.draws = geometry.mesh_draws(v, t, sx, sy, sz)
        except Exception as e:                      # noqa: BLE001 - mirror ROS_ERROR + continue
            log.error("Could not load resource [%s]: %s", meshname, e)
            self.draws = []


class URDFRenderer:
    """urdf_renderer.h:45-73 / src/urdf_renderer.cpp."""

    def __init__(self, model_description, tf_prefix, cam_frame, fixed_frame, tf, geometry_type="visual",
                 scale=1.0, ignore=(), mesh_loader=None):
        self.model_description_ = model_description
        self.tf_prefix_ = tf_prefix
        self.geometry_type = geometry_type
        self.scale = float(scale)
        self.ignore = set(ignore)
        self.camera_frame_ = cam_frame
        self.fixed_frame_ = fixed_frame
        self.tf_ = tf
        self.mesh_loader = mesh_loader
        self.renderables_ = []
        self.link_names_ = []                     # every link of the URDF, ignored ones included
        self.link_thresholds_ = {}                # URDF link name -> depth threshold of its own (RealtimeURDFFilter.loadModels)
        self.link_padding_ = {}                   # URDF link name -> padding in metres (RealtimeURDFFilter.loadModels)
        self.initURDFModel()

    def initURDFModel(self):
        try:
            model = urdf.Model.from_string(self.model_description_)
        except Exception as e:                      # noqa: BLE001 - ROS_FATAL + return
            log.critical("URDF failed Model parse: %s", e)
            return
        self.loadURDFModel(model)

    def loadURDFModel(self, model):
        self.link_names_ = [link.name for link in model.get_links()]
        for link in model.get_links():
            self.process_link(link)

    def process_link(self, link):
        """src/urdf_renderer.cpp:100-169."""
        if link.name in self.ignore:
            return
        if self.geometry_type in ("", "visual"):
            items = link.visual_array
        elif self.geometry_type == "collision":
            items = link.collision_array
        else:
            log.critical("invalid geometry type: %s", self.geometry_type)
            items = []
        s = self.scale
        for it in items:
            g = it.geometry
            if g.kind == "box":
                r = RenderableBox(s * g.size[0], s * g.size[1], s * g.size[2])
            elif g.kind == "cylinder":
                r = RenderableCylinder(s * g.radius, s * g.length)
            elif g.kind == "sphere":
                r = RenderableSphere(s * g.radius)
            elif g.kind == "mesh":
                r = RenderableMesh(g.filename, s * g.scale[0], s * g.scale[1], s * g.scale[2], self.mesh_loader)
            else:
                raise ValueError("unknown geometry type %r (the reference dereferences a null pointer here)" % g.kind)
            r.setLinkName(self.tf_prefix_ + "/" + link.name)
            r.urdf_link = link.name
            r.link_offset = urdf.pose_to_transform(it.xyz, it.rpy)
            self.renderables_.append(r)

    def update_link_transforms(self, timestamp=None, tf=None):
        """src/urdf_renderer.cpp:173-190, including quirk Q7: a failed lookup is swallowed and the
        link re-uses the transform left by the previous link."""
        tf = tf if tf is not None else self.tf_
        t = Transform()
        for r in self.renderables_:
            try:
                t = tf.lookup_transform(self.fixed_frame_, r.name, timestamp)
            except Exception as e:                  # noqa: BLE001 - ROS_DEBUG
                log.debug("%s", e)
            # tf::Transform(t.getRotation(), t.getOrigin()) (src/urdf_renderer.cpp:187): the rotation goes through a
            # quaternion and back, in double -- kept, because the last bits of the matrix decide float32 roundings
            r.link_to_fixed = Transform.from_quaternion(t.get_rotation(), t.origin)

    def link_matrices(self):
        return np.stack([r.gl_matrix() for r in self.renderables_]) if self.renderables_ else np.zeros((0, 16))


class FilterParameters:
    """The rosparams of the private node handle (src/urdf_filter.cpp:58-111, launch/filter_parameters.yaml)."""

    def __init__(self, fixed_frame, camera_frame, models, depth_distance_threshold,
                 camera_offset_translation=(0.0, 0.0, 0.0), camera_offset_rotation=(0.0, 0.0, 0.0, 1.0),
                 show_gui=False, filter_replace_value=0.0, use_own_calibration=False,
                 own_calibration=(585.260, 585.028, 317.387, 239.264), silhouette_dilation_px=0,
                 scene_margin=None, scene_margin_rel=0.0):
        self.fixed_frame = fixed_frame
        self.camera_frame = camera_frame
        self.models = models                 # list of dicts: model, tf_prefix, geometry_type, [scale], [ignore],
        #                                      [link_depth_distance_thresholds: [{"link": URDF link name, "threshold": metres,
        #                                        "padding": metres}]] (either value or both: include/rtuf.h, LINK PADDING)
        self.depth_distance_threshold = float(depth_distance_threshold)
        self.camera_offset_translation = tuple(camera_offset_translation)
        self.camera_offset_rotation = tuple(camera_offset_rotation)     # x y z w
        self.show_gui = bool(show_gui)       # accepted and ignored: there is no window system here
        self.filter_replace_value = float(filter_replace_value)
        # the reference's compile-time USE_OWN_CALIBRATION (src/urdf_filter.cpp:38, :462-472) as a parameter: fx fy cx cy used
        # instead of the CameraInfo's P (the reference's hard-coded values by default; they pass through float there)
        self.use_own_calibration = bool(use_own_calibration)
        self.own_calibration = tuple(float(np.float32(v)) for v in own_calibration)
        # new, beyond the reference: widen the rendered robot by this many pixels, 0 .. 16 (rtuf_params.silhouette_dilation_px)
        self.silhouette_dilation_px = int(silhouette_dilation_px)
        # new, beyond the reference: scene planes (include/rtuf.h, SCENE PLANES).  scene_margin (metres, >= 0) enables scene
        # filtering for every stream with the margins {scene_margin, scene_margin_rel in [0, 1)}; None: a scene can be learned
        # and set, but filters nothing
        self.scene_margin = None if scene_margin is None else float(scene_margin)
        self.scene_margin_rel = float(scene_margin_rel)

    @staticmethod
    def from_dict(d):
        off = d.get("camera_offset", {})
        return FilterParameters(d["fixed_frame"], d["camera_frame"], d.get("models", []), d["depth_distance_threshold"],
                                off.get("translation", (0.0, 0.0, 0.0)), off.get("rotation", (0.0, 0.0, 0.0, 1.0)),
                                d.get("show_gui", False), d.get("filter_replace_value", 0.0),
                                d.get("use_own_calibration", False), d.get("own_calibration", (585.260, 585.028, 317.387, 239.264)),
                                d.get("silhouette_dilation_px", 0), d.get("scene_margin"), d.get("scene_margin_rel", 0.0))


class RealtimeURDFFilter:
    """urdf_filter.h:51-143.  One instance serves `max_streams` concurrent cameras (stream 0 is the
    reference-shaped single-camera interface); the public attribute names follow the reference."""

    def __init__(self, params, tf, param_server=None, max_streams=1, mesh_loader=None, device=0, two_kernel=False, labels=False):
        self.params = params
        self.tf_ = tf
        self.param_server = param_server or {}
        self.mesh_loader = mesh_loader
        self.device = device
        self.max_streams = max_streams
        self.two_kernel = two_kernel
        self.fixed_frame_ = params.fixed_frame
        self.cam_frame_ = params.camera_frame
        self.camera_offset_t_ = np.asarray(params.camera_offset_translation, np.float64)
        self.camera_offset_q_ = tuple(params.camera_offset_rotation)
        self.depth_distance_threshold_ = params.depth_distance_threshold
        self.filter_replace_value_ = params.filter_replace_value
        self.silhouette_dilation_px_ = params.silhouette_dilation_px
        self.show_gui_ = params.show_gui
        self.far_plane_, self.near_plane_ = 8.0, 0.1         # src/urdf_filter.cpp:53-54
        self.width_ = self.height_ = 0
        self.camera_tx_ = self.camera_ty_ = 0.0
        self.need_mask_ = True
        self.renderers_ = []
        self.masked_depth_ = None
        self.mask_ = None
        self._ctx = None
        self.link_spheres_ = {}                     # setLinkSpheres: {model: (link, xyzr)}, kept across contexts
        self._spheres_given_ = False                # the context holds link_spheres_ (cleared by initGL and setLinkSpheres)
        self._padded_ = False                       # some model entry gave a link a "padding" (initGL)
        self._model_ids = []
        self._batch_masked = None
        self._batch_mask = None
        # new, beyond the reference: link labels (include/rtuf.h, LINK LABELS), off by default -- filter() costs what it did
        self.want_labels_ = bool(labels)
        self.labels_ = None
        self.virtual_depth_ = None            # new, beyond the reference: the plane of the last render() (VIRTUAL DEPTH)
        self.link_labels_ = {}                # (model index, URDF link name) -> label

    # ---- loading -------------------------------------------------------------------------
    def loadModels(self):
        """src/urdf_filter.cpp:127-197 (appends, like the reference: quirk Q12)."""
        models = self.params.models
        if not isinstance(models, (list, tuple)):
            log.error("models parameter must be an array!")
            return
        for elem in models:
            description_param = elem["model"]
            content = self.param_server.get(description_param)
            if content is None:
                log.error("Parameter [%s] does not exist, and was not found by searchParam()", description_param)
                continue
            if not content:
                log.error("URDF is empty")
                continue
            ignore = elem.get("ignore", [])
            if isinstance(ignore, str):
                ignore = [ignore]
            self.renderers_.append(URDFRenderer(content, elem.get("tf_prefix", ""), self.cam_frame_, self.fixed_frame_,
                                                self.tf_, elem.get("geometry_type", ""), elem.get("scale", 1.0),
                                                ignore, self.mesh_loader))
            # new, beyond the reference: per-link depth thresholds [{"link": <URDF link name>, "threshold": <metres>}, ...]
            # and, beside or instead of "threshold", a link's "padding": <metres> (include/rtuf.h, LINK PADDING)
            rd = self.renderers_[-1]
            rd.link_thresholds_ = {}
            rd.link_padding_ = {}
            for e in elem.get("link_depth_distance_thresholds", []) or []:
                if e["link"] not in rd.link_names_:
                    raise ValueError("link_depth_distance_thresholds of model %r: no link %r in its URDF" % (description_param, e["link"]))
                if "padding" in e:
                    rd.link_padding_[e["link"]] = float(e["padding"])
                if "threshold" in e or "padding" not in e:
                    rd.link_thresholds_[e["link"]] = float(e["threshold"])

    def initGL(self):
        """src/urdf_filter.cpp:386-436 without GL: create the device context for width_ x height_,
        load the models into device buffers, allocate the outputs."""
        p = _capi.default_params()
        p.near_plane, p.far_plane = self.near_plane_, self.far_plane_
        p.depth_distance_threshold = self.depth_distance_threshold_
        p.filter_replace_value = self.filter_replace_value_
        p.silhouette_dilation_px = self.silhouette_dilation_px_
        if self.two_kernel:
            p.flags |= _capi.FLAG_TWO_KERNEL
        if self._ctx is not None:
            self._ctx.close()
        self._cloud_intr_given_ = None              # (the new context has no cloud intrinsics: cloud() gives them again)
        self._pad_intr_given_ = None
        self._spheres_given_ = False                # (... and no link spheres: clearance() gives them again)
        self._ctx = _capi.Context(self.width_, self.height_, self.max_streams, self.device, p)
        self.loadModels()
        if not self.renderers_:
            raise RuntimeError("Could not load any models for filtering!")
        self._model_ids = []
        for rd in self.renderers_:
            m = self._ctx.add_model()
            for r in rd.renderables_:
                l = self._ctx.add_link(m)
                for d in r.draws:
                    self._ctx.add_draw(m, l, d.verts, d.tris, d.pre_op, d.op)
            self._model_ids.append(m)
        self._ctx.finalize_models()
        # one label per URDF link, numbered from 1 over the models in order (every renderable of a link shares it; links on a
        # model's `ignore` list have no renderable and so no label)
        self.link_labels_ = {}
        for mi, (rd, m) in enumerate(zip(self.renderers_, self._model_ids)):
            for r in rd.renderables_:
                self.link_labels_.setdefault((mi, r.urdf_link), len(self.link_labels_) + 1)
            if rd.renderables_ and self.want_labels_:
                self._ctx.set_link_labels(m, [self.link_labels_[(mi, r.urdf_link)] for r in rd.renderables_])
        self.labels_ = np.zeros((self.height_, self.width_), np.uint16) if self.want_labels_ else None
        # per-link depth thresholds: every renderable of a listed URDF link takes its value, the model's other links the
        # global threshold (links on the model's `ignore` list have no renderable: their entries have no effect)
        for rd, m in zip(self.renderers_, self._model_ids):
            if rd.link_thresholds_ and rd.renderables_:
                self._ctx.set_link_thresholds(m, [rd.link_thresholds_.get(r.urdf_link, self.depth_distance_threshold_)
                                                  for r in rd.renderables_])
        # link padding, in loadModels order: every renderable of a listed URDF link takes its margin, the model's other links none
        self._padded_ = False
        for rd, m in zip(self.renderers_, self._model_ids):
            if rd.link_padding_ and rd.renderables_:
                self._ctx.set_link_padding(m, [rd.link_padding_.get(r.urdf_link, 0.0) for r in rd.renderables_])
                self._padded_ = True
        self.masked_depth_ = np.zeros((self.height_, self.width_), np.float32)
        self.mask_ = np.zeros((self.height_, self.width_), np.uint8)
        self._enable_scene()

    def _enable_scene(self):
        """Scene filtering for every stream, with the parameters' margins (a new context's planes are all unknown: nothing is
        filtered until a scene is learned or set)."""
        if self.params.scene_margin is not None:
            self._ctx.set_scene_margins(0, [(self.params.scene_margin, self.params.scene_margin_rel)] * self.max_streams)

    def _give_padding_intrinsics(self, n):
        """Link padding projects its margins with the streams' focal lengths: streams 0 .. n-1 get the intrinsics of the last
        getProjectionMatrix() before a padded batch (initGL clears the record with every new context)."""
        if not self._padded_:
            return
        intr = getattr(self, "cloud_intrinsics_", None)
        if intr is None:
            raise RuntimeError("link padding: no intrinsics yet (getProjectionMatrix sets them)")
        if getattr(self, "_pad_intr_given_", None) != (intr, n):
            self._ctx.set_cloud_intrinsics(0, [intr] * n)
            self._pad_intr_given_ = (intr, n)
            self._cloud_intr_given_ = intr

    # ---- camera --------------------------------------------------------------------------
    def getProjectionMatrix(self, info):
        """src/urdf_filter.cpp:459-501; sets camera_tx_/camera_ty_ as a side effect."""
        if self.params.use_own_calibration:      # the #ifdef branch: own intrinsics, camera_tx_ / camera_ty_ untouched
            fx, fy, cx, cy = self.params.own_calibration
            P, _, _ = _capi.projection_from_intrinsics(fx, fy, cx, cy, info.width, info.height, self.near_plane_, self.far_plane_, 0.0, 0.0)
            self.cloud_intrinsics_ = (fx, fy, cx, cy)
            return P
        P, tx, ty = _capi.projection_from_intrinsics(info.P[0], info.P[5], info.P[2], info.P[6], info.width, info.height,
                                                     self.near_plane_, self.far_plane_, info.P[3], info.P[7])
        self.camera_tx_, self.camera_ty_ = tx, ty
        self.cloud_intrinsics_ = (info.P[0], info.P[5], info.P[2], info.P[6])      # (cloud(): the pinhole the projection was made from)
        return P

    def _camera_matrices(self, tf, timestamp):
        """src/urdf_filter.cpp:520-534, :602-614.  Raises on TF failure (caller implements Q6)."""
        cam = tf.lookup_transform(self.cam_frame_, self.fixed_frame_, timestamp)
        offset = Transform.from_quaternion(self.camera_offset_q_, self.camera_offset_t_)
        offset_inv = offset.inverse().opengl_matrix()
        rot = Transform.from_quaternion(cam.get_rotation())
        right = rot * np.array([1.0, 0.0, 0.0])
        origin = cam.origin + right * self.camera_tx_
        down = rot * np.array([0.0, 1.0, 0.0])
        origin = origin + down * self.camera_ty_
        return offset_inv, Transform(cam.basis, origin).opengl_matrix()

    # ---- the hot path --------------------------------------------------------------------
    def _ensure_size(self, width, height):
        if self.width_ != width or self.height_ != height:
            if self.width_ != 0 or self.height_ != 0:
                log.error("image size has changed (%ix%i) -> (%ix%i)", self.width_, self.height_, width, height)
            self.width_, self.height_ = width, height
            self.initGL()

    def _stage_stream(self, stream, projection, tf, timestamp):
        offset_inv, cam_tf = self._camera_matrices(tf, timestamp)
        self._ctx.set_camera(stream, projection, offset_inv, cam_tf)
        for rd, m in zip(self.renderers_, self._model_ids):
            rd.update_link_transforms(timestamp, tf)
            if rd.renderables_:
                self._ctx.set_link_poses(stream, m, rd.link_matrices())

    def filter(self, buffer, projection_matrix, width, height, timestamp=None):
        """filter(unsigned char* buffer, double* glTf, int width, int height, ros::Time)."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return
        self._give_padding_intrinsics(1)
        depth = np.frombuffer(buffer, np.float32, width * height) if not isinstance(buffer, np.ndarray) else buffer
        d = np.asarray(depth, np.float32).reshape(1, height, width)
        if self.want_labels_:
            masked, mask, labels = self._ctx.filter_batch_labels(d, want_mask=self.need_mask_)
            self.labels_ = labels[0]
        else:
            masked, mask = self._ctx.filter_batch(d, want_mask=self.need_mask_)
        self.masked_depth_ = masked[0]
        if self.need_mask_:
            self.mask_ = mask[0]

    def render(self, projection_matrix, width, height, timestamp=None, empty_value=0.0):
        """New, beyond the reference: the robot's own depth image (include/rtuf.h, VIRTUAL DEPTH) for the camera and link
        poses filter() would use, no sensor image involved.  getVirtualDepth() returns the plane; with labels=True the label
        plane of the same render is in getLabels().  Pixels no link covers hold empty_value."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return
        virt, labels = self._ctx.render_batch(1, empty_value, labels=self.want_labels_)
        self.virtual_depth_ = virt[0]
        if self.want_labels_:
            self.labels_ = labels[0]

    def link_residuals(self, depth, projection_matrix, width, height, timestamp=None):
        """New, beyond the reference: per link label, how the sensor image compares with the model (include/rtuf.h, LINK
        RESIDUAL TABLES) for the camera and link poses filter() would use: pixels covered, confirmed (agree), occluded
        (in_front), seen through (behind), without a reading (invalid), and the summed residual of the confirmed ones.
        depth: [H,W] float32 metres or uint16 millimetres.  Returns the [numLinkResidualRows()] structured array
        (_capi.LINK_RESIDUALS_DTYPE) of the frame, row = label (getLinkLabels() with labels=True, else 1 + the renderable's
        index over all models; row 0: no link), or None where filter() would have returned without a result."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return None
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return None
        d = np.asarray(depth)
        d = d.astype(np.uint16 if d.dtype == np.uint16 else np.float32, copy=False).reshape(1, height, width)
        if d.dtype == np.uint16 and width % 4:      # (the 16UC1 kernels need a width that is a multiple of 4)
            d = d.astype(np.float32) * np.float32(0.001)
        return self._ctx.link_residuals_batch(d, self.numLinkResidualRows())[0]

    def cloud(self, depth, projection_matrix, width, height, timestamp=None, compact=False):
        """New, beyond the reference: the pixels filter() would keep as XYZ points in the camera's optical frame (include/rtuf.h,
        FILTERED POINT CLOUDS), for the camera and link poses filter() would use and the intrinsics of the last
        getProjectionMatrix() (own_calibration, which FilterParameters keeps rounded to float, with use_own_calibration, as the
        projection and the C++ façade take it; else the camera info's fx fy cx cy as doubles).
        depth: [H,W] float32 metres or uint16 millimetres; the width must be a multiple of 4.  Returns [H,W,3] float32 with NaN
        where there is no point, or with compact=True (points [count,3], index [count] = v * width + u) in row-major order;
        None where filter() would have returned without a result."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return None
        intr = getattr(self, "cloud_intrinsics_", None)
        if intr is None:
            raise RuntimeError("cloud(): no intrinsics yet (getProjectionMatrix sets them)")
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return None
        if getattr(self, "_cloud_intr_given_", None) != intr:      # (initGL clears it with every new context)
            self._ctx.set_cloud_intrinsics(0, intr)
            self._cloud_intr_given_ = intr
        d = np.asarray(depth)
        d = d.astype(np.uint16 if d.dtype == np.uint16 else np.float32, copy=False).reshape(1, height, width)
        if not compact:
            return self._ctx.cloud_batch(d)[0]
        points, index, counts = self._ctx.cloud_compact_batch(d, width * height)
        return points[0, :counts[0]], index[0, :counts[0]]

    def filter_points(self, points, projection_matrix, width, height, timestamp=None, radius_px=0):
        """New, beyond the reference: a point list instead of a depth image (include/rtuf.h, POINT LIST BATCHES) -- a lidar's
        points, a cloud that was cropped or transformed, the compact output of cloud() -- for the camera and link poses filter()
        would use and the intrinsics of the last getProjectionMatrix(), as cloud() takes them.
        points: [count,3] float32 in the camera's optical frame (x right, y down, z forward); radius_px 0 .. 4 widens the robot
        by that many pixels.  Returns (verdict [count] uint8 -- 0 kept, 1 filtered: on the robot, 2 outside the image or without
        a positive finite z --, pixel [count] uint32 = v * width + u, 0xFFFFFFFF where the verdict is 2, summary [4] uint32: kept,
        filtered, outside, count); None where filter() would have returned without a result."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return None
        intr = getattr(self, "cloud_intrinsics_", None)
        if intr is None:
            raise RuntimeError("filter_points(): no intrinsics yet (getProjectionMatrix sets them)")
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return None
        if getattr(self, "_cloud_intr_given_", None) != intr:      # (initGL clears it with every new context)
            self._ctx.set_cloud_intrinsics(0, intr)
            self._cloud_intr_given_ = intr
        verdict, pixel, summary = self._ctx.points_batch([np.asarray(points, np.float32).reshape(-1, 3)], radius_px)
        return verdict[0], pixel[0], summary[0]

    def setLinkSpheres(self, model, link, xyzr):
        """New, beyond the reference: the sphere list of model `model` (index into the loaded models) for clearance(): link [n] =
        renderable index within the model, xyzr [n,4] = centre in the renderable's (link's) frame -- a draw's pre_op applied to its
        vertices first -- and radius
        (geometry.bounding_spheres makes them from a draw's vertices).  Kept across image-size changes."""
        li = np.ascontiguousarray(link, np.int32).reshape(-1).copy()
        q = np.ascontiguousarray(xyzr, np.float32).reshape(-1, 4).copy()
        self.link_spheres_[int(model)] = (li, q)
        self._spheres_given_ = False

    def clearance(self, depth, projection_matrix, width, height, max_distance, timestamp=None):
        """New, beyond the reference: per link label, the nearest kept point to the link's spheres (include/rtuf.h, LINK
        CLEARANCE TABLES) for the camera, link poses and intrinsics cloud() would use and the spheres of setLinkSpheres().
        depth: [H,W] float32 metres or uint16 millimetres.  Returns the [numLinkResidualRows()] structured array
        (_capi.LINK_CLEARANCE_DTYPE), row = label, row 0 = the whole robot; None where filter() would have returned without a
        result."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return None
        intr = getattr(self, "cloud_intrinsics_", None)
        if intr is None:
            raise RuntimeError("clearance(): no intrinsics yet (getProjectionMatrix sets them)")
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return None
        if getattr(self, "_cloud_intr_given_", None) != intr:      # (initGL clears it with every new context)
            self._ctx.set_cloud_intrinsics(0, intr)
            self._cloud_intr_given_ = intr
        if not self._spheres_given_:
            for model, (li, q) in sorted(self.link_spheres_.items()):
                self._ctx.set_link_spheres(model, li, q)
            self._spheres_given_ = True
        d = np.asarray(depth)
        d = d.astype(np.uint16 if d.dtype == np.uint16 else np.float32, copy=False).reshape(1, height, width)
        return self._ctx.link_clearance_batch(d, self.numLinkResidualRows(), max_distance)[0]

    # ---- voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS) ------------------------
    def setVoxelGrid(self, origin, voxel_size, dims, with_counts=True, world_from_optical=None):
        """New, beyond the reference: one world grid that voxelInsert() accumulates kept points in.  origin [3] and voxel_size
        in metres, dims (nx, ny, nz); world_from_optical: None or the camera's column-major [16] matrix.  The grid belongs to the
        device context: a new image size makes a new, empty one.  dims None drops it."""
        self.voxel_grid_ = None if dims is None else (tuple(float(q) for q in origin), float(voxel_size), tuple(int(q) for q in dims), bool(with_counts),
                                                      None if world_from_optical is None else np.array(world_from_optical, np.float64).reshape(16))
        self._voxel_ctx_ = None
        if dims is None and self._ctx is not None:
            self._ctx.set_voxel_grid(None, 0.0, None)

    def _give_voxel_grid(self):
        grid = getattr(self, "voxel_grid_", None)
        if grid is None:
            raise RuntimeError("no voxel grid yet (setVoxelGrid)")
        if getattr(self, "_voxel_ctx_", None) is not self._ctx:      # (a new context holds no grid)
            self._ctx.set_voxel_grid(grid[0], grid[1], grid[2], grid[3])
            self._ctx.set_voxel_transforms(0, grid[4])
            self._voxel_ctx_ = self._ctx

    def voxelInsert(self, depth, projection_matrix, width, height, timestamp=None):
        """Inserts the pixels filter() would keep -- dilation, thresholds, padding and scene honoured -- into the grid of
        setVoxelGrid(), for the camera and link poses filter() would use and the intrinsics cloud() would use.  depth: [H,W]
        float32 metres or uint16 millimetres; the width must be a multiple of 4.  Returns the summary [4] uint32 (inserted,
        outside the grid, not kept, total); None where filter() would have returned without a result."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return None
        intr = getattr(self, "cloud_intrinsics_", None)
        if intr is None:
            raise RuntimeError("voxelInsert(): no intrinsics yet (getProjectionMatrix sets them)")
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return None
        if getattr(self, "_cloud_intr_given_", None) != intr:      # (initGL clears it with every new context)
            self._ctx.set_cloud_intrinsics(0, intr)
            self._cloud_intr_given_ = intr
        self._give_voxel_grid()
        d = np.asarray(depth)
        d = d.astype(np.uint16 if d.dtype == np.uint16 else np.float32, copy=False).reshape(1, height, width)
        return self._ctx.voxel_insert_batch(d)[0]

    def voxelClear(self):
        if self._ctx is not None and getattr(self, "_voxel_ctx_", None) is self._ctx:
            self._ctx.voxel_clear()

    def voxelGrid(self):
        """(bits [ceil(nx * ny * nz / 32)] uint32, counts [nz,ny,nx] uint32 or None) of the grid as it stands."""
        if self._ctx is None:
            raise RuntimeError("voxelGrid(): no frame yet")
        self._give_voxel_grid()
        return self._ctx.voxel_grid()

    # ---- voxel free space (include/rtuf.h, VOXEL FREE SPACE) ----------------------------------
    def voxelCarve(self, depth, projection_matrix, width, height, margin, radius_px=0):
        """New, beyond the reference: marks the voxels of setVoxelGrid()'s grid that the camera sees THROUGH -- whose centre lies
        more than `margin` metres in front of the smallest valid reading within radius_px pixels of its pixel -- with the
        intrinsics cloud() would use.  The mask is not read and no model is posed.  depth: [H,W] float32 metres or uint16
        millimetres, any width; projection_matrix is not read (the pinhole is getProjectionMatrix's).  Returns the summary [4]
        uint32 (free, not free, not seen, n_voxels); None where filter() would have returned without a result."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return None
        intr = getattr(self, "cloud_intrinsics_", None)
        if intr is None:
            raise RuntimeError("voxelCarve(): no intrinsics yet (getProjectionMatrix sets them)")
        if getattr(self, "_cloud_intr_given_", None) != intr:      # (initGL clears it with every new context)
            self._ctx.set_cloud_intrinsics(0, intr)
            self._cloud_intr_given_ = intr
        self._give_voxel_grid()
        d = np.asarray(depth)
        d = d.astype(np.uint16 if d.dtype == np.uint16 else np.float32, copy=False).reshape(1, height, width)
        return self._ctx.voxel_carve_batch(d, margin, radius_px)[0]

    def voxelFree(self):
        """[ceil(nx * ny * nz / 32)] uint32: the free words of the grid as they stand.  Occupied wins over free; a voxel with
        neither bit is unknown."""
        if self._ctx is None:
            raise RuntimeError("voxelFree(): no frame yet")
        self._give_voxel_grid()
        return self._ctx.voxel_free()

    # ---- scene planes (include/rtuf.h, SCENE PLANES) ------------------------------------------
    def learnScene(self, depth, projection_matrix, width, height, timestamp=None):
        """New, beyond the reference: lowers stream 0's scene plane to the readings of every pixel the robot filter keeps, for the
        camera and link poses filter() would use -- call it for a few frames of the empty cell while the robot moves, with link
        padding in the model entries so that the arm's halo is not learned.  depth: [H,W] float32 metres or uint16 millimetres.
        Returns False where filter() would have returned without a result."""
        self._ensure_size(width, height)
        if not self.renderers_:
            return False
        try:
            self._stage_stream(0, projection_matrix, self.tf_, timestamp)
        except Exception as e:                      # noqa: BLE001 - ROS_ERROR + return (quirk Q6)
            log.error("%s", e)
            return False
        self._give_padding_intrinsics(1)
        d = np.asarray(depth)
        d = d.astype(np.uint16 if d.dtype == np.uint16 else np.float32, copy=False).reshape(1, height, width)
        self._ctx.learn_scene_batch(d)
        return True

    def learnSceneBatch(self, depths, projections, tfs, timestamp=None):
        """learnScene for streams 0 .. N-1 at once (the arguments of filter_batch); a stream whose camera lookup fails makes the
        call fail: a plane must not be learned with stale poses."""
        depths = np.asarray(depths)
        depths = np.ascontiguousarray(depths, np.uint16 if depths.dtype == np.uint16 else np.float32)
        n, height, width = depths.shape
        self._ensure_size(width, height)
        projections = np.asarray(projections, np.float64).reshape(-1, 16)
        for s in range(n):
            self._stage_stream(s, projections[s if len(projections) > 1 else 0], tfs[s], timestamp)
        self._give_padding_intrinsics(n)
        self._ctx.learn_scene_batch(depths)

    def setScene(self, planes, first_stream=0):
        """The scene planes of streams first_stream ..: [H,W] or [n,H,W] float32 metres, +inf or NaN where unknown.  The image
        size is the planes' (a context of another size is replaced, as by filter())."""
        a = np.ascontiguousarray(planes, np.float32)
        a = a.reshape((-1,) + a.shape[-2:])
        self._ensure_size(a.shape[2], a.shape[1])
        self._ctx.set_scene_planes(first_stream, a)

    def getScene(self):
        """Stream 0's scene plane [H,W] float32 (max_streams > 1: all of them, [n,H,W]); None before the first frame."""
        if self._ctx is None:
            return None
        planes = self._ctx.get_scene_planes()
        return planes[0] if self.max_streams == 1 else planes

    def clearScene(self):
        """Every stream's plane back to unknown; the parameters' margins stay in force for the next scene."""
        if self._ctx is not None:
            self._ctx.clear_scene()
            self._enable_scene()

    def numLinkResidualRows(self):
        """Rows of a link_residuals() table: one more than the largest label in effect."""
        if self.want_labels_:
            return max(self.link_labels_.values(), default=0) + 1
        return sum(len(rd.renderables_) for rd in self.renderers_) + 1

    def getVirtualDepth(self):
        """Virtual depth plane [H,W] float32 metres of the last render() (None before the first)."""
        return self.virtual_depth_

    def getMaskedDepth(self):
        return self.masked_depth_

    def getLabels(self):
        """Link label plane [H,W] uint16 of the last frame (labels=True), label 0 = background quad or nothing drawn."""
        return self.labels_

    def getLinkLabels(self):
        """{(model index, URDF link name): label} of the links the labels plane can show."""
        return dict(self.link_labels_)

    def filter_callback(self, image, encoding, camera_info, stamp=None):
        """src/urdf_filter.cpp:270-330.  image: [H,W] float32 metres ("32FC1") or uint16 millimetres
        ("16UC1").  Returns (output_depth in the input encoding, mask or None)."""
        if encoding == "32FC1":
            depth_image = np.ascontiguousarray(image, np.float32)
        elif encoding == "16UC1":
            depth_image = depth_u16_to_f32(image)
        else:
            log.error("cv_bridge Exception: unsupported encoding %s", encoding)
            return None, None
        projection_matrix = self.getProjectionMatrix(camera_info)
        self.filter(depth_image, projection_matrix, depth_image.shape[1], depth_image.shape[0], stamp)
        out = self.masked_depth_
        if encoding == "16UC1":
            out = depth_f32_to_u16(out)
        return out, (self.mask_ if self.need_mask_ else None)

    # ---- batched extension ---------------------------------------------------------------
    def filter_batch(self, depths, projections, tfs, timestamp=None, want_mask=True):
        """N streams at once: depths [N,H,W] f32, projections [N,16] (or one [16]), tfs: one
        transform provider per stream.  A stream whose camera lookup fails keeps its previous
        output (quirk Q6)."""
        depths = np.ascontiguousarray(depths, np.float32)
        n, height, width = depths.shape
        self._ensure_size(width, height)
        projections = np.asarray(projections, np.float64).reshape(-1, 16)
        failed = []
        for s in range(n):
            P = projections[s if len(projections) > 1 else 0]
            try:
                self._stage_stream(s, P, tfs[s], timestamp)
            except Exception as e:                  # noqa: BLE001
                log.error("stream %d: %s", s, e)
                failed.append(s)
        self._give_padding_intrinsics(n)
        masked, mask = self._ctx.filter_batch(depths, want_mask=want_mask)
        if self._batch_masked is None or self._batch_masked.shape != masked.shape:
            self._batch_masked = np.zeros_like(masked)
            self._batch_mask = np.zeros(masked.shape, np.uint8)
        for s in range(n):
            if s in failed:
                continue
            self._batch_masked[s] = masked[s]
            if want_mask:
                self._batch_mask[s] = mask[s]
        return self._batch_masked[:n], (self._batch_mask[:n] if want_mask else None)

    def stats(self):
        return self._ctx.stats() if self._ctx else {}


def depth_u16_to_f32(img_u16):
    """cv::Mat::convertTo(CV_32F, 0.001) (src/urdf_filter.cpp:288): float32 product, one rounding."""
    return (np.asarray(img_u16, np.uint16).astype(np.float32) * np.float32(0.001)).astype(np.float32)


def depth_f32_to_u16(img_f32):
    """cv::Mat::convertTo(CV_16U, 1000.0) (src/urdf_filter.cpp:311): float32 product, round half to even,
    saturate; NaN / +-inf -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(img_f32, np.float32) * np.float32(1000.0)).astype(np.float32)
        # cvRound on NaN / values outside the int32 range yields the "integer indefinite" value, which
        # saturate_cast<ushort> maps to 0
        bad = ~((v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0)))
        r = np.rint(np.where(bad, 0.0, v))
        return np.clip(r, 0, 65535).astype(np.uint16)
