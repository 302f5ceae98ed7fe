// urdf_filter.hpp -- C++ facade over the C ABI (include/rtuf.h) that keeps the reference's class
// surface for the hot path: same class names, method names, argument meaning and error behaviour as
//   realtime_urdf_filter::RealtimeURDFFilter   include/realtime_urdf_filter/urdf_filter.h:51-143
//   realtime_urdf_filter::URDFRenderer         include/realtime_urdf_filter/urdf_renderer.h:45-73
//   realtime_urdf_filter::Renderable*          include/realtime_urdf_filter/renderable.h:54-143
// with the ROS types replaced by plain ones (no ROS exists where this is built):
//   ros::NodeHandle rosparams        -> FilterParameters (+ a string map as parameter server)
//   tf::TransformListener            -> rtuf_host::TransformProvider
//   sensor_msgs::CameraInfo          -> CameraInfo {width, height, P[12]}
//   ros::Time                        -> double seconds (unused by static providers)
// A ROS adapter only has to fill these from its node handle / tf listener / messages
// (INTEGRATION.md).  Header-only; link with librtuf.so.
#pragma once

#include <cmath>
#include <map>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../rtuf.h"
#include "host.hpp"

namespace realtime_urdf_filter {

using rtuf_host::Transform;
using rtuf_host::TransformProvider;

struct CameraInfo {
  int width = 0, height = 0;
  double P[12] = {0};      // row-major 3x4 projection matrix of sensor_msgs/CameraInfo
};

// ---- renderable.h ---------------------------------------------------------------------------
struct Renderable {
  virtual ~Renderable() = default;
  void setLinkName(std::string n) { name = std::move(n); }
  std::string name;
  std::string urdf_link;                        // the URDF link's own name (`name` carries the tf prefix): its label's key
  Transform link_offset;
  Transform link_to_fixed;
  std::vector<rtuf_host::DrawCall> draws;       // what render() hands to the GPU
  // applyTransform (src/renderable.cpp:59-68): (link_to_fixed * link_offset).getOpenGLMatrix()
  void gl_matrix(double g[16]) const { (link_to_fixed * link_offset).opengl_matrix(g); }
};
struct RenderableBox : Renderable {
  RenderableBox(float dimx_, float dimy_, float dimz_) : dimx(dimx_), dimy(dimy_), dimz(dimz_) { draws = rtuf_host::box_draws(dimx, dimy, dimz); }
  float dimx, dimy, dimz;
};
struct RenderableSphere : Renderable {
  explicit RenderableSphere(float radius_) : radius(radius_) { draws = rtuf_host::sphere_draws(radius); }
  float radius;
};
struct RenderableCylinder : Renderable {
  RenderableCylinder(float radius_, float length_) : radius(radius_), length(length_) { draws = rtuf_host::cylinder_draws(radius, length); }
  float radius, length;
};
// Resolves a mesh URI (package://, file://, ...) to file contents; returns false when unavailable
// (resource_retriever in the reference).
using MeshResolver = bool (*)(const std::string& uri, std::string& data, void* user);
struct RenderableMesh : Renderable {
  // src/renderable.cpp:306-322: a mesh that cannot be loaded becomes a renderable that draws nothing
  RenderableMesh(const std::string& meshname, float sx, float sy, float sz, MeshResolver resolve, void* user)
  {
    std::string data;
    std::vector<float> v;
    std::vector<uint32_t> t;
    if (!resolve) resolve = &rtuf_host::default_mesh_resolver;        // package:// against ROS_PACKAGE_PATH, file://, plain paths
    if (resolve(meshname, data, user) && rtuf_host::load_mesh(meshname, data, v, t)) draws = rtuf_host::mesh_draws(v, t, sx, sy, sz);
    else std::fprintf(stderr, "[realtime_urdf_filter] Could not load resource [%s]\n", meshname.c_str());
  }
};

// ---- urdf_renderer.h ------------------------------------------------------------------------
class URDFRenderer {
 public:
  URDFRenderer(std::string model_description, std::string tf_prefix, std::string cam_frame, std::string fixed_frame,
               const TransformProvider& tf, const std::string& geometry_type_, double scale_,
               const std::unordered_set<std::string>& ignore_, MeshResolver resolve = nullptr, void* resolve_user = nullptr)
      : model_description_(std::move(model_description)), tf_prefix_(std::move(tf_prefix)), geometry_type(geometry_type_), scale(scale_),
        ignore(ignore_), camera_frame_(std::move(cam_frame)), fixed_frame_(std::move(fixed_frame)), tf_(tf), resolve_(resolve), resolve_user_(resolve_user)
  {
    initURDFModel();
  }

  // src/urdf_renderer.cpp:173-190 incl. the stale-transform behaviour on lookup failure (quirk Q7)
  void update_link_transforms(double /*timestamp*/ = 0.0)
  {
    Transform t;
    for (auto& r : renderables_) {
      Transform looked;
      if (tf_.lookup(fixed_frame_, r->name, looked)) t = looked;
      // tf::Transform(t.getRotation(), t.getOrigin()) (src/urdf_renderer.cpp:187): matrix -> quaternion -> matrix, in double
      r->link_to_fixed = Transform::from_quaternion(t.rotation(), t.o);
    }
  }
  std::vector<std::shared_ptr<Renderable>> renderables_;

 protected:
  void initURDFModel()
  {
    try {
      loadURDFModel(rtuf_host::UrdfModel::from_string(model_description_));
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[realtime_urdf_filter] URDF failed Model parse: %s\n", e.what());
    }
  }
  void loadURDFModel(const rtuf_host::UrdfModel& model)
  {
    for (const auto& l : model.links) link_names.insert(l.first);
    for (const auto& l : model.links) process_link(l.second);
  }
  // src/urdf_renderer.cpp:100-169
  void process_link(const rtuf_host::UrdfLink& link)
  {
    if (ignore.count(link.name)) return;
    const std::vector<rtuf_host::UrdfVisual>* items = nullptr;
    if (geometry_type.empty() || geometry_type == "visual") items = &link.visual_array;
    else if (geometry_type == "collision") items = &link.collision_array;
    else { std::fprintf(stderr, "[realtime_urdf_filter] invalid geometry type: %s\n", geometry_type.c_str()); return; }
    for (const auto& it : *items) {
      const rtuf_host::UrdfGeometry& g = it.geometry;
      std::shared_ptr<Renderable> r;
      switch (g.kind) {
        case rtuf_host::UrdfGeometry::BOX: r = std::make_shared<RenderableBox>((float)(scale * g.size.x), (float)(scale * g.size.y), (float)(scale * g.size.z)); break;
        case rtuf_host::UrdfGeometry::CYLINDER: r = std::make_shared<RenderableCylinder>((float)(scale * g.radius), (float)(scale * g.length)); break;
        case rtuf_host::UrdfGeometry::SPHERE: r = std::make_shared<RenderableSphere>((float)(scale * g.radius)); break;
        case rtuf_host::UrdfGeometry::MESH:
          r = std::make_shared<RenderableMesh>(g.filename, (float)(scale * g.scale.x), (float)(scale * g.scale.y), (float)(scale * g.scale.z), resolve_, resolve_user_);
          break;
      }
      r->setLinkName(tf_prefix_ + "/" + link.name);
      r->urdf_link = link.name;
      r->link_offset = rtuf_host::pose_to_transform(it.xyz, it.rpy);
      renderables_.push_back(r);
    }
  }

  std::string model_description_, tf_prefix_;
  const std::string geometry_type;
  const double scale;
  const std::unordered_set<std::string> ignore;
 public:
  std::unordered_set<std::string> link_names;    // every link of the URDF, ignored ones included
  std::map<std::string, double> link_thresholds; // URDF link name -> depth threshold of its own (RealtimeURDFFilter::loadModels)
  std::map<std::string, double> link_padding;    // URDF link name -> padding in metres (RealtimeURDFFilter::loadModels)
 protected:
  std::string camera_frame_, fixed_frame_;
  const TransformProvider& tf_;
  MeshResolver resolve_;
  void* resolve_user_;
};

// ---- the rosparams of the private node handle (src/urdf_filter.cpp:58-111) ------------------
struct ModelParameter {
  std::string model;            // name of the parameter that holds the URDF XML
  std::string tf_prefix;
  std::string geometry_type;    // "visual" | "collision"
  double scale = 1.0;
  std::unordered_set<std::string> ignore;
  // New, beyond the reference: per-link depth thresholds (include/rtuf.h, PER-LINK DEPTH THRESHOLDS), keyed by URDF link
  // name.  Every renderable of the link takes the value, the model's other links the global depth_distance_threshold; a name
  // that is no link of the model's URDF is an error at load, a link on the ignore list is accepted and has no effect.
  std::vector<std::pair<std::string, double>> link_depth_distance_thresholds;
  // New, beyond the reference: link padding (include/rtuf.h, LINK PADDING), keyed by URDF link name like the thresholds: a margin
  // in metres around the silhouette of every renderable of the link, none for the model's other links.  Needs the intrinsics
  // of getProjectionMatrix before the first frame; not together with thresholds, link_labels or silhouette_dilation_px > 0.
  std::vector<std::pair<std::string, double>> link_padding;
};
struct FilterParameters {
  std::string fixed_frame, camera_frame;
  double camera_offset_translation[3] = {0, 0, 0};
  double camera_offset_rotation[4] = {0, 0, 0, 1};   // x y z w
  double depth_distance_threshold = 0.05;
  bool show_gui = false;                             // accepted, ignored (no window system)
  double filter_replace_value = 0.0;
  std::vector<ModelParameter> models;
  // The reference's compile-time switch USE_OWN_CALIBRATION (src/urdf_filter.cpp:38, :462-472) as a run-time parameter: with
  // it, getProjectionMatrix ignores the CameraInfo's P (only width and height are used) and takes these intrinsics instead
  // -- the reference's hard-coded Kinect values by default -- and leaves camera_tx_ / camera_ty_ alone, as the #ifdef does.
  bool use_own_calibration = false;
  double own_calibration[4] = {585.260, 585.028, 317.387, 239.264};      // fx fy cx cy
  // New, beyond the reference: widen the rendered robot by this many pixels, 0 .. 16 (rtuf_params.silhouette_dilation_px)
  unsigned silhouette_dilation_px = 0;
  // New, beyond the reference: also produce the link label plane (include/rtuf.h, LINK LABELS; getLabels(), linkLabels()).
  // Off by default: filter() then costs what it did.  Not together with silhouette_dilation_px > 0.
  bool link_labels = false;
  // New, beyond the reference: scene planes (include/rtuf.h, SCENE PLANES).  scene_margin >= 0 (metres) enables scene filtering
  // with the margins {scene_margin, scene_margin_rel in [0, 1)}; negative (the default): a scene can be learned and set, but
  // filters nothing.
  double scene_margin = -1.0, scene_margin_rel = 0.0;
};

// ---- urdf_filter.h --------------------------------------------------------------------------
class RealtimeURDFFilter {
 public:
  RealtimeURDFFilter(const FilterParameters& params, const TransformProvider& tf,
                     std::map<std::string, std::string> param_server, int device = 0, MeshResolver resolve = nullptr, void* resolve_user = nullptr)
      : tf_(tf), fixed_frame_(params.fixed_frame), cam_frame_(params.camera_frame), show_gui_(params.show_gui),
        depth_distance_threshold_(params.depth_distance_threshold), filter_replace_value_(params.filter_replace_value),
        silhouette_dilation_px_(params.silhouette_dilation_px),
        params_(params), param_server_(std::move(param_server)), device_(device), resolve_(resolve), resolve_user_(resolve_user),
        want_labels_(params.link_labels)
  {
  }
  ~RealtimeURDFFilter() { if (ctx_) rtuf_destroy(ctx_); }
  RealtimeURDFFilter(const RealtimeURDFFilter&) = delete;
  RealtimeURDFFilter& operator=(const RealtimeURDFFilter&) = delete;

  // loads URDF models (src/urdf_filter.cpp:127-197)
  void loadModels()
  {
    for (const ModelParameter& elem : params_.models) {
      auto it = param_server_.find(elem.model);
      if (it == param_server_.end()) { std::fprintf(stderr, "[realtime_urdf_filter] Parameter [%s] does not exist\n", elem.model.c_str()); continue; }
      if (it->second.empty()) { std::fprintf(stderr, "[realtime_urdf_filter] URDF is empty\n"); continue; }
      renderers_.push_back(new URDFRenderer(it->second, elem.tf_prefix, cam_frame_, fixed_frame_, tf_, elem.geometry_type, elem.scale, elem.ignore,
                                            resolve_, resolve_user_));
      for (const auto& lt : elem.link_depth_distance_thresholds) {
        if (!renderers_.back()->link_names.count(lt.first))
          throw std::runtime_error("link_depth_distance_thresholds of model " + elem.model + ": no link '" + lt.first + "' in its URDF");
        renderers_.back()->link_thresholds[lt.first] = lt.second;
      }
      for (const auto& lp : elem.link_padding) {
        if (!renderers_.back()->link_names.count(lp.first))
          throw std::runtime_error("link_padding of model " + elem.model + ": no link '" + lp.first + "' in its URDF");
        renderers_.back()->link_padding[lp.first] = lp.second;
      }
    }
  }

  // does virtual rendering and filtering based on depth buffer and opengl proj. matrix
  // (src/urdf_filter.cpp:207-267)
  void filter(unsigned char* buffer, double* glTf, int width, int height, double timestamp = 0.0)
  {
    if (width_ != width || height_ != height) {
      if (width_ != 0 || height_ != 0) std::fprintf(stderr, "[realtime_urdf_filter] image size has changed (%ix%i) -> (%ix%i)\n", width_, height_, width, height);
      width_ = width;
      height_ = height;
      this->initGL();
    }
    if (renderers_.empty()) return;
    textureBufferFromDepthBuffer(buffer, width_ * height_ * (int)sizeof(float));
    this->render(glTf, timestamp);
  }

  // set up the device context (the reference's OpenGL set-up, src/urdf_filter.cpp:386-436)
  void initGL()
  {
    rtuf_params p;
    rtuf_default_params(&p);
    p.near_plane = (float)near_plane_;
    p.far_plane = (float)far_plane_;
    p.depth_distance_threshold = (float)depth_distance_threshold_;
    p.filter_replace_value = (float)filter_replace_value_;
    p.silhouette_dilation_px = silhouette_dilation_px_;
    if (ctx_) { rtuf_destroy(ctx_); ctx_ = nullptr; }
    cloud_intr_sent_ = false;                  // (the new context has no cloud intrinsics: cloud_into gives them again)
    spheres_sent_ = false;                     // (... and no link spheres: clearance_into gives them again)
    voxel_sent_ = false;                       // (... and no voxel grid: voxel_insert gives it again, empty)
    if (rtuf_create(&ctx_, device_, width_, height_, 1, &p) != RTUF_OK) throw std::runtime_error(std::string("ERROR: could not initialize the GPU context: ") + rtuf_last_error(nullptr));
    this->loadModels();
    if (renderers_.empty()) throw std::runtime_error("Could not load any models for filtering!");
    model_ids_.clear();
    for (URDFRenderer* rd : renderers_) {
      const int m = rtuf_add_model(ctx_);
      for (const auto& r : rd->renderables_) {
        const int l = rtuf_add_link(ctx_, m);
        for (const rtuf_host::DrawCall& d : r->draws)
          check(rtuf_add_draw(ctx_, m, l, d.pre_op, d.op, d.verts.data(), (int)(d.verts.size() / 3), d.tris.data(), (int)(d.tris.size() / 3)));
      }
      model_ids_.push_back(m);
    }
    check(rtuf_finalize_models(ctx_));
    // one label per URDF link, numbered from 1 over the models in order; every renderable of a link shares it, links on a
    // model's ignore list have no renderable and no label
    link_labels_.clear();
    for (size_t i = 0; i < renderers_.size(); i++) {
      std::vector<uint16_t> lab;
      for (const auto& r : renderers_[i]->renderables_) {
        auto key = std::make_pair((int)i, r->urdf_link);
        auto it = link_labels_.find(key);
        if (it == link_labels_.end()) it = link_labels_.emplace(key, (uint16_t)(link_labels_.size() + 1)).first;
        lab.push_back(it->second);
      }
      if (want_labels_ && !lab.empty()) check(rtuf_set_link_labels(ctx_, model_ids_[i], lab.data(), (int)lab.size()));
    }
    applied_threshold_ = depth_distance_threshold_;
    apply_link_thresholds();
    // link padding, in loadModels order: every renderable of a listed URDF link takes its margin, the model's other links none
    padded_ = false;
    for (size_t i = 0; i < renderers_.size(); i++) {
      const URDFRenderer* rd = renderers_[i];
      if (rd->link_padding.empty() || rd->renderables_.empty()) continue;
      std::vector<float> pad;
      for (const auto& r : rd->renderables_) {
        auto it = rd->link_padding.find(r->urdf_link);
        pad.push_back(it != rd->link_padding.end() ? (float)it->second : 0.0f);
      }
      check(rtuf_set_link_padding(ctx_, model_ids_[i], pad.data(), (int)pad.size()));
      padded_ = true;
    }
    labels_.assign(want_labels_ ? (size_t)width_ * height_ : 0, 0);
    masked_depth_ = nullptr;
    mask_ = nullptr;
    enable_scene();
  }

  // compute Projection matrix from CameraInfo message (src/urdf_filter.cpp:459-501)
  void getProjectionMatrix(const CameraInfo& info, double* glTf)
  {
    if (params_.use_own_calibration) {          // (P[3] = P[7] = 0 into a scratch pair: the members keep their values)
      const double* k = params_.own_calibration;
      double tx = 0, ty = 0;
      rtuf_projection_from_intrinsics((float)k[0], (float)k[1], (float)k[2], (float)k[3], 0.0, 0.0, info.width, info.height, near_plane_, far_plane_, glTf, &tx, &ty);
      for (int i = 0; i < 4; i++) cloud_intr_[i] = (double)(float)k[i];      // (own_calibration counts as floats, here as in the projection above and in filter.py)
      have_cloud_intr_ = true;
      return;
    }
    rtuf_projection_from_intrinsics(info.P[0], info.P[5], info.P[2], info.P[6], info.P[3], info.P[7], info.width, info.height, near_plane_, far_plane_, glTf,
                                    &camera_tx_, &camera_ty_);
    cloud_intr_[0] = info.P[0]; cloud_intr_[1] = info.P[5]; cloud_intr_[2] = info.P[2]; cloud_intr_[3] = info.P[6];      // (cloud_into: the pinhole the projection was made from)
    have_cloud_intr_ = true;
  }

  // src/urdf_filter.cpp:503-744 without GL
  void render(const double* camera_projection_matrix, double timestamp = 0.0)
  {
    if (!ctx_ || !stage_frame(camera_projection_matrix, timestamp)) return;
    if (want_labels_) {
      // the single-stream call has no label form: the same frame through the labelled batch call into the façade's planes
      const size_t px = (size_t)width_ * height_;
      own_masked_.resize(px);
      own_mask_.resize(need_mask_ ? px : 0);
      const float* in = reinterpret_cast<const float*>(pending_buffer_);
      float* out = own_masked_.data();
      uint8_t* km = need_mask_ ? own_mask_.data() : nullptr;
      uint16_t* lab = labels_.data();
      check(rtuf_filter_batch_labels(ctx_, 1, &in, &out, need_mask_ ? &km : nullptr, &lab));
      masked_depth_ = own_masked_.data();
      if (need_mask_) mask_ = own_mask_.data();
      return;
    }
    check(rtuf_filter(ctx_, pending_buffer_, nullptr, width_, height_));
    masked_depth_ = rtuf_get_masked_depth(ctx_);
    if (need_mask_) mask_ = rtuf_get_mask(ctx_);
  }

  // Link labels (FilterParameters::link_labels): the label plane of the last frame (width x height, row 0 first; 0 = the
  // background quad or nothing drawn; empty while labels are off), and the label of every (model index, URDF link name).
  const std::vector<uint16_t>& getLabels() const { return labels_; }
  const std::map<std::pair<int, std::string>, uint16_t>& linkLabels() const { return link_labels_; }

  // Virtual depth (include/rtuf.h, VIRTUAL DEPTH): the robot's own depth image for the camera and link poses filter_into would
  // use, no sensor image involved.  virtual_out: width x height float metres, or uint16 millimetres with is_16uc1 (width a
  // multiple of 4); pixels no link covers hold empty_value.  labels_out: nullptr or width x height uint16 (needs
  // FilterParameters::link_labels, kept for getLabels()).  The plane is also kept for getVirtualDepth(), in metres.
  bool render_into(double* glTf, int width, int height, double timestamp, void* virtual_out, bool is_16uc1 = false, float empty_value = 0.0f,
                   uint16_t* labels_out = nullptr)
  {
    prepare(width, height);
    if (!virtual_out || (labels_out && !want_labels_)) throw std::runtime_error("render_into: needs virtual_out, and FilterParameters::link_labels for labels_out");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    const size_t px = (size_t)width_ * height_;
    if (is_16uc1) check(rtuf_render_batch_u16(ctx_, 1, reinterpret_cast<uint16_t* const*>(&virtual_out), labels_out ? &labels_out : nullptr, empty_value));
    else check(rtuf_render_batch(ctx_, 1, reinterpret_cast<float* const*>(&virtual_out), labels_out ? &labels_out : nullptr, empty_value));
    virtual_depth_.resize(px);
    for (size_t i = 0; i < px; i++)
      virtual_depth_[i] = is_16uc1 ? (float)static_cast<const uint16_t*>(virtual_out)[i] * 0.001f : static_cast<const float*>(virtual_out)[i];
    if (labels_out) labels_.assign(labels_out, labels_out + px);
    return true;
  }
  // the virtual depth plane of the last render_into (width x height metres, row 0 first; empty before the first)
  const std::vector<float>& getVirtualDepth() const { return virtual_depth_; }

  // Filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS): the pixels filter_into would keep as XYZ points in the
  // camera's optical frame, with the intrinsics of the last getProjectionMatrix (own_calibration rounded to float with
  // use_own_calibration, as the projection takes it, else the CameraInfo's fx fy cx cy as doubles).  depth: width x height
  // float metres, or uint16 millimetres with is_16uc1; the width must be a multiple of 4.  count_out == nullptr: the organized form, points_out width x height x 3 floats, NaN where there is no
  // point.  count_out != nullptr: the compacted form in row-major order, points_out capacity x 3 floats, index_out nullptr or
  // capacity words (v * width + u), *count_out the full number of kept pixels; entries from min(*count_out, capacity) on are
  // not written.
  bool cloud_into(const void* depth, bool is_16uc1, double* glTf, int width, int height, double timestamp, float* points_out,
                  uint32_t* index_out = nullptr, uint32_t* count_out = nullptr, int capacity = 0)
  {
    prepare(width, height);
    if (!depth || !points_out) throw std::runtime_error("cloud_into: needs depth and points_out");
    if (!have_cloud_intr_) throw std::runtime_error("cloud_into: no intrinsics yet (getProjectionMatrix sets them)");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    send_cloud_intrinsics();
    const void* in = depth;
    if (!count_out) {
      if (is_16uc1) check(rtuf_cloud_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), &points_out));
      else check(rtuf_cloud_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in), &points_out));
    } else if (is_16uc1) {
      check(rtuf_cloud_compact_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), &points_out, index_out ? &index_out : nullptr, count_out, capacity));
    } else {
      check(rtuf_cloud_compact_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in), &points_out, index_out ? &index_out : nullptr, count_out, capacity));
    }
    return true;
  }

  // Point list batches (include/rtuf.h, POINT LIST BATCHES): a point list instead of a depth image -- a lidar's points, a cloud
  // that was cropped or transformed, the compacted output of cloud_into -- for the camera and link poses filter_into would use
  // and the intrinsics cloud_into would use.  points: count x 3 floats in the camera's optical frame; radius_px 0 .. 4 widens
  // the robot by that many pixels.  verdict_out: count bytes (0 kept, 1 filtered, 2 outside the image or without a positive
  // finite z); pixel_out: nullptr or count words (v * width + u, 0xFFFFFFFF where the verdict is 2); summary_out: nullptr or
  // four words (kept, filtered, outside, count).
  bool points_into(const float* points, uint32_t count, double* glTf, int width, int height, double timestamp, uint8_t* verdict_out,
                   uint32_t* pixel_out = nullptr, uint32_t* summary_out = nullptr, int radius_px = 0)
  {
    prepare(width, height);
    if (!points || !verdict_out) throw std::runtime_error("points_into: needs points and verdict_out");
    if (!have_cloud_intr_) throw std::runtime_error("points_into: no intrinsics yet (getProjectionMatrix sets them)");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    send_cloud_intrinsics();
    check(rtuf_points_batch(ctx_, 1, &points, &count, radius_px, &verdict_out, pixel_out ? &pixel_out : nullptr, summary_out));
    return true;
  }

  // Link residual tables (include/rtuf.h, LINK RESIDUAL TABLES): per link label, how the sensor image compares with the model
  // for the camera and link poses filter_into would use.  depth: width x height float metres, or uint16 millimetres with
  // is_16uc1; table_out: n_labels rows, at least numLinkResidualRows(); row = label (linkLabels() with
  // FilterParameters::link_labels, else 1 + the renderable's index over all models; row 0: no link).  No plane is written.
  bool link_residuals_into(const void* depth, bool is_16uc1, double* glTf, int width, int height, double timestamp, rtuf_link_residuals* table_out,
                           int n_labels)
  {
    prepare(width, height);
    if (!depth || !table_out) throw std::runtime_error("link_residuals_into: needs depth and table_out");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    const void* in = depth;
    if (is_16uc1 && (width_ & 3) != 0) {
      // (the 16UC1 kernels need a width that is a multiple of 4: the reference's conversion on the host, as filter_into does)
      const size_t px = (size_t)width_ * height_;
      scratch_in_.resize(px);
      for (size_t i = 0; i < px; i++) scratch_in_[i] = (float)static_cast<const uint16_t*>(depth)[i] * 0.001f;
      const float* fin = scratch_in_.data();
      check(rtuf_link_residuals_batch(ctx_, 1, &fin, table_out, n_labels));
    } else if (is_16uc1) {
      check(rtuf_link_residuals_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), table_out, n_labels));
    } else {
      check(rtuf_link_residuals_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in), table_out, n_labels));
    }
    return true;
  }
  // Link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES): per link label, the nearest kept point to the spheres of
  // setLinkSpheres (link = renderable index within the model, centres in the renderable's frame: a draw's pre_op applied to its vertices first), for the camera, link poses and intrinsics cloud_into would use.  depth: width x height float metres, or
  // uint16 millimetres with is_16uc1 (any width); table_out: n_labels rows, row = label as in link_residuals_into, row 0 = the
  // whole robot.  No plane is written.
  void setLinkSpheres(int model, const std::vector<int32_t>& link, const std::vector<float>& xyzr)
  {
    if (xyzr.size() != 4 * link.size()) throw std::runtime_error("setLinkSpheres: xyzr must hold four floats per sphere");
    link_spheres_[model] = std::make_pair(link, xyzr);
    spheres_sent_ = false;
  }
  bool clearance_into(const void* depth, bool is_16uc1, double* glTf, int width, int height, double timestamp, rtuf_link_clearance* table_out,
                      int n_labels, float max_distance)
  {
    prepare(width, height);
    if (!depth || !table_out) throw std::runtime_error("clearance_into: needs depth and table_out");
    if (!have_cloud_intr_) throw std::runtime_error("clearance_into: no intrinsics yet (getProjectionMatrix sets them)");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    send_cloud_intrinsics();
    if (!spheres_sent_) {
      for (const auto& kv : link_spheres_)
        check(rtuf_set_link_spheres(ctx_, kv.first, kv.second.first.data(), kv.second.second.data(), (int)kv.second.first.size()));
      spheres_sent_ = true;
    }
    const void* in = depth;
    if (is_16uc1) check(rtuf_link_clearance_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), table_out, n_labels, max_distance));
    else check(rtuf_link_clearance_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in), table_out, n_labels, max_distance));
    return true;
  }
  // ---- voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS) ----
  // One world grid that voxel_insert accumulates kept points in: origin and voxel_size in metres, dims = (nx, ny, nz),
  // world_from_optical nullptr or the camera's column-major 4 x 4 matrix.  The grid belongs to the device context: a new image
  // size makes a new, empty one.
  void setVoxelGrid(const double origin[3], double voxel_size, const int dims[3], bool with_counts = true, const double* world_from_optical = nullptr)
  {
    std::memcpy(voxel_origin_, origin, sizeof voxel_origin_);
    std::memcpy(voxel_dims_, dims, sizeof voxel_dims_);
    voxel_size_ = voxel_size; voxel_counts_ = with_counts; voxel_has_tf_ = world_from_optical != nullptr;
    if (world_from_optical) std::memcpy(voxel_tf_, world_from_optical, sizeof voxel_tf_);
    have_voxel_ = true; voxel_sent_ = false;
  }
  // Inserts the pixels filter_into would keep -- dilation, thresholds, padding and scene honoured -- for the camera and link
  // poses filter_into would use and the intrinsics cloud_into would use.  depth: width x height float metres, or uint16
  // millimetres with is_16uc1; the width must be a multiple of 4.  summary_out: nullptr or four words (inserted, outside the
  // grid, not kept, total).
  bool voxel_insert(const void* depth, bool is_16uc1, double* glTf, int width, int height, double timestamp, uint32_t* summary_out = nullptr)
  {
    prepare(width, height);
    if (!depth) throw std::runtime_error("voxel_insert: needs depth");
    if (!have_cloud_intr_) throw std::runtime_error("voxel_insert: no intrinsics yet (getProjectionMatrix sets them)");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    send_cloud_intrinsics();
    send_voxel_grid();
    const void* in = depth;
    if (is_16uc1) check(rtuf_voxel_insert_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), summary_out));
    else check(rtuf_voxel_insert_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in), summary_out));
    return true;
  }
  void voxelClear() { if (ctx_ && voxel_sent_) check(rtuf_voxel_clear(ctx_)); }
  // bits_out: ceil(nx * ny * nz / 32) words; counts_out: nullptr or nx * ny * nz words.  false before the first insert.
  bool getVoxelGrid(uint32_t* bits_out, uint32_t* counts_out = nullptr)
  {
    if (!ctx_ || !voxel_sent_) return false;
    check(rtuf_get_voxel_grid(ctx_, bits_out, counts_out));
    return true;
  }

  // ---- voxel free space (include/rtuf.h, VOXEL FREE SPACE) ----
  // Marks the voxels of setVoxelGrid's grid that the camera sees THROUGH: whose centre lies more than `margin` metres in front
  // of the smallest valid reading within radius_px pixels of its pixel, with the intrinsics cloud_into would use.  The mask is
  // not read, no model is posed and glTf is not read.  depth: width x height float metres, or uint16 millimetres with is_16uc1;
  // any width.  summary_out: nullptr or four words (free, not free, not seen, nx * ny * nz).
  bool voxel_carve(const void* depth, bool is_16uc1, const double* glTf, int width, int height, double margin, int radius_px = 0, uint32_t* summary_out = nullptr)
  {
    (void)glTf;
    prepare(width, height);
    if (!depth) throw std::runtime_error("voxel_carve: needs depth");
    if (!have_cloud_intr_) throw std::runtime_error("voxel_carve: no intrinsics yet (getProjectionMatrix sets them)");
    if (renderers_.empty()) return false;
    send_cloud_intrinsics();
    send_voxel_grid();
    const void* in = depth;
    if (is_16uc1) check(rtuf_voxel_carve_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), margin, radius_px, summary_out));
    else check(rtuf_voxel_carve_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in), margin, radius_px, summary_out));
    return true;
  }
  // free_bits: ceil(nx * ny * nz / 32) words; occupied wins over free, a voxel with neither bit is unknown.  false before the
  // first insert or carve.
  bool getVoxelFree(uint32_t* free_bits)
  {
    if (!ctx_ || !voxel_sent_) return false;
    check(rtuf_get_voxel_free(ctx_, free_bits));
    return true;
  }

  // ---- scene planes (include/rtuf.h, SCENE PLANES) ----
  // Lowers the scene plane to the readings of every pixel the robot filter keeps, for the camera and link poses filter_into
  // would use: call it for a few frames of the empty cell while the robot moves, with link padding in the model entries so
  // that the arm's halo is not learned.  Returns false when the camera transform is not available (nothing was learned).
  bool learnScene(const void* depth, bool is_16uc1, double* glTf, int width, int height, double timestamp = 0.0)
  {
    prepare(width, height);
    if (!depth) throw std::runtime_error("learnScene: needs depth");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    const void* in = depth;
    if (is_16uc1) check(rtuf_learn_scene_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in)));
    else check(rtuf_learn_scene_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in)));
    return true;
  }
  // The scene plane: width x height floats in metres, +inf or NaN where unknown (a context of another size is replaced, as by
  // filter()).
  void setScene(const float* plane, int width, int height)
  {
    prepare(width, height);
    check(rtuf_set_scene_planes(ctx_, 0, 1, &plane));
  }
  // false before the first frame (no context yet: nothing is written)
  bool getScene(float* plane_out)
  {
    if (!ctx_) return false;
    check(rtuf_get_scene_planes(ctx_, 0, 1, &plane_out));
    return true;
  }
  // the plane back to unknown; the parameters' margins stay in force for the next scene
  void clearScene()
  {
    if (!ctx_) return;
    check(rtuf_clear_scene(ctx_, 0, 1));
    enable_scene();
  }

  // rows a link_residuals_into table needs: one more than the largest label in effect (0 before the models are loaded)
  int numLinkResidualRows() const
  {
    if (want_labels_) {
      int largest = 0;
      for (const auto& kv : link_labels_) largest = std::max(largest, (int)kv.second);
      return largest + 1;
    }
    size_t n = 0;
    for (const URDFRenderer* rd : renderers_) n += rd->renderables_.size();
    return (int)n + 1;
  }

  // filter_into with the link label plane as well (labels_out: width x height uint16; needs FilterParameters::link_labels and
  // a masked_out).  The plane is also kept for getLabels().
  bool filter_into(const void* depth, bool is_16uc1, double* glTf, int width, int height, double timestamp, void* masked_out, uint8_t* mask_out,
                   uint16_t* labels_out)
  {
    prepare(width, height);
    if (!want_labels_ || !masked_out || !labels_out) throw std::runtime_error("filter_into with labels: needs FilterParameters::link_labels and masked_out");
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    const size_t px = (size_t)width_ * height_;
    const void* in = depth;
    if (is_16uc1 && (width_ & 3) != 0) {
      // (the 16UC1 kernels need a width that is a multiple of 4: the reference's two conversions on the host, as filter_into does)
      scratch_in_.resize(px);
      scratch_out_.resize(px);
      for (size_t i = 0; i < px; i++) scratch_in_[i] = (float)static_cast<const uint16_t*>(depth)[i] * 0.001f;
      const float* fin = scratch_in_.data();
      float* fout = scratch_out_.data();
      check(rtuf_filter_batch_labels(ctx_, 1, &fin, &fout, mask_out ? &mask_out : nullptr, &labels_out));
      uint16_t* o = static_cast<uint16_t*>(masked_out);
      for (size_t i = 0; i < px; i++) {
        const float v = fout[i] * 1000.0f;
        long q = 0;
        if (v >= -2147483648.0f && v < 2147483648.0f) q = std::lrintf(v);
        o[i] = (uint16_t)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
      }
    } else if (is_16uc1) {
      check(rtuf_filter_batch_u16_labels(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), reinterpret_cast<uint16_t* const*>(&masked_out),
                                         mask_out ? &mask_out : nullptr, &labels_out));
    } else {
      check(rtuf_filter_batch_labels(ctx_, 1, reinterpret_cast<const float* const*>(&in), reinterpret_cast<float* const*>(&masked_out),
                                     mask_out ? &mask_out : nullptr, &labels_out));
    }
    labels_.assign(labels_out, labels_out + px);
    return true;
  }

  // ---- beyond the reference's surface: what a ROS adapter needs to leave the CPU out of the pixel path ----------------
  // The reference converts 16UC1 <-> 32FC1 with cv::Mat::convertTo around filter() (src/urdf_filter.cpp:280-289, :308-312);
  // here the frame goes to the GPU in the encoding it arrived in and the outputs land in the caller's buffers (e.g. the
  // data vectors of the messages to publish).  Either output may be null.  Returns false when the camera transform is not
  // available yet (nothing was written; the reference's quirk Q6 keeps the previous frame instead).
  bool filter_into(const void* depth, bool is_16uc1, double* glTf, int width, int height, double timestamp, void* masked_out, uint8_t* mask_out)
  {
    prepare(width, height);
    if (renderers_.empty() || !stage_frame(glTf, timestamp)) return false;
    if ((width_ & 3) != 0 && (is_16uc1 || !masked_out)) {
      // The fused 16UC1 kernels and the bit-packed mask need a width that is a multiple of 4.  Any other camera goes through
      // the full 32FC1 planes, with the reference's own two conversions (src/urdf_filter.cpp:287-288, :309-312: convertTo
      // 0.001 / 1000.0, round half to even, saturated) done here on the host -- slower, and right for every width.
      const size_t px = (size_t)width_ * height_;
      scratch_in_.resize(is_16uc1 ? px : 0);
      scratch_out_.resize(px);
      const float* in = static_cast<const float*>(depth);
      if (is_16uc1) {
        const uint16_t* u = static_cast<const uint16_t*>(depth);
        for (size_t i = 0; i < px; i++) scratch_in_[i] = (float)u[i] * 0.001f;
        in = scratch_in_.data();
      }
      float* out = (masked_out && !is_16uc1) ? static_cast<float*>(masked_out) : scratch_out_.data();
      check(rtuf_filter_batch(ctx_, 1, &in, &out, mask_out ? &mask_out : nullptr));
      if (masked_out && is_16uc1) {
        uint16_t* o = static_cast<uint16_t*>(masked_out);
        for (size_t i = 0; i < px; i++) {
          const float v = out[i] * 1000.0f;
          long q = 0;
          if (v >= -2147483648.0f && v < 2147483648.0f) q = std::lrintf(v);
          o[i] = (uint16_t)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
        }
      }
      return true;
    }
    if (!masked_out) {
      // mask only: one bit per pixel comes back over the bus (rtuf_filter_batch_bits*), expanded here
      bits_.resize(rtuf_mask_bits_words(width_, height_));
      uint32_t* bits = bits_.data();
      const void* in = depth;
      check(is_16uc1 ? rtuf_filter_batch_bits_u16_async(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), &bits)
                     : rtuf_filter_batch_bits_async(ctx_, 1, reinterpret_cast<const float* const*>(&in), &bits));
      check(rtuf_sync(ctx_));
      if (mask_out) check(rtuf_expand_mask_bits(depth, is_16uc1 ? 1 : 0, bits, width_, height_, (float)filter_replace_value_, nullptr, mask_out));
      return true;
    }
    const void* in = depth;
    check(is_16uc1 ? rtuf_filter_batch_u16(ctx_, 1, reinterpret_cast<const uint16_t* const*>(&in), reinterpret_cast<uint16_t* const*>(&masked_out), mask_out ? &mask_out : nullptr)
                   : rtuf_filter_batch(ctx_, 1, reinterpret_cast<const float* const*>(&in), reinterpret_cast<float* const*>(&masked_out), mask_out ? &mask_out : nullptr));
    return true;
  }

 private:
  void prepare(int width, int height)
  {
    if (width_ == width && height_ == height) return;
    width_ = width;
    height_ = height;
    this->initGL();
  }
  // camera + link poses + uniforms of one frame (the part of render() before the draw calls, src/urdf_filter.cpp:576-632)
  bool stage_frame(const double* camera_projection_matrix, double timestamp)
  {
    Transform camera_transform;
    if (!tf_.lookup(cam_frame_, fixed_frame_, camera_transform)) {
      std::fprintf(stderr, "[realtime_urdf_filter] no transform %s <- %s\n", cam_frame_.c_str(), fixed_frame_.c_str());
      return false;                               // outputs keep the previous frame (quirk Q6)
    }
    double off[16], cam[16];
    const Transform offset = Transform::from_quaternion({params_.camera_offset_rotation[0], params_.camera_offset_rotation[1], params_.camera_offset_rotation[2], params_.camera_offset_rotation[3]},
                                                        {params_.camera_offset_translation[0], params_.camera_offset_translation[1], params_.camera_offset_translation[2]});
    offset.inverse().opengl_matrix(off);
    const Transform rot = Transform::from_quaternion(camera_transform.rotation());
    const rtuf_host::Vec3 right = rot.apply({1, 0, 0}), down = rot.apply({0, 1, 0});
    camera_transform.o.x += right.x * camera_tx_; camera_transform.o.y += right.y * camera_tx_; camera_transform.o.z += right.z * camera_tx_;
    camera_transform.o.x += down.x * camera_ty_; camera_transform.o.y += down.y * camera_ty_; camera_transform.o.z += down.z * camera_ty_;
    camera_transform.opengl_matrix(cam);
    check(rtuf_set_camera(ctx_, 0, camera_projection_matrix, off, cam));
    if (padded_) {                                  // link padding projects its margins with the stream's focal lengths
      if (!have_cloud_intr_) throw std::runtime_error("link padding: no intrinsics yet (getProjectionMatrix sets them)");
      send_cloud_intrinsics();
    }
    for (size_t i = 0; i < renderers_.size(); i++) {
      URDFRenderer* rd = renderers_[i];
      rd->update_link_transforms(timestamp);
      std::vector<double> tf(16 * rd->renderables_.size());
      for (size_t k = 0; k < rd->renderables_.size(); k++) rd->renderables_[k]->gl_matrix(&tf[16 * k]);
      if (!tf.empty()) check(rtuf_set_link_poses(ctx_, 0, model_ids_[i], tf.data(), (int)rd->renderables_.size()));
    }
    {
      // the thresholds are public members the reference re-reads every frame (uniform upload, :630-631)
      rtuf_params p;
      rtuf_default_params(&p);
      p.near_plane = (float)near_plane_;
      p.far_plane = (float)far_plane_;
      p.depth_distance_threshold = (float)depth_distance_threshold_;
      p.filter_replace_value = (float)filter_replace_value_;
      p.silhouette_dilation_px = silhouette_dilation_px_;
      check(rtuf_set_params(ctx_, &p));
      // per-link thresholds: the links of such a model without a value of their own follow the global one
      if (depth_distance_threshold_ != applied_threshold_) { applied_threshold_ = depth_distance_threshold_; apply_link_thresholds(); }
    }
    return true;
  }

 public:
  // copy char buffer to the device (src/urdf_filter.cpp:332-353): deferred to render(), which uploads
  void textureBufferFromDepthBuffer(unsigned char* buffer, int /*size_in_bytes*/) { pending_buffer_ = buffer; }

  const float* getMaskedDepth() { return masked_depth_; }

 public:
  const TransformProvider& tf_;
  std::vector<URDFRenderer*> renderers_;
  // parameters from launch file
  std::string fixed_frame_, cam_frame_;
  bool show_gui_;
  bool need_mask_ = true;
  int width_ = 0, height_ = 0;
  double camera_tx_ = 0, camera_ty_ = 0;
  double far_plane_ = 8, near_plane_ = 0.1;        // src/urdf_filter.cpp:53-54
  double depth_distance_threshold_, filter_replace_value_;
  unsigned silhouette_dilation_px_;                // re-read every frame like the thresholds
  // output from rendering (library-owned, valid until the next filter())
  const float* masked_depth_ = nullptr;
  const uint8_t* mask_ = nullptr;

 private:
  void check(int rc)
  {
    if (rc < 0) throw std::runtime_error(std::string("rtuf: ") + rtuf_last_error(ctx_));
  }
  FilterParameters params_;
  std::map<std::string, std::string> param_server_;
  int device_;
  MeshResolver resolve_;
  void* resolve_user_;
  rtuf_context* ctx_ = nullptr;
  std::vector<int> model_ids_;
  unsigned char* pending_buffer_ = nullptr;
  std::vector<uint32_t> bits_;
  std::vector<float> scratch_in_, scratch_out_;      // filter_into for widths that are not a multiple of 4
  // per-link depth thresholds (ModelParameter::link_depth_distance_thresholds): every renderable of a listed URDF link takes
  // its value, the model's other links the global threshold it was last applied with
  void apply_link_thresholds()
  {
    for (size_t i = 0; i < renderers_.size(); i++) {
      const URDFRenderer* rd = renderers_[i];
      if (rd->link_thresholds.empty() || rd->renderables_.empty()) continue;
      std::vector<float> t;
      for (const auto& r : rd->renderables_) {
        auto it = rd->link_thresholds.find(r->urdf_link);
        t.push_back((float)(it != rd->link_thresholds.end() ? it->second : applied_threshold_));
      }
      check(rtuf_set_link_thresholds(ctx_, model_ids_[i], t.data(), (int)t.size()));
    }
  }
  double applied_threshold_ = 0.0;                   // the global threshold apply_link_thresholds last used
  // scene filtering with the parameters' margins (a new context's plane is all unknown: nothing is filtered until a scene is
  // learned or set)
  void enable_scene()
  {
    if (params_.scene_margin < 0.0) return;
    const float abs_rel[2] = {(float)params_.scene_margin, (float)params_.scene_margin_rel};
    check(rtuf_set_scene_margins(ctx_, 0, 1, abs_rel));
  }
  // the context gets the intrinsics of the last getProjectionMatrix, when it has not got them yet
  void send_cloud_intrinsics()
  {
    if (cloud_intr_sent_ && std::memcmp(cloud_intr_given_, cloud_intr_, sizeof cloud_intr_) == 0) return;
    check(rtuf_set_cloud_intrinsics(ctx_, 0, 1, cloud_intr_));
    cloud_intr_sent_ = true;
    std::memcpy(cloud_intr_given_, cloud_intr_, sizeof cloud_intr_);
  }
  bool padded_ = false;                              // some model entry gave a link a padding (initGL)
  bool want_labels_;                                 // FilterParameters::link_labels
  std::vector<uint16_t> labels_;                     // label plane of the last frame (getLabels)
  std::vector<float> virtual_depth_;                 // virtual depth plane of the last render_into (getVirtualDepth)
  double cloud_intr_[4] = {0, 0, 0, 0};              // fx fy cx cy of the last getProjectionMatrix (cloud_into)
  double cloud_intr_given_[4] = {0, 0, 0, 0};        // ... and what the context was last given
  bool have_cloud_intr_ = false;
  std::map<int, std::pair<std::vector<int32_t>, std::vector<float>>> link_spheres_;      // setLinkSpheres: per model, link and xyzr of every sphere
  bool spheres_sent_ = false;                        // ctx_ holds link_spheres_ (cleared whenever initGL makes a new context)
  bool cloud_intr_sent_ = false;                     // ctx_ holds cloud_intr_given_ (cleared whenever initGL makes a new context)
  // the context gets the grid of setVoxelGrid, when it has not got it yet
  void send_voxel_grid()
  {
    if (!have_voxel_) throw std::runtime_error("no voxel grid yet (setVoxelGrid)");
    if (voxel_sent_) return;
    check(rtuf_set_voxel_grid(ctx_, voxel_origin_, voxel_size_, voxel_dims_, voxel_counts_ ? 1 : 0));
    check(rtuf_set_voxel_transforms(ctx_, 0, 1, voxel_has_tf_ ? voxel_tf_ : nullptr));
    voxel_sent_ = true;
  }
  double voxel_origin_[3] = {0, 0, 0}, voxel_size_ = 0.0, voxel_tf_[16] = {};      // setVoxelGrid
  int voxel_dims_[3] = {0, 0, 0};
  bool have_voxel_ = false, voxel_counts_ = false, voxel_has_tf_ = false;
  bool voxel_sent_ = false;                          // ctx_ holds the grid (cleared whenever initGL makes a new context)
  std::map<std::pair<int, std::string>, uint16_t> link_labels_;
  std::vector<float> own_masked_;                    // render() with labels: the outputs the library-owned planes hold otherwise
  std::vector<uint8_t> own_mask_;
};

}  // namespace realtime_urdf_filter
