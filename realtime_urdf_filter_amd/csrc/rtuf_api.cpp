// rtuf_api.cpp -- host side of the C ABI declared in include/rtuf.h.
//
// Owns device memory, uploads geometry once, stages per-frame poses, and enqueues the
// kernels of rtuf_kernels.hip on one HIP stream per context.  There is no CPU compute
// path in this library: without a HIP device rtuf_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "rtuf.h"
#include "rtuf_device.h"
#include "rtuf_groups.h"
#include "rtuf_numerics.h"
#include "rtuf_routes.h"


using namespace rtuf;

namespace {

struct HostDraw {
  int pre_op;
  float op[3];
  std::vector<float> verts;       // xyz
  std::vector<uint32_t> tris;     // 3 per triangle, local vertex ids
};
struct HostLink { std::vector<HostDraw> draws; };
static constexpr int kMaxInflight = 2;      // device batches that may be in flight at once
#ifndef RTUF_MAX_LANES
#define RTUF_MAX_LANES 3            // (an experiment's build may raise it: more lanes than the runtime has hardware queues -- GPU_MAX_HW_QUEUES, 4 by default -- share queues)
#endif
static constexpr int kMaxLanes = RTUF_MAX_LANES;         // raster lanes a context can have (rtuf_params.raster_lanes; the default is kDefaultLanes)
static constexpr int kDefaultLanes = 3;     // (three lanes + the pose stage's stream = the HIP runtime's four hardware queues)

struct Kinematics {               // on-device forward kinematics of one model
  int n_frames = 0, camera_frame = -1, max_depth = 0;
  int32_t* d_depth = nullptr;
  bool has_root = false, any_enabled = false;
  bool dirty_q = true, dirty_aux = true;     // joint positions / root poses + enable flags changed on the host
  int32_t* d_parent = nullptr; int32_t* d_type = nullptr; double* d_origin = nullptr; double* d_axis = nullptr;
  int32_t* d_link_frame = nullptr; double* d_link_offset = nullptr;
  // joint positions are staged in a ring of pinned buffers that the forward-kinematics kernel reads in
  // place (zero-copy): every batch in flight owns the buffer it was enqueued with, rtuf_set_joint_positions
  // writes h_q[q_write], so the next frame's joint states can be staged while the GPU filters
  double* h_q[kMaxInflight + 1] = {};                      // [max_streams][n_frames]
  int q_live = 0, q_write = 0;
  int aux_uploaded_streams = 0;
  bool q_carried = true;                                    // h_q[q_write] holds everything h_q[q_live] does
  double* h_root = nullptr; double* d_root = nullptr;       // [max_streams][12]
  uint8_t* h_enabled = nullptr; uint8_t* d_enabled = nullptr;
};
// labels: rtuf_set_link_labels's labels of the model's links (empty: the default, 1 + link_base + link)
// thresholds: rtuf_set_link_thresholds's depth thresholds of the model's links (empty: rtuf_params.depth_distance_threshold)
// sph_link / sph_xyzr: rtuf_set_link_spheres's list of the model (the link and x, y, z, r of every sphere)
// padding: rtuf_set_link_padding's margins of the model's links in metres (empty: none)
struct HostModel { std::vector<HostLink> links; int link_base = 0; Kinematics kin; std::vector<uint16_t> labels; std::vector<float> thresholds;
                   std::vector<int32_t> sph_link; std::vector<float> sph_xyzr; std::vector<float> padding; };

// One batch as its caller asked for it: the kind, and the device buffers and scalars that kind has (the rest stays nullptr / 0).
// A slot keeps the record of its batch (Batch::rq) for re-runs; which kernels a kind runs is route_of's to say (rtuf_routes.h).
struct BatchRequest {
  using Kind = BatchKind;
  Kind kind; int n; bool u16;               // (u16: the sensor / masked / virtual planes are 16UC1)
  bool robot_only = false;                  // rtuf_learn_scene_batch*'s mask-bits batch: the robot's bits alone, whatever scene is in effect
  bool wait_upload = false;                 // host planes: the lanes wait for the slot's `uploaded` event before the first kernel that reads them
  const float* depth = nullptr;             // sensor planes (every kind but Render)
  float* masked = nullptr; uint8_t* mask = nullptr;      // Filter (mask may be nullptr)
  uint16_t* labels = nullptr;               // Filter, Render: the link label plane, or nullptr
  uint32_t* bits = nullptr;                 // Bits: the mask-only output, 1 bit per pixel; Cloud: the slot's own cl_bits
  float* virt = nullptr; float empty_value = 0.0f;       // Render: the virtual depth plane (float, or uint16 with u16) and the value of its empty pixels
  rtuf_link_residuals* resid = nullptr; int n_labels = 0;      // Residual: the table [n][n_labels] the tile kernel sums into, zeroed on every run, re-runs included
  // Cloud (a mask-bits batch with the cloud kernels behind it).  capacity == 0: the organized form, index and counts unused; index may be nullptr anyway
  float* points = nullptr; uint32_t* index = nullptr; uint32_t* counts = nullptr; int capacity = 0;
  // Clearance (a mask-bits batch with the clearance kernels behind it): the table [n][n_labels] and the cutoff
  rtuf_link_clearance* clr = nullptr; float max_distance = 0.0f;
  // Points (a render batch into the slot's own plane -- virt, set by submit_batch -- with the points kernel behind it): the point
  // lists [n][capacity][3] with their device counts [n] (capacity: the field above), the window radius, and the outputs:
  // verdict [n][capacity], pixel [n][capacity] or nullptr, summary [n][4] or nullptr
  const float* pt_points = nullptr; const uint32_t* pt_counts = nullptr; int pt_radius = 0;
  uint8_t* pt_verdict = nullptr; uint32_t* pt_pixel = nullptr; uint32_t* pt_summary = nullptr;
  BatchRequest(Kind k = Kind::Filter, int n_ = 0, bool u16_ = false) : kind(k), n(n_), u16(u16_) {}
};
using Kind = BatchRequest::Kind;

char g_create_error[512] = "";

constexpr uint32_t kKnownFlags = RTUF_FLAG_TWO_KERNEL | RTUF_FLAG_STRICT_GRID;
static bool dilation_valid(const rtuf_params* p) { return p->silhouette_dilation_px <= (uint32_t)kMaxDilation; }
static_assert(kMaxLinkPaddingPx == RTUF_MAX_LINK_PADDING_PX, "the header's clamp is the kernels'");
inline bool flags_valid(uint32_t flags)
{
#ifdef RTUF_ABLATE
  (void)flags; return true;          // timing-experiment build: bits 8.. select what the kernels skip
#else
  return (flags & ~kKnownFlags) == 0u;
#endif
}

}  // namespace

struct rtuf_context {
  int device = 0;
  int width = 0, height = 0, tiles_x = 0, tiles_y = 0, max_streams = 0;
  rtuf_params params{};
  std::string error;

  // models (host)
  std::vector<HostModel> models;
  bool finalized = false;
  bool broken = false;                 // a bin regrowth failed half-way: the bins are gone, every later filter call fails
  int n_links = 0, n_draws = 0, n_chunks = 0;
  int key_shift = 3;                   // depth keys: draw order << key_shift (32 - the bits the context's draw orders need)
  int64_t n_tris = 0, n_cverts = 0;
  uint32_t bg_chunk = 0;

  // static geometry (device)
  float4* d_cverts = nullptr; uint32_t* d_ctris = nullptr; uint32_t* d_corder = nullptr; Chunk* d_chunks = nullptr; Draw* d_draws = nullptr;
  // Link labels (rtuf_filter_batch*_labels): every draw's global link and the last draw order it owns (draw orders are assigned
  // draw by draw, model -> link -> draw order), and the device table draw order -> label, [n_tris + 1] (entry 0 = 0).  The
  // table is allocated by the first label call or rtuf_set_link_labels and rewritten in place after that (captured graphs
  // keep its address); contexts that never ask for labels allocate nothing.
  std::vector<uint32_t> draw_link, draw_last_order;
  uint16_t* d_order_labels = nullptr;
  bool labels_dirty = true;
  uint32_t max_label = 0;                    // the largest label of any link (ensure_label_table): what a residual table's n_labels must exceed
  // Per-link depth thresholds: the device table draw order -> threshold, [n_tris + 1] (entry 0, the background quad: the
  // global threshold), allocated by the first rtuf_set_link_thresholds and rewritten in place after that (captured graphs
  // keep its address).  The tile kernels read it only while thresh_models > 0 (models with thresholds of their own).
  float* d_order_thr = nullptr;
  int thresh_models = 0;
  // Filtered point clouds: kx, ky, cx, cy of every stream, [max_streams], allocated by the first rtuf_set_cloud_intrinsics and
  // rewritten in place after that (captured graphs keep its address), and which streams have been given theirs.
  CloudIntrinsics* d_cloud_intr = nullptr;
  std::vector<uint8_t> cloud_intr_set;
  // Point list batches: fx, fy, cx, cy of every stream as floats, [max_streams], written beside d_cloud_intr by
  // rtuf_set_cloud_intrinsics, and the streams' optional transforms (rtuf_set_point_transforms; point_tf: the host's copy),
  // [max_streams], allocated by the first setter or batch that needs them and rewritten in place after that (captured graphs
  // keep their addresses).  d_pt_stage / pt_stage_bytes: the host form's grow-only staging (points, counts, verdicts, pixels,
  // summary: one block).
  PointIntrinsics* d_point_intr = nullptr;
  PointTransform* d_point_tf = nullptr;
  std::vector<PointTransform> point_tf;
  char* d_pt_stage = nullptr; size_t pt_stage_bytes = 0;
  // Link padding: the device tables draw order -> link slot, [n_tris + 1] (entry 0 = 0; a link's slot is 1 + its context-global
  // number), slot -> padding in metres, [n_links + 1] (entry 0 = 0), and stream -> (float)max(fx, fy), [max_streams], allocated
  // by the first rtuf_set_link_padding and rewritten in place after that (captured graphs keep their addresses).  The kernels
  // read them only while pad_models > 0 (models that hold a non-zero padding).  focal: the host's copy, kept since the first
  // rtuf_set_cloud_intrinsics.
  uint16_t* d_order_slot = nullptr; float* d_slot_pad = nullptr; float* d_pad_focal = nullptr;
  std::vector<float> focal;
  int pad_models = 0;
  // Link clearance tables: the spheres of every model sorted by label (label 0 left out) with their label slots, rebuilt on
  // the host when the lists or the labels changed (clr_dirty) and uploaded before the next clearance batch; the device
  // arrays are allocated once for the most a context can hold (captured graphs keep their addresses).
  std::vector<ClearanceSphere> clr_spheres;
  std::vector<uint32_t> clr_slot_label;
  ClearanceSphere* d_clr_spheres = nullptr; uint32_t* d_clr_slot_label = nullptr;
  bool clr_dirty = true;
  // Scene planes (include/rtuf.h, SCENE PLANES): one float plane per stream, [max_streams][H][W], +inf until set or learned, and
  // the streams' margins and switches (scene_streams: the host's copy), allocated by the first scene call that needs them and
  // rewritten in place after that (captured graphs keep their addresses).  The scene kernels run only while scene_enabled > 0
  // (streams with filtering enabled).  scene_touched: streams whose plane, margins or switch may differ from a fresh
  // context's; when rtuf_clear_scene clears the last of them everything here is returned.  d_scene_bits / d_scene_stage:
  // learning's scratch -- the robot's mask bits of a learn call, [max_streams] bits planes, and the sensor planes of a
  // host-plane learn call, [max_streams][H][W] floats.
  float* d_scene = nullptr; SceneStream* d_scene_streams = nullptr;
  std::vector<SceneStream> scene_streams;
  std::vector<uint8_t> scene_touched;
  int scene_enabled = 0;
  uint32_t* d_scene_bits = nullptr; float* d_scene_stage = nullptr;
  // Voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS): the grid as the kernels read it (vox_grid; nx = 0: none),
  // its bit words and optional counts (allocated in multiples of 16 bytes: voxel_clear_kernel's stores), the streams'
  // world_from_optical transforms (allocated by the first rtuf_set_voxel_transforms; vox_tf: the host's copy), and the inserts'
  // scratch, allocated by the first insert that needs it: the mask bits of a plane insert, [max_streams] bits planes, and one
  // block for the host forms -- the sensor planes, [max_streams][H][W] floats, with the summary [max_streams][4] behind them.
  // With several pipelines all of this lives in the first one.
  VoxelGrid vox_grid{};
  size_t vox_voxels = 0, vox_words = 0;
  float vox_size = 0.0f;      // (float)voxel_size: the voxel centres of a carve
  uint32_t* d_vox_bits = nullptr; uint32_t* d_vox_counts = nullptr;
  PointTransform* d_vox_tf = nullptr;
  std::vector<PointTransform> vox_tf;
  uint32_t* d_vox_mask_bits = nullptr; float* d_vox_stage = nullptr;
  // Voxel free space (include/rtuf.h, VOXEL FREE SPACE): the free words beside d_vox_bits (the same indexing and rounding;
  // allocated and zeroed by the first carve or read, freed with the grid), the host's optical_from_world inverses of vox_tf
  // (vox_inv, rebuilt by every rtuf_set_voxel_transforms; vox_inv_ok: the stream's matrix could be inverted) and their device
  // table, allocated by the first carve that finds a transform and freed with the grid.  Host carves share d_vox_stage.
  uint32_t* d_vox_free = nullptr;
  PointTransform* d_vox_inv = nullptr;
  std::vector<PointTransform> vox_inv;
  std::vector<uint8_t> vox_inv_ok;

  // per-frame pose staging
  // Cameras and link matrices are staged in a ring of kMaxInflight + 1 pinned sets, like the joint positions: every
  // batch in flight owns the set it was enqueued with (a bin regrowth re-reads it), the setters write into a set no
  // batch reads, so staging the next frame's TF-derived matrices never waits for the GPU.  h_cams / h_link_tf alias the
  // set being written.
  Camera* ring_cams[kMaxInflight + 1] = {};        // pinned [max_streams]
  double* ring_link_tf[kMaxInflight + 1] = {};     // pinned [max_streams][n_links][16]
  Camera* h_cams = nullptr;
  double* h_link_tf = nullptr;
  struct StageRing {                               // one per array: cameras and link matrices advance independently
    int live = 0, write = 0;                       // set of the newest batch / set the setters write
    bool written = false;                          // the write set has changes no batch has taken yet
    bool carried = true;                           // the write set holds everything the live set does
  } cam_ring, link_ring;
  uint64_t* h_model_mask = nullptr;    // pinned [max_streams]
  uint64_t* d_model_mask = nullptr;

  // Rasteriser working set.  A RASTER LANE is a HIP stream plus the arrays one launch group is rasterised through (tile
  // bins, clip list, many-tile list, work list); the launch groups of a batch alternate between the lanes, so group B's
  // set-up kernel runs under group A's tile kernel and every kernel's ramp, tail and launch gap is filled by the other
  // lane -- what two contexts of half the streams gave a caller by hand (509 k instead of 455 k frames/s on the 256-stream
  // VGA workload in round 3), now inside one context.  Three lanes by default: with the pose stage's stream that is one HIP
  // stream per hardware queue of the runtime's default four.  Kernels of one lane
  // are ordered by its stream, which is all the hand-over its arrays need; lanes share nothing that is written per group.
  struct Lane {
    hipStream_t stream = nullptr;
    PackedTri* d_bins = nullptr; BinHeader* d_bin_hdr = nullptr;
    Frag* d_fbins = nullptr; uint32_t* d_fbin_count = nullptr;
    ClipItem* d_clip_list = nullptr;
    float4* d_clip_spill = nullptr;
    BigRec* d_big_list = nullptr;                                // many-tile records (per counter shard), see bigrec_kernel
    WorkItem* d_items[kMaxInflight] = {};                        // the launch group's set-up work list (cull_kernel -> setup_kernel), one per
                                                                 // batch slot: the cull of a lane's first group runs in the batch's pose
                                                                 // stage, under the set-up kernel of the batch before it
    float* d_zsurface = nullptr;
    uint16_t* d_slots = nullptr;                                 // link padding: the link slot plane beside the z-surface, [G][H][W]
  };
  Lane lane[kMaxLanes];
  int n_lanes = 1;
  // (The lanes run free of each other.  Chaining the set-up kernels across the lanes, so that one group's set-up always
  // runs under the other group's tile kernel, was measured and is WORSE -- 426 k instead of 457 k frames/s at four groups,
  // 466 k instead of 478 k at two: both kernels are bound by VALU issue, and side by side the set-up kernel loses the
  // occupancy its latency hiding needs.  What the lanes buy is each kernel's ramp, tail and launch gap filled by the other
  // lane)
  bool lanes_share_queue = false;      // no stream was found that runs beside lane 0's: the lanes work, one after the other
  int next_lane = 0;                   // lane of the next batch that is not split
  int last_lane = 0;                   // lane of the newest batch's last group (debug read-back of the z-surface)
  int group = 0;                       // streams per launch group at most (= streams a lane's bins are sized for)
  int max_groups = 1;                  // counter blocks of a batch slot: launch groups of any batch up to max_streams at most
  uint32_t capacity = 0, fcapacity = 0, clip_capacity = 0;
  uint32_t big_capacity = 0;           // many-tile list, per counter shard
  uint32_t items_hint = 0; int items_hint_streams = 0;      // longest work list of the last batch's groups, and their size
  std::vector<uint32_t> group_items;   // work-list length of every launch group of the last retired batch ...
  std::vector<int> group_streams;      // ... and its streams: a group of the same index and size takes its own list length as the hint
  bool force_worst_grid = false;       // re-runs after a set-up grid that was too short: the worst-case grid, which cannot be
  size_t memory_budget = 0;            // upper bound of the lanes' tile bins (rtuf_params.memory_limit_mb or a third of the free memory)
  // every device allocation of the context goes through dev_alloc / dev_free: rtuf_stats.device_bytes is their sum
  std::unordered_map<void*, size_t> dev_blocks;
  size_t device_bytes = 0;

  // staging for the host-pointer API
  hipStream_t h2d = nullptr, d2h = nullptr;  // copy streams of the host-plane calls (rtuf_filter_batch*)
  std::vector<void*> pinned;                 // rtuf_host_alloc blocks not yet freed

  // single-stream outputs (masked_depth_ / mask_ of the reference)
  std::vector<float> single_masked; std::vector<uint8_t> single_mask;

  // Batches in flight.  Up to kMaxInflight device batches may be enqueued before the oldest is retired
  // (rtuf_sync, or the next rtuf_filter_batch_device* call when the ring is full), so the host round
  // trip of one batch overlaps the GPU work of the next.  A batch keeps what a re-run after a bin
  // regrowth needs: the request it was submitted with and which staging sets of the poses it read.
  struct Batch {
    bool active = false;
    BatchRequest rq;                         // what the caller asked for (submit_batch); every run of the batch reads it
    Route route{};                           // the kernels it runs (route_of, when it is first enqueued; kept for re-runs): the tile variant -- cover pass
                                             // and per-link thresholds among its fields -- and what runs behind the tile kernel
    // cloud batches: the slot's own bits buffer and row scratch ([2][max_streams][H]: row counts, row starts), allocated on the
    // slot's first (compacted) cloud batch for max_streams, so that captured graphs keep their addresses
    uint32_t* cl_bits = nullptr; uint32_t* cl_rows = nullptr;
    // point list batches: the virtual depth plane the slot's batch renders into and its points kernel reads, [max_streams][H][W]
    // float, allocated on the slot's first such batch (one per slot, not per lane: batches in flight keep planes of their own,
    // and the launch groups of a batch write disjoint streams of it)
    float* pt_plane = nullptr;
    // clearance batches: the posed spheres of the slot's batch, [max_streams][clr_posed_have], regrown when the context holds more spheres
    float4* clr_posed = nullptr; size_t clr_posed_have = 0;
    Counters* h_counters = nullptr;          // pinned [max_groups]: one block per launch group, filled by the copies that end the batch
    hipEvent_t done[kMaxLanes] = {};         // recorded on each lane after its copy
    uint32_t lanes_used = 0;                 // bit l: the batch has launch groups on lane l
    int n_groups = 0;                        // launch groups of the batch
    std::vector<hipEvent_t> events;          // stage timing
    std::vector<int> q_idx;                  // per model: joint-position staging buffer
    int cam_idx = 0, link_idx = 0;           // camera / link-matrix staging sets
    // The batch's pose stage (uploads, forward kinematics, matrix stacks, cull) runs on a side stream and
    // writes only buffers of its own slot, so it overlaps the raster kernels of the batch before it.
    Camera* d_cams = nullptr; double* d_link_tf = nullptr;
    float* d_mvp = nullptr; BgInfo* d_bg = nullptr;
    Counters* d_counters = nullptr;          // [max_groups]
    uint32_t* d_status = nullptr;            // the slot's status word (kStatus* in rtuf_device.h; rtuf_batch_status_device)
    bool dirty_cams = true, dirty_link_tf = true;
    int uploaded_streams = 0;
    hipEvent_t posed = nullptr;              // recorded on the side stream after the pose stage
    // small batches: captured launch sequences of this slot, keyed by the hash of the argument blocks they were
    // captured with (a slot meets a few recurring sets: the ring of joint-position buffers, the caller's output sets)
    static constexpr int kGraphs = 6;
    struct { uint64_t hash = 0; hipGraphExec_t exec = nullptr; } graphs[kGraphs];
    int graph_next = 0;
    std::vector<uint32_t> setup_grid;        // per launch group: work items its set-up launch covered (0xffffffff = the worst case)
    int dilation = 0;                        // Post::Dilate: the radius (set when the batch is first enqueued, kept for re-runs)
    int timing = 0;                          // event timing of this batch: 0 none, 1 every stage, 2 tile/compare kernel only
    // Host-plane batches (submit_host_planes): grow-only device staging of this slot (ensure_staging; `have` in the units its
    // user counts in: streams, table rows, floats, words), the caller's planes of an asynchronous download, and the events
    // that order upload -> kernels -> download across the copy streams.
    bool host_io = false;                    // the batch ends with a download on d2h (`downloaded`)
    enum { kStDepth, kStMasked, kStMask, kStBits, kStLabels, kStVirtual, kStTable, kStPoints, kStIndex, kStClearance, kStKinds };
    struct { char* p = nullptr; size_t have = 0; } st[kStKinds];      // (depth and virtual are float-sized: large enough for uint16 planes)
    uint32_t* st_counts = nullptr;           // compacted clouds: [max_streams], allocated once
    std::vector<void*> h_out, h_mask, h_labels;      // masked / bits / virtual planes; byte masks (any may be nullptr); label planes
    rtuf_link_residuals* h_table = nullptr;
    hipEvent_t uploaded = nullptr, downloaded = nullptr;
  };
  Batch batch[kMaxInflight];
  hipStream_t side = nullptr;                // pose stages (see Batch)
  hipEvent_t fork_ev = nullptr;              // graph capture: forks the side stream off the main stream
  bool side_used_plain = false;              // the side stream carries work that was enqueued outside a graph
  // Small batches of a context that is one of several pipelines replay a captured hipGraph (one launch call instead of
  // ~12 API calls: there the host's launch cost is the limit, and the pipelines provide the overlap between batches).
  // A single-pipeline context keeps plain launches: its pose stage runs on the side stream underneath the previous
  // batch's raster kernels, which a graph on the main stream would serialise (batch = 1: 75 us plain, 94 us as a graph).
  // Cleared when the runtime refuses stream capture / instantiation.
  bool graphs_ok = false;
  uint32_t graph_evictions = 0;              // captures of the current 64-batch window that replaced a live cache entry
  uint64_t graph_hits = 0, graph_misses = 0; // replays / captures: a caller that never repeats an argument set (fresh output buffers
                                             // every frame) would pay a capture + instantiate per batch -- then graphs are switched off
  // The cover pass (bigrec_kernel<0> + the cover-aware tile kernel) pays where triangles cover whole tiles -- walls, anything
  // close to the lens -- and costs 3 % where none do (a finely tessellated robot at arm's length).  It is an optimisation
  // only (the image is the same with and without), so the context switches it by what the batches show: three batches in a
  // row without a single cover tile turn it off, every 64th batch runs it again as a probe.
  bool cover_on = true;
  int cover_idle = 0, cover_sleep = 0;
  int oldest = 0;                            // ring index of the oldest batch in flight
  int pending = 0;                           // batches in flight

  // host staging areas changed since the last upload?
  bool dirty_mask = true;
  int mask_uploaded_streams = 0;
  int last_slot = 0;                         // slot of the most recently enqueued batch (debug read-back)

  // rtuf_params.pipelines > 1: this context is only a front; `kids` are complete contexts (own streams, bins, staging,
  // geometry copy) that the batches alternate between, so one batch's small / low-occupancy kernels (pose stage, cull,
  // clip, kernel tails) overlap another batch's set-up and tile kernels.  Every setter goes to all kids (state is
  // replicated), every filter call to the next kid in turn; `order` lists the kids of the batches in flight, oldest first.
  std::vector<rtuf_context*> kids;
  int next_kid = 0, last_kid = 0;
  std::deque<int> order;

  rtuf_stats stats{};
#ifdef RTUF_LANECOUNT
  unsigned long long lane_slots[kLaneLoops] = {}, lane_live[kLaneLoops] = {};      // of the last retired batch (instrumented build)
  unsigned long long lane_roles[kLaneRoleWords] = {};
#endif
  int timing = 0;            // 0 off, 1 every stage, 2 only around the tile (and compare) kernel, 3 = 2 on every fourth batch
  uint32_t timing_seq = 0;
  double acc_ms[6] = {0, 0, 0, 0, 0, 0};  // sums of ms_pose .. ms_total, ms_clip over the timed batches
  uint64_t acc_batches = 0;

  int fail(int code, const char* fmt, ...)
  {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    error = buf;
    return code;
  }
};

#define HIP_TRY(ctx, expr)                                                                 \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return (ctx)->fail(e_ == hipErrorOutOfMemory ? RTUF_ERR_OOM : RTUF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

template <typename T>
static hipError_t dev_alloc(rtuf_context* c, T** p, size_t bytes)
{
  void* q = nullptr;
  const hipError_t e = hipMalloc(&q, bytes ? bytes : 1);
  *p = e == hipSuccess ? static_cast<T*>(q) : nullptr;
  if (e == hipSuccess) { c->dev_blocks[q] = bytes; c->device_bytes += bytes; }
  return e;
}
template <typename T>
static void dev_free(rtuf_context* c, T*& p)
{
  if (!p) return;
  auto it = c->dev_blocks.find((void*)p);
  if (it != c->dev_blocks.end()) { c->device_bytes -= it->second; c->dev_blocks.erase(it); }
  (void)hipFree((void*)p);
  p = nullptr;
}

// Launch groups a batch of n streams is split into (rtuf_groups.h)
static int groups_for(const rtuf_context* c, int n) { return rtuf::groups_for(n, c->group, c->n_lanes); }

static void sync_lanes(rtuf_context* c)
{
  for (int l = 0; l < c->n_lanes; l++) if (c->lane[l].stream) (void)hipStreamSynchronize(c->lane[l].stream);
}

// A working buffer of the rasteriser is too small for the batch in flight (its contents are not needed: the batch is run
// again).  The new one is allocated BEFORE the old one is freed whenever both fit; when they do not, the old one goes first.
// On failure the buffer is gone (nullptr) and the caller decides: smaller launch groups, or give up.
template <typename T>
static hipError_t realloc_dev(rtuf_context* c, T*& buf, size_t new_bytes)
{
  T* fresh = nullptr;
  hipError_t e = dev_alloc(c, &fresh, new_bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    dev_free(c, buf);
    e = dev_alloc(c, &fresh, new_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
  } else {
    dev_free(c, buf);
  }
  buf = fresh;
  return hipSuccess;
}
template <typename T>
static int regrow(rtuf_context* c, T*& buf, size_t new_bytes, const char* what)
{
  const hipError_t e = realloc_dev(c, buf, new_bytes);
  if (e != hipSuccess) {
    c->broken = true;
    return c->fail(RTUF_ERR_OOM, "growing the %s to %zu bytes failed: %s", what, new_bytes, hipGetErrorString(e));
  }
  c->stats.regrowths++;
  return RTUF_OK;
}

static size_t lane_bins_bytes(const rtuf_context* c, int G, uint32_t cap, uint32_t fcap)
{
  return (size_t)G * (size_t)c->tiles_x * c->tiles_y * ((size_t)cap * sizeof(PackedTri) + (size_t)fcap * sizeof(Frag));
}

// The per-batch counter blocks (one per launch group): enough for the groups of every batch of 1 .. max_streams streams
// (rtuf_groups.h: a full batch can make fewer groups than a partial one).
static int alloc_counter_blocks(rtuf_context* c)
{
  c->max_groups = rtuf::counter_blocks_for(c->max_streams, c->group, c->n_lanes);
  for (auto& b : c->batch) {
    dev_free(c, b.d_counters);
    if (b.h_counters) { (void)hipHostFree(b.h_counters); b.h_counters = nullptr; }
    HIP_TRY(c, hipHostMalloc(&b.h_counters, sizeof(Counters) * (size_t)c->max_groups));
    HIP_TRY(c, dev_alloc(c, &b.d_counters, sizeof(Counters) * (size_t)c->max_groups));
    HIP_TRY(c, hipMemset(b.d_counters, 0, sizeof(Counters) * (size_t)c->max_groups));
  }
  return RTUF_OK;
}

// Bins sized from what the batch asked for: a quarter above the fullest record / fragment bin, in steps of 256 / 1024 entries
// (never smaller than they are).  One allocation holds what used to be sized for the worst tile any scene could have.
// When the larger bins do not fit -- the memory limit of the context, or what the device has left (a shared GPU, several
// pipelines, 720p with many streams) -- the LAUNCH GROUP shrinks instead: the same bytes then hold deeper bins for fewer
// streams, a batch is rasterised in more, smaller launches, and nothing fails.  Only when not even one stream's bins can
// be had the context is lost.
static int grow_bins(rtuf_context* c, uint32_t needed, uint32_t fneeded)
{
  auto round_up = [](uint64_t v, uint64_t q) { return (uint32_t)std::min<uint64_t>(((v + q - 1) / q) * q, 0x7fffffffu); };
  const uint32_t cap = std::max(c->capacity, needed > c->capacity ? round_up((uint64_t)needed + needed / 4, 256) : c->capacity);
  const uint32_t fcap = std::max(c->fcapacity, fneeded > c->fcapacity ? round_up((uint64_t)fneeded + fneeded / 4, 1024) : c->fcapacity);
  if (cap == c->capacity && fcap == c->fcapacity) return RTUF_OK;
  // what may be spent: the context's limit, and no more than the device can give once the present bins are returned
  size_t free_b = 0, total_b = 0;
  HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
  const size_t held = (size_t)c->n_lanes * lane_bins_bytes(c, c->group, c->capacity, c->fcapacity);
  // (the context's limit -- rtuf_params.memory_limit_mb, or the third of the free memory taken at rtuf_finalize_models -- and
  // never more than the device can give)
  const size_t budget = std::min((size_t)((double)(free_b + held) * 0.9), c->memory_budget);
  int G = c->group;
  while (G > 1 && (size_t)c->n_lanes * lane_bins_bytes(c, G, cap, fcap) > budget) G = (G + 1) / 2;
  c->stats.over_memory_limit = (size_t)c->n_lanes * lane_bins_bytes(c, G, cap, fcap) > c->memory_budget ? 1u : 0u;      // (set: G == 1 and one stream's bins alone exceed it; cleared otherwise)
  for (;;) {
    hipError_t e = hipSuccess;
    for (int l = 0; l < c->n_lanes && e == hipSuccess; l++) {
      rtuf_context::Lane& ln = c->lane[l];
      // (a smaller group with deeper bins may fit the allocation that is there)
      const size_t want = (size_t)G * c->tiles_x * c->tiles_y * (size_t)cap * sizeof(PackedTri);
      const size_t fwant = (size_t)G * c->tiles_x * c->tiles_y * (size_t)fcap * sizeof(Frag);
      auto have = [&](void* q) { auto it = c->dev_blocks.find(q); return (q && it != c->dev_blocks.end()) ? it->second : (size_t)0; };
      if (have(ln.d_bins) < want) e = realloc_dev(c, ln.d_bins, want);
      if (e == hipSuccess && have(ln.d_fbins) < fwant) e = realloc_dev(c, ln.d_fbins, fwant);
    }
    if (e == hipSuccess) break;
    if (G == 1) {
      c->broken = true;
      return c->fail(RTUF_ERR_OOM, "growing the tile bins to %u + %u entries failed even for launch groups of one stream: %s", cap, fcap, hipGetErrorString(e));
    }
    G = (G + 1) / 2;            // the device has less than it said: halve the launch group and try again
  }
  c->stats.regrowths++;
  c->capacity = cap;
  c->fcapacity = fcap;
  if (G != c->group) {
    c->group = G;
    c->items_hint = 0;
    const int rc = alloc_counter_blocks(c);
    if (rc != RTUF_OK) { c->broken = true; return rc; }
  }
  return RTUF_OK;
}

// Setters of single-buffered state (model selection, parameters, forward-kinematics root poses / enable flags) wait for
// the batches in flight, which may still read it (or would re-read it on a bin regrowth).  The per-frame pose setters --
// joint positions, cameras, link matrices -- are staged in rings and never wait.
#define WAIT_IF_PENDING(c) do { if ((c)->pending) { const int rc_ = rtuf_sync(c); if (rc_ != RTUF_OK) return rc_; } } while (0)

// ---- pipelines: forwarding from the front context to its kids -------------------------------------------------
#define KIDS_ALL(c, expr)                                                                  \
  if ((c) && !(c)->kids.empty()) {                                                         \
    int rc_ = RTUF_OK;                                                                     \
    for (rtuf_context* k : (c)->kids) { rc_ = (expr); if (rc_ < 0) { (c)->error = k->error; return rc_; } } \
    return rc_;                                                                            \
  }
#define KIDS_ONE(c, which, expr)                                                           \
  if ((c) && !(c)->kids.empty()) {                                                         \
    rtuf_context* k = (c)->kids[which];                                                    \
    const int rc_ = (expr);                                                                \
    if (rc_ < 0) (c)->error = k->error;                                                    \
    return rc_;                                                                            \
  }
// The kid that takes the next batch is chosen without side effects; the rotation and `order` (the kids of the batches in
// flight, oldest first) change only after the call, from what the kid really did: a successful call adds one entry, and
// whatever the kid retired on the way (its oldest when it was full, everything after a failed regrowth) is trimmed from
// the front -- so a call that fails before or after retiring leaves `order` describing exactly the batches in flight.
static void settle_order(rtuf_context* c, int j, bool accepted)
{
  if (accepted) {
    c->order.push_back(j);
    c->last_kid = j;
    c->next_kid = (j + 1) % (int)c->kids.size();
  }
  int have = (int)std::count(c->order.begin(), c->order.end(), j);
  for (const int want = c->kids[j]->pending; have > want; have--)
    c->order.erase(std::find(c->order.begin(), c->order.end(), j));
}
#define KIDS_NEXT(c, expr)                                                                 \
  if ((c) && !(c)->kids.empty()) {                                                         \
    const int j_ = (c)->next_kid;                                                          \
    rtuf_context* k = (c)->kids[j_];                                                       \
    const int rc_ = (expr);                                                                \
    settle_order((c), j_, rc_ >= 0);                                                       \
    if (rc_ < 0) (c)->error = k->error;                                                    \
    return rc_;                                                                            \
  }

// Do kernels of streams a and b run side by side?  The HIP runtime maps streams onto a handful of hardware queues
// (GPU_MAX_HW_QUEUES, 4 by default) in the order they are created, across everything in the process; two streams on one queue
// execute strictly one after the other.  Whether a new stream shares the queue of another cannot be asked, only measured: an
// idle kernel of 300 us on each, timed against one alone.  (Found the hard way: with an RCCL communicator in the process the
// two raster lanes of a context landed on one queue -- 381 k instead of 484 k frames/s, per-launch times those of kernels
// running alone.)
// RTUF_QUEUE_PROBE=0 in the environment skips the measurement (every stream is taken as the runtime hands it out): for hosts
// that share the GPU with other processes, where idle kernels cannot be timed, or that cannot spare the ~10 ms at start-up.
static bool queue_probe_enabled()
{
  static const bool on = [] { const char* e = getenv("RTUF_QUEUE_PROBE"); return !(e && e[0] == '0' && e[1] == 0); }();
  return on;
}
static bool streams_run_side_by_side(hipStream_t a, hipStream_t b)
{
  if (!queue_probe_enabled()) return true;
  using clk = std::chrono::steady_clock;
  const unsigned long long ticks = 30000;      // 300 us at 100 MHz
  launch_spin(100, a); launch_spin(100, b);    // (code object load, queue creation)
  if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) { (void)hipGetLastError(); return true; }
  auto timed = [&](bool both) {
    const auto t0 = clk::now();
    launch_spin(ticks, a);
    if (both) launch_spin(ticks, b);
    (void)hipStreamSynchronize(a);
    if (both) (void)hipStreamSynchronize(b);
    return std::chrono::duration<double>(clk::now() - t0).count();
  };
  // (the smallest of three: whatever else the GPU or the host is doing can only make a repetition longer)
  const double one = std::min(timed(false), std::min(timed(false), timed(false))), two = std::min(timed(true), std::min(timed(true), timed(true)));
  return two < 1.5 * one;
}

// A new non-blocking stream that runs beside every stream of `refs` (none: any stream).  Streams that turn out to share a
// hardware queue with one of them are set aside -- still alive, so that the runtime places the next one elsewhere -- and
// released afterwards; after eight of them the last one is taken as it is (*beside = false: it will work, behind whatever
// is queued in front of it).
static hipError_t create_stream_beside(const std::vector<hipStream_t>& refs, hipStream_t* out, bool* beside)
{
  *beside = true;
  hipError_t e = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
  if (e != hipSuccess || refs.empty()) return e;
  std::vector<hipStream_t> rejected;
  auto beside_all = [&](hipStream_t s) { for (hipStream_t r : refs) if (r && !streams_run_side_by_side(r, s)) return false; return true; };
  while (e == hipSuccess && !beside_all(*out)) {
    if (rejected.size() >= 8) { *beside = false; break; }
    rejected.push_back(*out);
    e = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
  }
  for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
  return e;
}
static hipError_t create_stream_beside(hipStream_t ref, hipStream_t* out, bool* beside)
{
  return create_stream_beside(ref ? std::vector<hipStream_t>{ref} : std::vector<hipStream_t>{}, out, beside);
}
static std::vector<hipStream_t> lane_streams(const rtuf_context* c)
{
  std::vector<hipStream_t> v;
  for (int l = 0; l < c->n_lanes; l++) v.push_back(c->lane[l].stream);
  return v;
}

extern "C" {

int rtuf_abi_version(void) { return RTUF_ABI_VERSION; }

void rtuf_default_params(rtuf_params* p)
{
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->near_plane = 0.1f;                  // src/urdf_filter.cpp:54
  p->far_plane = 8.0f;                   // src/urdf_filter.cpp:53
  p->depth_distance_threshold = 0.05f;   // launch/filter_parameters.yaml:14
  p->filter_replace_value = 0.0f;        // src/urdf_filter.cpp:106 default
  p->flags = RTUF_FLAG_DEFAULT;
}

const char* rtuf_last_error(const rtuf_context* ctx) { return ctx ? ctx->error.c_str() : g_create_error; }

int rtuf_create(rtuf_context** out, int device_id, int width, int height, int max_streams,
                const rtuf_params* params)
{
  if (!out) return RTUF_ERR_INVALID;
  *out = nullptr;
  if (width <= 0 || height <= 0 || width > 2048 || height > 2048 || max_streams <= 0) {
    snprintf(g_create_error, sizeof g_create_error, "invalid size %dx%d or stream count %d", width, height, max_streams);
    return RTUF_ERR_INVALID;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) {
    snprintf(g_create_error, sizeof g_create_error,
             "no usable HIP device (count=%d, requested %d): %s -- this library has no CPU fallback",
             ndev, device_id, e == hipSuccess ? "ok" : hipGetErrorString(e));
    return RTUF_ERR_NO_DEVICE;
  }
  if (params && !flags_valid(params->flags)) {
    snprintf(g_create_error, sizeof g_create_error, "unknown rtuf_params.flags bits 0x%x", params->flags & ~kKnownFlags);
    return RTUF_ERR_INVALID;
  }
  if (params && !dilation_valid(params)) {
    snprintf(g_create_error, sizeof g_create_error, "silhouette_dilation_px = %u: at most %d", params->silhouette_dilation_px, kMaxDilation);
    return RTUF_ERR_INVALID;
  }
  if (params && params->raster_lanes > (uint32_t)kMaxLanes) {
    snprintf(g_create_error, sizeof g_create_error, "raster_lanes = %u: at most %d", params->raster_lanes, kMaxLanes);
    return RTUF_ERR_INVALID;
  }
  {
    // the kernels exist for gfx950 (MI350X / MI355X) only: on any other device the first launch would fail with an opaque
    // "invalid device function"
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      snprintf(g_create_error, sizeof g_create_error,
               "device %d is %s, not gfx950 (MI350X / MI355X): this library carries gfx950 code only and has no CPU fallback",
               device_id, e == hipSuccess ? prop.gcnArchName : hipGetErrorString(e));
      return RTUF_ERR_NO_DEVICE;
    }
  }
  rtuf_context* c = new (std::nothrow) rtuf_context();
  if (!c) return RTUF_ERR_OOM;
  c->device = device_id;
  c->width = width; c->height = height; c->max_streams = max_streams;
  c->tiles_x = (width + kTileW - 1) / kTileW;
  c->tiles_y = (height + kTileH - 1) / kTileH;
  if (params) c->params = *params; else rtuf_default_params(&c->params);
  e = hipSetDevice(device_id);
  // (a front context of several pipelines owns no streams of its own: HIP multiplexes streams onto a few hardware queues,
  // and two pipelines whose main streams share a queue do not overlap at all)
  const bool front = c->params.pipelines > 1;
  c->n_lanes = c->params.raster_lanes ? (int)c->params.raster_lanes : kDefaultLanes;
  for (int l = 0; l < c->n_lanes && e == hipSuccess && !front; l++) {
    // every further lane must be able to run beside the ones before it
    bool beside = true;
    std::vector<hipStream_t> before;
    for (int k = 0; k < l; k++) before.push_back(c->lane[k].stream);
    e = create_stream_beside(before, &c->lane[l].stream, &beside);
    if (!beside) c->lanes_share_queue = true;
  }
  // The pose stage's stream must not share a hardware queue with a lane either: its few microseconds of kernels (forward
  // kinematics, matrix stacks, the first cull) would queue behind a quarter of a millisecond of set-up or tile kernel, and
  // every lane waits for them.  (Seen with an RCCL communicator in the process: 463 k instead of 504 k frames/s.)
  if (e == hipSuccess && !front) {
    bool beside = true;
    e = create_stream_beside(lane_streams(c), &c->side, &beside);
    if (!beside) c->lanes_share_queue = true;
  }
  if (e != hipSuccess) {
    snprintf(g_create_error, sizeof g_create_error, "hip init failed: %s", hipGetErrorString(e));
    delete c;
    return RTUF_ERR_HIP;
  }
  if (c->params.pipelines > 1) {
    if (c->params.pipelines > 4) { snprintf(g_create_error, sizeof g_create_error, "pipelines = %u: at most 4", c->params.pipelines); rtuf_destroy(c); return RTUF_ERR_INVALID; }
    // (the pipelines are the overlap here: every child is a context of one raster lane, whose small batches can replay graphs)
    rtuf_params kp = c->params;
    kp.pipelines = 0;
    kp.raster_lanes = 1;
    for (uint32_t i = 0; i < c->params.pipelines; i++) {
      rtuf_context* k = nullptr;
      const int rc = rtuf_create(&k, device_id, width, height, max_streams, &kp);
      if (rc != RTUF_OK) { rtuf_destroy(c); return rc; }
      k->graphs_ok = true;
      if (!c->kids.empty()) {
        // the pipelines exist to overlap: a child whose raster stream shares the first child's hardware queue gets another
        hipStream_t fresh = nullptr;
        bool beside = true;
        if (!streams_run_side_by_side(c->kids[0]->lane[0].stream, k->lane[0].stream) &&
            create_stream_beside(c->kids[0]->lane[0].stream, &fresh, &beside) == hipSuccess && fresh) {
          (void)hipStreamDestroy(k->lane[0].stream);
          k->lane[0].stream = fresh;
          if (!beside) c->lanes_share_queue = true;
        }
      }
      c->kids.push_back(k);
    }
  }
  *out = c;
  return RTUF_OK;
}

static void free_frame_buffers(rtuf_context* c)
{
  hipSetDevice(c->device);
  auto hfree = [](auto*& p) { if (p) { hipHostFree(p); p = nullptr; } };
  dev_free(c, c->d_model_mask);
  for (auto& b : c->batch) { dev_free(c, b.d_cams); dev_free(c, b.d_link_tf); dev_free(c, b.d_mvp); dev_free(c, b.d_bg); dev_free(c, b.d_counters); dev_free(c, b.d_status); }
  for (auto& ln : c->lane) {
    dev_free(c, ln.d_bins); dev_free(c, ln.d_bin_hdr); dev_free(c, ln.d_fbins); dev_free(c, ln.d_fbin_count); dev_free(c, ln.d_clip_list);
    dev_free(c, ln.d_clip_spill); dev_free(c, ln.d_big_list); dev_free(c, ln.d_zsurface); dev_free(c, ln.d_slots);
    for (auto*& it : ln.d_items) dev_free(c, it);
  }
  for (auto& b : c->batch) for (auto& st : b.st) { dev_free(c, st.p); st.have = 0; }
  for (auto& b : c->batch) { dev_free(c, b.cl_bits); dev_free(c, b.cl_rows); dev_free(c, b.pt_plane); dev_free(c, b.st_counts); dev_free(c, b.clr_posed); }
  for (auto*& p : c->ring_cams) hfree(p);
  for (auto*& p : c->ring_link_tf) hfree(p);
  c->h_cams = nullptr; c->h_link_tf = nullptr;
  hfree(c->h_model_mask);
  for (auto& b : c->batch) hfree(b.h_counters);
}

void rtuf_destroy(rtuf_context* c)
{
  if (!c) return;
  for (rtuf_context* k : c->kids) rtuf_destroy(k);
  c->kids.clear();
  hipSetDevice(c->device);
  if (c->side) hipStreamSynchronize(c->side);
  sync_lanes(c);
  if (c->h2d) hipStreamSynchronize(c->h2d);
  if (c->d2h) hipStreamSynchronize(c->d2h);
  for (HostModel& m : c->models) {
    Kinematics& k = m.kin;
    dev_free(c, k.d_depth); dev_free(c, k.d_parent); dev_free(c, k.d_type); dev_free(c, k.d_origin); dev_free(c, k.d_axis); dev_free(c, k.d_link_frame); dev_free(c, k.d_link_offset);
    dev_free(c, k.d_root); dev_free(c, k.d_enabled);
    for (double* q : k.h_q) if (q) hipHostFree(q);
    if (k.h_root) hipHostFree(k.h_root);
    if (k.h_enabled) hipHostFree(k.h_enabled);
  }
  free_frame_buffers(c);
  dev_free(c, c->d_cverts); dev_free(c, c->d_ctris); dev_free(c, c->d_corder); dev_free(c, c->d_chunks); dev_free(c, c->d_draws);
  dev_free(c, c->d_order_labels);
  dev_free(c, c->d_order_slot); dev_free(c, c->d_slot_pad); dev_free(c, c->d_pad_focal);
  dev_free(c, c->d_order_thr);
  dev_free(c, c->d_cloud_intr);
  dev_free(c, c->d_point_intr); dev_free(c, c->d_point_tf); dev_free(c, c->d_pt_stage);
  dev_free(c, c->d_clr_spheres); dev_free(c, c->d_clr_slot_label);
  dev_free(c, c->d_scene); dev_free(c, c->d_scene_streams); dev_free(c, c->d_scene_bits); dev_free(c, c->d_scene_stage);
  dev_free(c, c->d_vox_bits); dev_free(c, c->d_vox_counts); dev_free(c, c->d_vox_tf); dev_free(c, c->d_vox_mask_bits); dev_free(c, c->d_vox_stage);
  dev_free(c, c->d_vox_free); dev_free(c, c->d_vox_inv);
  for (auto& b : c->batch) {
    for (hipEvent_t ev : b.events) hipEventDestroy(ev);
    for (hipEvent_t ev : b.done) if (ev) hipEventDestroy(ev);
    if (b.posed) hipEventDestroy(b.posed);
    for (auto& g : b.graphs) if (g.exec) hipGraphExecDestroy(g.exec);
    if (b.uploaded) hipEventDestroy(b.uploaded);
    if (b.downloaded) hipEventDestroy(b.downloaded);
  }
  if (c->fork_ev) hipEventDestroy(c->fork_ev);
  for (void* p : c->pinned) hipHostFree(p);
  if (c->h2d) hipStreamDestroy(c->h2d);
  if (c->d2h) hipStreamDestroy(c->d2h);
  if (c->side) hipStreamDestroy(c->side);
  for (auto& ln : c->lane) if (ln.stream) hipStreamDestroy(ln.stream);
  delete c;
}

static int build_thresh_table(rtuf_context* c);

int rtuf_set_params(rtuf_context* c, const rtuf_params* p)
{
  if (!c || !p) return RTUF_ERR_INVALID;
  if (!flags_valid(p->flags)) return c->fail(RTUF_ERR_INVALID, "unknown rtuf_params.flags bits 0x%x", p->flags & ~kKnownFlags);
  if (!dilation_valid(p)) return c->fail(RTUF_ERR_INVALID, "silhouette_dilation_px = %u: at most %d", p->silhouette_dilation_px, kMaxDilation);
  if (!c->kids.empty()) {
    rtuf_params kp = *p;
    kp.pipelines = 0;
    for (rtuf_context* k : c->kids) { const int rc = rtuf_set_params(k, &kp); if (rc < 0) { c->error = k->error; return rc; } }
    const uint32_t keep = c->params.pipelines;
    c->params = c->kids[0]->params;
    c->params.pipelines = keep;
    return RTUF_OK;
  }
  WAIT_IF_PENDING(c);
  // the background quad's geometry (0.99 * far, src/urdf_filter.cpp:591-596) is built by rtuf_finalize_models
  if (c->finalized && p->far_plane != c->params.far_plane)
    return c->fail(RTUF_ERR_STATE, "far_plane is fixed once the models are finalized (was %g)", (double)c->params.far_plane);
  const uint32_t keep_cap = c->params.bin_capacity, keep_inf = c->params.max_inflight_streams, keep_pipes = c->params.pipelines;
  const uint32_t keep_lanes = c->params.raster_lanes, keep_limit = c->params.memory_limit_mb;
  const float keep_thr = c->params.depth_distance_threshold;
  c->params = *p;
  c->params.bin_capacity = keep_cap;
  c->params.max_inflight_streams = keep_inf;
  c->params.pipelines = keep_pipes;
  c->params.raster_lanes = keep_lanes;
  c->params.memory_limit_mb = keep_limit;
  // links without a threshold of their own (and the background quad drawn as geometry) follow the global one (bitwise: NaN too)
  if (c->thresh_models > 0 && memcmp(&keep_thr, &c->params.depth_distance_threshold, sizeof(float)) != 0) return build_thresh_table(c);
  return RTUF_OK;      // (two-kernel mode's z-surfaces are allocated by the first batch that needs them)
}

// ---- geometry -------------------------------------------------------------------------
int rtuf_add_model(rtuf_context* c)
{
  KIDS_ALL(c, rtuf_add_model(k));
  if (!c) return RTUF_ERR_INVALID;
  if (c->finalized) return c->fail(RTUF_ERR_STATE, "models already finalised");
  if (c->models.size() >= 64) return c->fail(RTUF_ERR_INVALID, "at most 64 models per context");
  c->models.emplace_back();
  return (int)c->models.size() - 1;
}

int rtuf_add_link(rtuf_context* c, int model)
{
  KIDS_ALL(c, rtuf_add_link(k, model));
  if (!c) return RTUF_ERR_INVALID;
  if (c->finalized) return c->fail(RTUF_ERR_STATE, "models already finalised");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  c->models[model].links.emplace_back();
  return (int)c->models[model].links.size() - 1;
}

int rtuf_add_draw(rtuf_context* c, int model, int link, int pre_op, const float op_xyz[3],
                  const float* vertices_xyz, int n_vertices, const uint32_t* triangles, int n_triangles)
{
  KIDS_ALL(c, rtuf_add_draw(k, model, link, pre_op, op_xyz, vertices_xyz, n_vertices, triangles, n_triangles));
  if (!c) return RTUF_ERR_INVALID;
  if (c->finalized) return c->fail(RTUF_ERR_STATE, "models already finalised");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  HostModel& m = c->models[model];
  if (link < 0 || link >= (int)m.links.size()) return c->fail(RTUF_ERR_INVALID, "bad link id %d", link);
  if (pre_op < RTUF_OP_NONE || pre_op > RTUF_OP_TRANSLATE) return c->fail(RTUF_ERR_INVALID, "bad pre_op %d", pre_op);
  if (n_vertices < 0 || n_triangles < 0 || (n_vertices && !vertices_xyz) || (n_triangles && !triangles))
    return c->fail(RTUF_ERR_INVALID, "bad geometry arrays");
  for (int i = 0; i < 3 * n_triangles; i++)
    if (triangles[i] >= (uint32_t)n_vertices) return c->fail(RTUF_ERR_INVALID, "triangle index %u out of range", triangles[i]);
  HostDraw d;
  d.pre_op = pre_op;
  for (int k = 0; k < 3; k++) d.op[k] = (pre_op != RTUF_OP_NONE && op_xyz) ? op_xyz[k] : 0.0f;
  d.verts.assign(vertices_xyz, vertices_xyz + 3 * (size_t)n_vertices);
  d.tris.assign(triangles, triangles + 3 * (size_t)n_triangles);
  m.links[link].draws.push_back(std::move(d));
  return (int)m.links[link].draws.size() - 1;
}

int rtuf_num_links(const rtuf_context* c, int model)
{
  if (c && !c->kids.empty()) return rtuf_num_links(c->kids[0], model);
  if (!c || model < 0 || model >= (int)c->models.size()) return RTUF_ERR_INVALID;
  return (int)c->models[model].links.size();
}

int64_t rtuf_num_triangles(const rtuf_context* c) { return c ? (c->kids.empty() ? c->n_tris : c->kids[0]->n_tris) : 0; }
int64_t rtuf_num_vertices(const rtuf_context* c) { return c ? (c->kids.empty() ? c->n_cverts : c->kids[0]->n_cverts) : 0; }

static int alloc_frame_buffers(rtuf_context* c)
{
  const int N = c->max_streams;
  const size_t tiles = (size_t)c->tiles_x * c->tiles_y;
  const size_t L = (size_t)std::max(c->n_links, 1);
  for (int r = 0; r <= kMaxInflight; r++) {
    HIP_TRY(c, hipHostMalloc(&c->ring_cams[r], sizeof(Camera) * N));
    HIP_TRY(c, hipHostMalloc(&c->ring_link_tf[r], sizeof(double) * 16 * L * N));
  }
  c->cam_ring = rtuf_context::StageRing(); c->link_ring = rtuf_context::StageRing();
  c->h_cams = c->ring_cams[0]; c->h_link_tf = c->ring_link_tf[0];
  HIP_TRY(c, hipHostMalloc(&c->h_model_mask, sizeof(uint64_t) * N));
  for (auto& b : c->batch)
    for (int l = 0; l < c->n_lanes; l++)
      if (!b.done[l]) HIP_TRY(c, hipEventCreateWithFlags(&b.done[l], hipEventDisableTiming));
  HIP_TRY(c, dev_alloc(c, &c->d_model_mask, sizeof(uint64_t) * N));
  for (auto& b : c->batch) {
    HIP_TRY(c, dev_alloc(c, &b.d_cams, sizeof(Camera) * N));
    HIP_TRY(c, dev_alloc(c, &b.d_link_tf, sizeof(double) * 16 * L * N));
    HIP_TRY(c, dev_alloc(c, &b.d_mvp, sizeof(float) * 16 * (size_t)(c->n_draws + 1) * N));
    HIP_TRY(c, dev_alloc(c, &b.d_bg, sizeof(BgInfo) * N));
    HIP_TRY(c, dev_alloc(c, &b.d_status, 64));
    HIP_TRY(c, hipMemset(b.d_status, 0, 64));
    b.dirty_cams = b.dirty_link_tf = true; b.uploaded_streams = 0;
    if (!b.posed) HIP_TRY(c, hipEventCreateWithFlags(&b.posed, hipEventDisableTiming));
  }
  c->dirty_mask = true; c->mask_uploaded_streams = 0;
  // identity defaults
  static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int s = 0; s < N; s++) {
    for (int r = 0; r <= kMaxInflight; r++) {
      Camera& cam = c->ring_cams[r][s];
      memcpy(cam.projection, I, sizeof I);
      memcpy(cam.offset_inv, I, sizeof I);
      memcpy(cam.cam_tf, I, sizeof I);
      cam.shift[0] = cam.shift[1] = 0.0;
      for (size_t l = 0; l < L; l++) memcpy(c->ring_link_tf[r] + ((size_t)s * L + l) * 16, I, sizeof I);
    }
    c->h_model_mask[s] = ~0ull;
  }
  // rasteriser working set
  // Launch group = the streams one lane's bins are sized for.  One lane: the whole batch up to 1024 streams (kernels of 4x
  // the work lose 4x less to their ramp and tail: 1024 streams in one group 522 k frames/s, in four groups of 256 one
  // after the other 460 k).  Several lanes: the streams divided by the lanes -- a full batch is one group per lane, the
  // lanes' kernels fill each other's ramps, tails and launch gaps, and the bins are what one group for all streams would
  // take.  (Measured on the 256-stream VGA workload: three lanes x 86 streams 514-525 k frames/s in 8.9 GB, two lanes x 128
  // 497-508 k in 8.8 GB, two x four groups of 64 490 k in 4.45 GB, one lane 469 k in 8.7 GB; 64 x 720p with two walls:
  // three lanes 180 k, two 168 k, one 143 k.  rtuf_params.memory_limit_mb / max_inflight_streams pick smaller working sets.)
  int G = c->params.max_inflight_streams ? (int)c->params.max_inflight_streams
                                         : (c->n_lanes > 1 && N >= kSplitMin ? std::min((N + c->n_lanes - 1) / c->n_lanes, 1024) : 1024);
  G = std::min(G, N);
  // Bins: fixed capacity per (stream, tile), direct addressing (one atomicAdd gives the slot: anything cleverer -- paged
  // bins were built and measured, DESIGN.md appendix A.2 -- costs the two big kernels 8 to 24 %).  What is NOT fixed any more is
  // the size: 1024 records + 4096 fragments per bin to start with (64 KiB per bin), grown on the first
  // batch to a quarter above the fullest bin that batch produced (the 250 k-triangle robot: 3840 + 13568; round 2
  // reserved 8192 + 32768 whatever the scene).  rtuf_params.bin_capacity fixes the starting point.
  uint32_t cap = c->params.bin_capacity ? c->params.bin_capacity : 1024u;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
  c->memory_budget = std::max(free_b / 3, (size_t)1 << 30);
  if (c->params.memory_limit_mb) c->memory_budget = (size_t)c->params.memory_limit_mb << 20;
  c->capacity = cap;
  c->fcapacity = std::max<uint32_t>(4 * cap, 1024);   // 8-byte fragments of all boxes up to 4x4 pixel centres
  while (G > 1 && (size_t)c->n_lanes * lane_bins_bytes(c, G, c->capacity, c->fcapacity) > c->memory_budget) G = (G + 1) / 2;
  c->group = G;
  c->stats.over_memory_limit = (size_t)c->n_lanes * lane_bins_bytes(c, G, c->capacity, c->fcapacity) > c->memory_budget ? 1u : 0u;      // (the first allocation can exceed it already)
  c->clip_capacity = (uint32_t)std::min<size_t>(std::max<size_t>((size_t)G * 8192 / kCounterShards, 1024), (size_t)1 << 22);   // per shard
  c->big_capacity = (uint32_t)std::min<size_t>(std::max<size_t>((size_t)G * 64, 1024), (size_t)1 << 20);                 // per shard
  for (int l = 0; l < c->n_lanes; l++) {
    rtuf_context::Lane& ln = c->lane[l];
    HIP_TRY(c, dev_alloc(c, &ln.d_bins, (size_t)G * tiles * cap * sizeof(PackedTri)));
    HIP_TRY(c, dev_alloc(c, &ln.d_bin_hdr, (size_t)G * tiles * sizeof(BinHeader)));
    HIP_TRY(c, dev_alloc(c, &ln.d_fbins, (size_t)G * tiles * c->fcapacity * sizeof(Frag)));
    HIP_TRY(c, dev_alloc(c, &ln.d_fbin_count, (size_t)G * tiles * sizeof(uint32_t)));
    HIP_TRY(c, hipMemsetAsync(ln.d_fbin_count, 0, (size_t)G * tiles * sizeof(uint32_t), ln.stream));
    launch_init_headers(ln.d_bin_hdr, (size_t)G * tiles, ln.stream);
    HIP_TRY(c, hipStreamSynchronize(ln.stream));
    HIP_TRY(c, dev_alloc(c, &ln.d_clip_list, (size_t)c->clip_capacity * kCounterShards * sizeof(ClipItem)));
    HIP_TRY(c, dev_alloc(c, &ln.d_clip_spill, clip_spill_bytes(c->clip_capacity)));
    HIP_TRY(c, dev_alloc(c, &ln.d_big_list, (size_t)c->big_capacity * kCounterShards * sizeof(BigRec)));
    for (auto*& it : ln.d_items) HIP_TRY(c, dev_alloc(c, &it, (size_t)c->n_chunks * (size_t)max_items_per_chunk(G) * sizeof(WorkItem)));
  }
  return alloc_counter_blocks(c);
}

int rtuf_finalize_models(rtuf_context* c)
{
  KIDS_ALL(c, rtuf_finalize_models(k));
  if (!c) return RTUF_ERR_INVALID;
  if (c->finalized) return c->fail(RTUF_ERR_STATE, "models already finalised");
  hipSetDevice(c->device);
  std::vector<float4> cverts;
  std::vector<uint32_t> ctris, corder;
  std::vector<Chunk> chunks;
  std::vector<Draw> draws;
  int64_t tri_seq = 0;
  // Splits one draw's triangle list into chunks of <= kBlock triangles / <= kMaxChunkVerts vertices.
  // Triangles are taken in Morton order of their centroids, so a chunk is a compact patch of the surface:
  // fewer distinct vertices per chunk (each is transformed once per chunk and stream) and a tighter
  // bounding sphere (more whole-chunk frustum culls) than the file order of a mesh gives.  The depth
  // test's tie-break is the GL draw order, so every triangle keeps its original sequence number (corder).
  auto add_chunks = [&](const std::vector<float>& v, const std::vector<uint32_t>& t, uint32_t draw_id, uint32_t model, bool background) {
    const uint32_t nt = (uint32_t)(t.size() / 3);
    // Vertices with bit-identical coordinates are one vertex here: STL (and Assimp's importers in general) bring three
    // vertices of their own per facet, and the vertex shader gives identical inputs identical results, so the image
    // cannot change -- but a chunk then transforms ~0.5 instead of 3 vertices per triangle and holds 256 triangles.
    std::vector<uint32_t> canon(v.size() / 3);
    {
      struct Key { uint32_t x, y, z; bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; } };
      struct KeyHash { size_t operator()(const Key& k) const { uint64_t h = k.x * 0x9E3779B97F4A7C15ull; h ^= (h >> 29) + k.y * 0xC2B2AE3D27D4EB4Full; h ^= (h >> 31) + k.z * 0x165667B19E3779F9ull; return (size_t)(h ^ (h >> 32)); } };
      std::unordered_map<Key, uint32_t, KeyHash> first;
      first.reserve(canon.size());
      for (uint32_t i = 0; i < (uint32_t)canon.size(); i++) {
        Key k;
        memcpy(&k, &v[3 * (size_t)i], sizeof k);
        canon[i] = first.emplace(k, i).first->second;
      }
    }
    std::vector<int32_t> local(v.size() / 3, -1);
    std::vector<uint32_t> touched;
    std::vector<uint32_t> perm(nt);
    for (uint32_t i = 0; i < nt; i++) perm[i] = i;
    if (nt > (uint32_t)kBlock && !RTUF_ABL(c->params.flags, 0x8000u)) {        // (0x8000 in RTUF_ABLATE builds: timing experiment, file order)
      float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
      for (size_t i = 0; i < v.size(); i++) { lo[i % 3] = std::min(lo[i % 3], v[i]); hi[i % 3] = std::max(hi[i % 3], v[i]); }
      auto spread = [](uint32_t x) {          // 10 bits -> every third bit
        x &= 1023u; x = (x | (x << 16)) & 0x030000ffu; x = (x | (x << 8)) & 0x0300f00fu;
        x = (x | (x << 4)) & 0x030c30c3u; x = (x | (x << 2)) & 0x09249249u;
        return x;
      };
      std::vector<uint32_t> code(nt);
      for (uint32_t i = 0; i < nt; i++) {
        uint32_t m = 0;
        for (int k = 0; k < 3; k++) {
          const float cen = (v[3 * (size_t)t[3 * (size_t)i] + k] + v[3 * (size_t)t[3 * (size_t)i + 1] + k] + v[3 * (size_t)t[3 * (size_t)i + 2] + k]) * (1.0f / 3.0f);
          const float ext = hi[k] - lo[k];
          const float u = ext > 0 ? (cen - lo[k]) / ext : 0.0f;
          m |= spread((uint32_t)std::min(1023.0f, std::max(0.0f, u * 1023.0f))) << k;
        }
        code[i] = m;
      }
      std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return code[x] < code[y]; });
    }
    uint32_t done = 0;
    while (done < nt) {
      Chunk ch{};
      ch.tri_begin = (uint32_t)ctris.size();
      ch.vert_begin = (uint32_t)cverts.size();
      ch.draw = draw_id; ch.model = model;
      touched.clear();
      uint32_t nv = 0, n = 0;
      while (done + n < nt && n < (uint32_t)kBlock) {
        const uint32_t ix[3] = {canon[t[3 * (size_t)perm[done + n]]], canon[t[3 * (size_t)perm[done + n] + 1]], canon[t[3 * (size_t)perm[done + n] + 2]]};
        uint32_t fresh = 0;
        for (int k = 0; k < 3; k++) {
          bool seen = local[ix[k]] >= 0;
          for (int q = 0; q < k && !seen; q++) seen = ix[q] == ix[k];
          if (!seen) fresh++;
        }
        if (nv + fresh > (uint32_t)kMaxChunkVerts) break;
        uint32_t li[3];
        for (int k = 0; k < 3; k++) {
          if (local[ix[k]] < 0) {
            local[ix[k]] = (int32_t)nv++;
            touched.push_back(ix[k]);
            cverts.push_back(make_float4(v[3 * (size_t)ix[k]], v[3 * (size_t)ix[k] + 1], v[3 * (size_t)ix[k] + 2], 1.0f));
          }
          li[k] = (uint32_t)local[ix[k]];
        }
        ctris.push_back(li[0] | (li[1] << 10) | (li[2] << 20));
        corder.push_back(background ? 0u : (uint32_t)(tri_seq + perm[done + n] + 1));
        n++;
      }
      ch.tri_count = n; ch.vert_count = nv;
      {
        // bounding box (centre + half extents, padded): used for whole-chunk frustum culling
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
        for (uint32_t q = 0; q < nv; q++) {
          const float4& p = cverts[ch.vert_begin + q];
          const float pp[3] = {p.x, p.y, p.z};
          for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], pp[k]); hi[k] = std::max(hi[k], pp[k]); }
        }
        for (int k = 0; k < 3; k++) {
          ch.center[k] = 0.5f * (lo[k] + hi[k]);
          // half extent about the rounded centre, rounded up (the cull test must stay conservative)
          ch.half[k] = std::nextafter(std::max(hi[k] - ch.center[k], ch.center[k] - lo[k]), INFINITY) * 1.0001f + 1e-7f;
        }
      }
      chunks.push_back(ch);
      for (uint32_t id : touched) local[id] = -1;
      done += n;
    }
    tri_seq += nt;
  };
  int link_base = 0;
  for (size_t mi = 0; mi < c->models.size(); mi++) {
    HostModel& m = c->models[mi];
    m.link_base = link_base;
    for (size_t li = 0; li < m.links.size(); li++) {
      for (const HostDraw& hd : m.links[li].draws) {
        Draw d{};
        d.link = (uint32_t)(link_base + li);
        d.pre_op = (uint32_t)hd.pre_op;
        d.op[0] = hd.op[0]; d.op[1] = hd.op[1]; d.op[2] = hd.op[2];
        d.model = (uint32_t)mi;
        const uint32_t draw_id = (uint32_t)draws.size();
        draws.push_back(d);
        add_chunks(hd.verts, hd.tris, draw_id, (uint32_t)mi, false);
        c->draw_link.push_back(d.link);
        c->draw_last_order.push_back((uint32_t)tri_seq);
      }
    }
    link_base += (int)m.links.size();
  }
  c->n_links = link_base;
  c->n_draws = (int)draws.size();
  c->n_tris = tri_seq;
  if (tri_seq >= (int64_t)kMaxOrder) return c->fail(RTUF_ERR_CAPACITY, "%lld triangles: draw-order keys are limited to %u", (long long)tri_seq, kMaxOrder);
  c->key_shift = key_shift_for((uint32_t)tri_seq);
  // background quad as the hidden last draw (used only when a stream's projection does not make
  // it a constant full-screen plane): GL_QUADS -> (0,1,3), (1,2,3); both get order 0
  {
    const float zq = (float)((double)c->params.far_plane * 0.99);
    const std::vector<float> bv = {-100.0f, -100.0f, zq, 100.0f, -100.0f, zq, 100.0f, 100.0f, zq, -100.0f, 100.0f, zq};
    const std::vector<uint32_t> bt = {0, 1, 3, 1, 2, 3};
    c->bg_chunk = (uint32_t)chunks.size();
    add_chunks(bv, bt, (uint32_t)c->n_draws, 0, true);
  }
  c->n_chunks = (int)chunks.size();
  c->n_cverts = (int64_t)cverts.size();
  if (draws.empty()) draws.push_back(Draw{});
  HIP_TRY(c, dev_alloc(c, &c->d_cverts, cverts.size() * sizeof(float4)));
  HIP_TRY(c, dev_alloc(c, &c->d_ctris, ctris.size() * sizeof(uint32_t)));
  HIP_TRY(c, dev_alloc(c, &c->d_corder, corder.size() * sizeof(uint32_t)));
  HIP_TRY(c, dev_alloc(c, &c->d_chunks, chunks.size() * sizeof(Chunk)));
  HIP_TRY(c, dev_alloc(c, &c->d_draws, draws.size() * sizeof(Draw)));
  HIP_TRY(c, hipMemcpy(c->d_cverts, cverts.data(), cverts.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_ctris, ctris.data(), ctris.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_corder, corder.data(), corder.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_chunks, chunks.data(), chunks.size() * sizeof(Chunk), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_draws, draws.data(), draws.size() * sizeof(Draw), hipMemcpyHostToDevice));
  const int rc = alloc_frame_buffers(c);
  if (rc != RTUF_OK) return rc;
  // host copies of the geometry are no longer needed
  for (HostModel& m : c->models)
    for (HostLink& l : m.links)
      for (HostDraw& d : l.draws) { d.verts.clear(); d.verts.shrink_to_fit(); d.tris.clear(); d.tris.shrink_to_fit(); }
  c->finalized = true;
  return RTUF_OK;
}

}  // extern "C"

// The setters of cameras / link matrices write into the staging set no batch in flight reads.  The first write after a
// batch took the previous set carries over what this call does not overwrite (`whole` = it overwrites everything).
template <typename T>
static void begin_write(rtuf_context::StageRing& r, T* const* sets, size_t count, bool whole)
{
  if (!r.carried) {
    if (!whole) memcpy(sets[r.write], sets[r.live], sizeof(T) * count);
    r.carried = true;
  }
  r.written = true;
}
static void begin_camera_write(rtuf_context* c, bool whole) { begin_write(c->cam_ring, c->ring_cams, (size_t)c->max_streams, whole); }
static void begin_link_write(rtuf_context* c, bool whole) { begin_write(c->link_ring, c->ring_link_tf, 16 * (size_t)std::max(c->n_links, 1) * (size_t)c->max_streams, whole); }
// The staging set that neither batch b, which reads `live`, nor a batch in flight beside it reads (idx_of: the set a batch
// reads, or -1): of kMaxInflight + 1 sets one is always free.
template <typename IdxOf>
static int free_set(const rtuf_context* c, const rtuf_context::Batch& b, int live, IdxOf idx_of)
{
  bool used[kMaxInflight + 1] = {};
  used[live] = true;
  for (const auto& o : c->batch) if (o.active && &o != &b && idx_of(o) >= 0) used[idx_of(o)] = true;
  int i = 0;
  while (i < kMaxInflight && used[i]) i++;
  return i;
}
// A new batch takes the staged set of one array (if anything was staged since the last batch) and moves the setters on
// to a set no batch in flight reads.  Returns the set the batch reads.
template <typename IdxOf>
static int take_staged(rtuf_context* c, rtuf_context::StageRing& r, const rtuf_context::Batch& b, IdxOf idx_of)
{
  // (nothing staged since the last batch, or ever: the batch reads the live set, so the setters must move on all the same --
  // a setter called while this batch is in flight would otherwise write into the pinned set its upload is still reading)
  if (r.written || r.write == r.live) {
    if (r.written) r.live = r.write;
    r.write = free_set(c, b, r.live, idx_of);
    r.written = r.carried = false;
  }
  return r.live;
}

extern "C" {

int rtuf_set_stream_models(rtuf_context* c, int stream, const int* model_ids, int n_models)
{
  KIDS_ALL(c, rtuf_set_stream_models(k, stream, model_ids, n_models));
  if (!c) return RTUF_ERR_INVALID;
  WAIT_IF_PENDING(c);
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (stream < 0 || stream >= c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad stream %d", stream);
  uint64_t mask = 0;
  for (int i = 0; i < n_models; i++) {
    if (model_ids[i] < 0 || model_ids[i] >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model_ids[i]);
    mask |= 1ull << model_ids[i];
  }
  c->h_model_mask[stream] = mask;
  c->dirty_mask = true;
  return RTUF_OK;
}

// ---- poses ----------------------------------------------------------------------------
int rtuf_set_camera(rtuf_context* c, int stream, const double projection[16], const double camera_offset_inv[16],
                    const double camera_tf[16])
{
  KIDS_ALL(c, rtuf_set_camera(k, stream, projection, camera_offset_inv, camera_tf));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (stream < 0 || stream >= c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad stream %d", stream);
  begin_camera_write(c, false);
  Camera& cam = c->h_cams[stream];
  if (projection) memcpy(cam.projection, projection, sizeof cam.projection);
  if (camera_offset_inv) memcpy(cam.offset_inv, camera_offset_inv, sizeof cam.offset_inv);
  if (camera_tf) memcpy(cam.cam_tf, camera_tf, sizeof cam.cam_tf);
  for (auto& b : c->batch) b.dirty_cams = true;
  return RTUF_OK;
}

// getProjectionMatrix, src/urdf_filter.cpp:459-501
void rtuf_projection_from_intrinsics(double fx, double fy, double cx, double cy, double Tx, double Ty, int width,
                                     int height, double near_plane, double far_plane, double P[16],
                                     double* camera_tx, double* camera_ty)
{
  if (camera_tx) *camera_tx = -1 * (Tx / fx);
  if (camera_ty) *camera_ty = -1 * (Ty / fy);
  for (int i = 0; i < 16; i++) P[i] = 0.0;
  P[0] = -2.0 * fx / width;
  P[5] = 2.0 * fy / height;
  P[8] = 2.0 * (0.5 - cx / width);
  P[9] = 2.0 * (cy / height - 0.5);
  P[10] = -(far_plane + near_plane) / (far_plane - near_plane);
  P[14] = -2.0 * far_plane * near_plane / (far_plane - near_plane);
  P[11] = -1;
}

int rtuf_set_link_poses(rtuf_context* c, int stream, int model, const double* link_tf, int n_links)
{
  KIDS_ALL(c, rtuf_set_link_poses(k, stream, model, link_tf, n_links));
  if (!c || !link_tf) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (stream < 0 || stream >= c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad stream %d", stream);
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  const HostModel& m = c->models[model];
  if (n_links != (int)m.links.size()) return c->fail(RTUF_ERR_INVALID, "model %d has %d links, got %d", model, (int)m.links.size(), n_links);
  // (switching a stream off forward kinematics changes single-buffered state: that alone waits for the batches in flight)
  if (m.kin.h_enabled && m.kin.h_enabled[stream]) WAIT_IF_PENDING(c);
  begin_link_write(c, false);
  memcpy(c->h_link_tf + ((size_t)stream * c->n_links + m.link_base) * 16, link_tf, sizeof(double) * 16 * (size_t)n_links);
  // (a stream that leaves forward kinematics also gets its host-set camera back: the FK kernel may have overwritten cam_tf)
  if (m.kin.h_enabled && m.kin.h_enabled[stream]) { c->models[model].kin.h_enabled[stream] = 0; c->models[model].kin.dirty_aux = true; for (auto& b : c->batch) b.dirty_cams = true; }
  for (auto& b : c->batch) b.dirty_link_tf = true;
  return RTUF_OK;
}

int rtuf_set_cameras(rtuf_context* c, int first, int n, const double* projection, const double* offset_inv,
                     const double* cam_tf)
{
  KIDS_ALL(c, rtuf_set_cameras(k, first, n, projection, offset_inv, cam_tf));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (first < 0 || n < 0 || first + n > c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad stream range %d+%d", first, n);
  begin_camera_write(c, false);
  for (int s = 0; s < n; s++) {
    Camera& cam = c->h_cams[first + s];
    if (projection) memcpy(cam.projection, projection + 16 * (size_t)s, sizeof cam.projection);
    if (offset_inv) memcpy(cam.offset_inv, offset_inv + 16 * (size_t)s, sizeof cam.offset_inv);
    if (cam_tf) memcpy(cam.cam_tf, cam_tf + 16 * (size_t)s, sizeof cam.cam_tf);
  }
  for (auto& b : c->batch) b.dirty_cams = true;
  return RTUF_OK;
}

int rtuf_set_camera_shift(rtuf_context* c, int first, int n, const double* camera_tx, const double* camera_ty)
{
  KIDS_ALL(c, rtuf_set_camera_shift(k, first, n, camera_tx, camera_ty));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (first < 0 || n < 0 || first + n > c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad stream range %d+%d", first, n);
  begin_camera_write(c, false);
  for (int s = 0; s < n; s++) {
    c->h_cams[first + s].shift[0] = camera_tx ? camera_tx[s] : 0.0;
    c->h_cams[first + s].shift[1] = camera_ty ? camera_ty[s] : 0.0;
  }
  for (auto& b : c->batch) b.dirty_cams = true;
  return RTUF_OK;
}

int rtuf_set_link_poses_batch(rtuf_context* c, int first, int n, int model, const double* link_tf, int n_links)
{
  KIDS_ALL(c, rtuf_set_link_poses_batch(k, first, n, model, link_tf, n_links));
  if (!c || !link_tf) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (first < 0 || n < 0 || first + n > c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad stream range %d+%d", first, n);
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  const HostModel& m = c->models[model];
  if (n_links != (int)m.links.size()) return c->fail(RTUF_ERR_INVALID, "model %d has %d links, got %d", model, (int)m.links.size(), n_links);
  // (switching streams off forward kinematics changes single-buffered state: that alone waits for the batches in flight)
  if (m.kin.h_enabled) for (int s = 0; s < n; s++) if (m.kin.h_enabled[first + s]) { WAIT_IF_PENDING(c); break; }
  // one model that owns every link, all streams: this call overwrites the whole set, nothing to carry over
  begin_link_write(c, first == 0 && n == c->max_streams && n_links == c->n_links);
  for (int s = 0; s < n; s++) {
    memcpy(c->h_link_tf + ((size_t)(first + s) * c->n_links + m.link_base) * 16, link_tf + (size_t)s * n_links * 16,
           sizeof(double) * 16 * (size_t)n_links);
    if (m.kin.h_enabled && m.kin.h_enabled[first + s]) { c->models[model].kin.h_enabled[first + s] = 0; c->models[model].kin.dirty_aux = true; for (auto& b : c->batch) b.dirty_cams = true; }
  }
  for (auto& b : c->batch) b.dirty_link_tf = true;
  return RTUF_OK;
}


// column-major GL matrix -> row-major 3x3 basis + origin
static void gl_to_tf12(const double* g, double* t)
{
  t[0] = g[0]; t[1] = g[4]; t[2] = g[8];
  t[3] = g[1]; t[4] = g[5]; t[5] = g[9];
  t[6] = g[2]; t[7] = g[6]; t[8] = g[10];
  t[9] = g[12]; t[10] = g[13]; t[11] = g[14];
}

int rtuf_set_kinematics(rtuf_context* c, int model, int n_frames, const int32_t* parent, const int32_t* joint_type,
                        const double* joint_origin, const double* joint_axis, const int32_t* link_frame,
                        const double* link_offset, int n_links)
{
  KIDS_ALL(c, rtuf_set_kinematics(k, model, n_frames, parent, joint_type, joint_origin, joint_axis, link_frame, link_offset, n_links));
  if (!c || !parent || !joint_type || !joint_origin || !joint_axis || !link_frame || !link_offset) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  HostModel& m = c->models[model];
  if (n_links != (int)m.links.size()) return c->fail(RTUF_ERR_INVALID, "model %d has %d links, got %d", model, (int)m.links.size(), n_links);
  if (n_frames <= 0 || n_frames > 4096) return c->fail(RTUF_ERR_INVALID, "bad frame count %d", n_frames);
  for (int i = 0; i < n_frames; i++) {
    if (parent[i] >= i || parent[i] < -1) return c->fail(RTUF_ERR_INVALID, "frame %d: parent %d must precede it", i, parent[i]);
    if (joint_type[i] < 0 || joint_type[i] > 2) return c->fail(RTUF_ERR_INVALID, "frame %d: bad joint type %d", i, joint_type[i]);
    int depth = 0;
    for (int f = i; f >= 0; f = parent[f]) if (++depth > 64) return c->fail(RTUF_ERR_INVALID, "kinematic chain deeper than 64");
  }
  for (int l = 0; l < n_links; l++)
    if (link_frame[l] < 0 || link_frame[l] >= n_frames) return c->fail(RTUF_ERR_INVALID, "link %d: bad frame %d", l, link_frame[l]);
  hipSetDevice(c->device);
  Kinematics& k = m.kin;
  if (k.n_frames) return c->fail(RTUF_ERR_STATE, "kinematics of model %d already set", model);
  std::vector<double> org(12 * (size_t)n_frames), off(12 * (size_t)std::max(n_links, 1));
  for (int i = 0; i < n_frames; i++) gl_to_tf12(joint_origin + 16 * (size_t)i, &org[12 * (size_t)i]);
  for (int l = 0; l < n_links; l++) gl_to_tf12(link_offset + 16 * (size_t)l, &off[12 * (size_t)l]);
  const size_t N = (size_t)c->max_streams;
  std::vector<int32_t> depth(n_frames, 0);
  int max_depth = 0;
  for (int i = 0; i < n_frames; i++) { depth[i] = parent[i] < 0 ? 0 : depth[parent[i]] + 1; max_depth = std::max(max_depth, depth[i]); }
  // all or nothing: a failure part-way releases what this call allocated, so the call can simply be made again
  auto release = [&]() {
    dev_free(c, k.d_depth); dev_free(c, k.d_parent); dev_free(c, k.d_type); dev_free(c, k.d_origin); dev_free(c, k.d_axis);
    dev_free(c, k.d_link_frame); dev_free(c, k.d_link_offset); dev_free(c, k.d_root); dev_free(c, k.d_enabled);
    for (double*& q : k.h_q) if (q) { hipHostFree(q); q = nullptr; }
    if (k.h_root) { hipHostFree(k.h_root); k.h_root = nullptr; }
    if (k.h_enabled) { hipHostFree(k.h_enabled); k.h_enabled = nullptr; }
  };
  auto build = [&]() -> hipError_t {
    hipError_t e;
#define KIN_TRY(expr) do { e = (expr); if (e != hipSuccess) return e; } while (0)
    KIN_TRY(dev_alloc(c, &k.d_depth, sizeof(int32_t) * n_frames));
    KIN_TRY(dev_alloc(c, &k.d_parent, sizeof(int32_t) * n_frames));
    KIN_TRY(dev_alloc(c, &k.d_type, sizeof(int32_t) * n_frames));
    KIN_TRY(dev_alloc(c, &k.d_origin, sizeof(double) * 12 * n_frames));
    KIN_TRY(dev_alloc(c, &k.d_axis, sizeof(double) * 3 * n_frames));
    KIN_TRY(dev_alloc(c, &k.d_link_frame, sizeof(int32_t) * std::max(n_links, 1)));
    KIN_TRY(dev_alloc(c, &k.d_link_offset, sizeof(double) * off.size()));
    KIN_TRY(dev_alloc(c, &k.d_root, sizeof(double) * N * 12));
    KIN_TRY(dev_alloc(c, &k.d_enabled, N));
    for (double*& q : k.h_q) KIN_TRY(hipHostMalloc(&q, sizeof(double) * N * n_frames));
    KIN_TRY(hipHostMalloc(&k.h_root, sizeof(double) * N * 12));
    KIN_TRY(hipHostMalloc(&k.h_enabled, N));
    memset(k.h_enabled, 0, N);
    for (double* q : k.h_q) memset(q, 0, sizeof(double) * N * n_frames);
    KIN_TRY(hipMemcpy(k.d_depth, depth.data(), sizeof(int32_t) * n_frames, hipMemcpyHostToDevice));
    KIN_TRY(hipMemcpy(k.d_parent, parent, sizeof(int32_t) * n_frames, hipMemcpyHostToDevice));
    KIN_TRY(hipMemcpy(k.d_type, joint_type, sizeof(int32_t) * n_frames, hipMemcpyHostToDevice));
    KIN_TRY(hipMemcpy(k.d_origin, org.data(), sizeof(double) * org.size(), hipMemcpyHostToDevice));
    KIN_TRY(hipMemcpy(k.d_axis, joint_axis, sizeof(double) * 3 * n_frames, hipMemcpyHostToDevice));
    if (n_links) KIN_TRY(hipMemcpy(k.d_link_frame, link_frame, sizeof(int32_t) * n_links, hipMemcpyHostToDevice));
    KIN_TRY(hipMemcpy(k.d_link_offset, off.data(), sizeof(double) * off.size(), hipMemcpyHostToDevice));
#undef KIN_TRY
    return hipSuccess;
  };
  const hipError_t e = build();
  if (e != hipSuccess) {
    release();
    return c->fail(e == hipErrorOutOfMemory ? RTUF_ERR_OOM : RTUF_ERR_HIP, "rtuf_set_kinematics: %s", hipGetErrorString(e));
  }
  k.max_depth = max_depth;
  k.n_frames = n_frames;
  return RTUF_OK;
}

int rtuf_set_joint_positions(rtuf_context* c, int first, int n, int model, const double* q, const double* root_tf, int camera_frame)
{
  KIDS_ALL(c, rtuf_set_joint_positions(k, first, n, model, q, root_tf, camera_frame));
  if (!c || !q) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  if (first < 0 || n < 0 || first + n > c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad stream range %d+%d", first, n);
  Kinematics& k = c->models[model].kin;
  if (!k.n_frames) return c->fail(RTUF_ERR_STATE, "call rtuf_set_kinematics for model %d first", model);
  if (camera_frame < -1 || camera_frame >= k.n_frames) return c->fail(RTUF_ERR_INVALID, "bad camera frame %d", camera_frame);
  static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  // root transforms, enable flags and the camera frame are staged in single buffers: changing them
  // while a batch is in flight waits for that batch first (joint positions alone never wait)
  bool aux_changes = camera_frame != k.camera_frame;
  std::vector<double> roots(12 * (size_t)n);
  for (int s = 0; s < n; s++) {
    double* r12 = &roots[12 * (size_t)s];
    if (root_tf) gl_to_tf12(root_tf + 16 * (size_t)s, r12);
    else memcpy(r12, I12, sizeof I12);
    if (memcmp(k.h_root + 12 * (size_t)(first + s), r12, sizeof I12) != 0 || !k.h_enabled[first + s]) aux_changes = true;
  }
  if (aux_changes && c->pending) { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }
  if (!k.q_carried) {
    // first write after a batch took the other buffer: carry the streams this call does not set
    if (first != 0 || n != c->max_streams) memcpy(k.h_q[k.q_write], k.h_q[k.q_live], sizeof(double) * (size_t)c->max_streams * k.n_frames);
    k.q_carried = true;
  }
  memcpy(k.h_q[k.q_write] + (size_t)first * k.n_frames, q, sizeof(double) * (size_t)n * k.n_frames);
  k.dirty_q = true;
  if (aux_changes) {
    for (int s = 0; s < n; s++) {
      memcpy(k.h_root + 12 * (size_t)(first + s), &roots[12 * (size_t)s], sizeof I12);
      k.h_enabled[first + s] = 1;
    }
    k.dirty_aux = true;
  }
  // leaving the robot-mounted camera: both slots take the host-set camera transforms again
  if (camera_frame != k.camera_frame) for (auto& b : c->batch) b.dirty_cams = true;
  k.camera_frame = camera_frame;
  k.any_enabled = true;
  return RTUF_OK;
}

int rtuf_debug_read_poses(rtuf_context* c, int n, double* link_tf_out, double* cam_tf_out)
{
  KIDS_ONE(c, c->last_kid, rtuf_debug_read_poses(k, n, link_tf_out, cam_tf_out));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized || n <= 0 || n > c->max_streams) return c->fail(RTUF_ERR_INVALID, "bad arguments");
  hipSetDevice(c->device);
  HIP_TRY(c, hipStreamSynchronize(c->side));
  sync_lanes(c);
  const size_t L = (size_t)std::max(c->n_links, 1);
  if (link_tf_out) HIP_TRY(c, hipMemcpy(link_tf_out, c->batch[c->last_slot].d_link_tf, sizeof(double) * 16 * L * n, hipMemcpyDeviceToHost));
  if (cam_tf_out) {
    std::vector<Camera> cams(n);
    HIP_TRY(c, hipMemcpy(cams.data(), c->batch[c->last_slot].d_cams, sizeof(Camera) * n, hipMemcpyDeviceToHost));
    for (int s = 0; s < n; s++) memcpy(cam_tf_out + 16 * (size_t)s, cams[s].cam_tf, sizeof(double) * 16);
  }
  return RTUF_OK;
}

// ---- what a batch of each kind does ----
// Which kernels it runs, or why none, is its route (route_of in rtuf_routes.h, asked by check_route for the calls and once by
// enqueue_batch; a new kind starts there).  The two predicates below are still asked BEFORE a batch has a route -- when a slot is
// taken (the in-flight limit of one) and when its buffers are allocated (the z-surface and slot planes, last_lane) -- and say
// more than the route would: a cloud batch under the two-kernel flag never takes the z-surface route, but its context has always
// allocated the z-surface for it, and rtuf_stats.device_bytes counts it.
// the batches of this context write the z-surface: two-kernel mode, a silhouette dilation radius, or link padding in effect
static bool uses_zsurface(const rtuf_context* c) { return (c->params.flags & RTUF_FLAG_TWO_KERNEL) != 0 || c->params.silhouette_dilation_px > 0 || c->pad_models > 0; }
// may write the z-surface, and so needs d_zsurface and moves last_lane (render and residual batches never take that route and leave it alone)
static bool may_write_zsurface(const BatchRequest& r) { return r.kind != Kind::Render && r.kind != Kind::Residual && r.kind != Kind::Points; }

// The facts the route of a request follows from, as the context stands (r.labels: only whether there is one is asked).
static RouteFacts route_facts(const rtuf_context* c, const BatchRequest& r)
{
  return RouteFacts{r.kind, r.u16, r.labels != nullptr, c->thresh_models > 0, (c->params.flags & RTUF_FLAG_TWO_KERNEL) != 0, (int)c->params.silhouette_dilation_px,
                    c->cover_on, c->pad_models > 0, c->scene_enabled > 0 && !r.robot_only};
}

// Refuses the request if it has no route, with the reason's message (rtuf_routes.h, enum class Refusal: the rules and their
// order).  Every batch call asks once, behind the checks of its own arguments and before it builds, allocates, stages or
// enqueues anything: a refused call leaves the context as it found it.
static int check_route(rtuf_context* c, const BatchRequest& r)
{
  static const char* const text[] = {
    nullptr,
    "internal: a label plane for a batch kind that has none",      // (NoLabelPlane: no call has the argument)
    "link labels are not supported with silhouette dilation yet",
    "link labels are not supported with link padding yet",
    "virtual depth is not supported with silhouette dilation yet",
    "virtual depth is not supported with link padding yet",
    "link residual tables are not supported with silhouette dilation yet",
    "link residual tables are not supported with link padding yet",
    "silhouette dilation is not supported with link padding yet",
    "per-link depth thresholds are not supported with link padding yet",
    "per-link depth thresholds are not supported with RTUF_FLAG_TWO_KERNEL or silhouette dilation yet",
    "per-link depth thresholds are not supported with silhouette dilation yet",
    "mask-bits output exists in fused mode only (RTUF_FLAG_TWO_KERNEL is set)",
    "point list batches are not supported with silhouette dilation yet (radius_px is this batch's own margin)",
    "point list batches are not supported with link padding yet",
    "point list batches are not supported with per-link depth thresholds yet",
  };
  static_assert(sizeof text / sizeof *text == (size_t)Refusal::PointsThresh + 1, "one message per reason, in the enum's order");
  const Refusal why = route_of(route_facts(c, r)).why;
  return why == Refusal::None ? RTUF_OK : c->fail(RTUF_ERR_INVALID, "%s", text[(int)why]);
}

// ---- the hot path ---------------------------------------------------------------------
static hipEvent_t get_event(rtuf_context::Batch& b, size_t i)
{
  while (b.events.size() <= i) {
    hipEvent_t ev; hipEventCreate(&ev); b.events.push_back(ev);
  }
  return b.events[i];
}

// Everything one batch launches, as plain argument blocks: built first, then either enqueued kernel by kernel or --
// for small batches, whose cost is the host's launch overhead, not GPU time -- captured once into a hipGraph per
// batch slot and replayed with one call for as long as the blocks do not change (same buffers, sizes, parameters).
struct BatchPlan {
  std::vector<FkArgs> fks;
  PoseArgs pa{};
  // (ca, da, pd, sc, cl, cr, pt: filled and read where the route's post / scene stage / tail has that kernel)
  struct Group { SetupArgs sa{}; TileArgs ta{}; CompareArgs ca{}; DilateArgs da{}; PadArgs pd{}; SceneArgs sc{}; CloudArgs cl{}; ClearanceArgs cr{}; PointsArgs pt{}; int lane = 0; };
  std::vector<Group> groups;
  Route route{};                // the batch's (Batch::route): every group runs the same kernels
  uint64_t hash() const
  {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const void* p, size_t n) { const unsigned char* q = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; i++) { h ^= q[i]; h *= 1099511628211ull; } };
    for (const FkArgs& f : fks) mix(&f, sizeof f);
    mix(&pa, sizeof pa);
    for (const Group& g : groups) {
      mix(&g.sa, sizeof g.sa); mix(&g.ta, sizeof g.ta);
      if (route.post == Post::Compare) mix(&g.ca, sizeof g.ca);
      if (route.post == Post::Dilate) mix(&g.da, sizeof g.da);
      if (route.post == Post::Pad) mix(&g.pd, sizeof g.pd);
      if (route.scene) mix(&g.sc, sizeof g.sc);
      if (route.tail == Tail::Cloud) mix(&g.cl, sizeof g.cl);
      if (route.tail == Tail::Clearance) mix(&g.cr, sizeof g.cr);
      if (route.tail == Tail::Points) mix(&g.pt, sizeof g.pt);
      mix(&g.lane, sizeof g.lane);
    }
    // (the route too: equal argument blocks on another route are other kernels)
    return h ^ (uint64_t)fks.size() << 56 ^ (uint64_t)groups.size() << 48 ^ (uint64_t)route_index(route) << 32;
  }
};

static constexpr int kGraphMaxStreams = 32;     // batches up to this size replay a captured hipGraph (timing off)

// Timing events of a batch: start and end of the pose stage, the end of every lane's part, and five per launch group --
// E0 before its first kernel (mode 1: the cull; mode 2: the set-up kernel), E1 after the set-up kernel (mode 2), E2 after
// clip + many-tile kernels, E3 after the tile kernel, E4 after the compare kernel (two-kernel mode).
enum { kEvStart = 0, kEvPoseEnd = 1, kEvLaneEnd = 2, kEvGroup0 = 2 + kMaxLanes, kEvPerGroup = 5 };

// Enqueues the kernels of a plan: pose stage (forward kinematics, matrix stacks) on `sp`, then every launch group on the
// stream of its lane, which waits for the pose stage through the batch's `posed` event.  The cull of every lane's first
// group still belongs to the pose stage (it then runs under the previous batch's raster kernels).
static int issue_plan(rtuf_context* c, rtuf_context::Batch& b, const BatchPlan& plan, hipStream_t sp, bool worst_case_grid)
{
  const Route& rt = plan.route;
  worst_case_grid = worst_case_grid || c->force_worst_grid || (c->params.flags & RTUF_FLAG_STRICT_GRID) != 0;
  auto mark = [&](size_t i, hipStream_t s) { hipEventRecord(get_event(b, i), s); };
  if (b.timing) (void)get_event(b, kEvGroup0 + kEvPerGroup * plan.groups.size() - 1);      // (all of the batch's events exist)
  if (b.timing == 1) mark(kEvStart, sp);
  for (const FkArgs& fa : plan.fks) launch_fk(fa, sp);
  launch_pose(plan.pa, sp);
  if (b.timing == 1) mark(kEvPoseEnd, sp);
  // The cull of every lane's FIRST group belongs to the pose stage: it then runs under the raster kernels of the batch before
  // (its work list is the lane's own array of this batch slot, which nothing in flight reads), and the lane starts with the
  // set-up kernel instead of a 6 us kernel and the gap behind it (256 VGA streams +0.8 %, 64 x 720p +2.2 %, four groups of 64
  // +1.4 %).  Later groups of a lane reuse that array and cull in turn.  (Moving the other small kernel of a lane's chain --
  // the copy of the counters -- to a stream of its own behind an event was measured as well: -0.5 %, one camera -12 %.)
  auto cull_in_pose = [&](size_t g) {
    return g < (size_t)c->n_lanes && (g == 0 || plan.groups[g].lane != plan.groups[g - 1].lane);
  };
  for (size_t g = 0; g < plan.groups.size() && g < (size_t)c->n_lanes; g++)
    if (cull_in_pose(g)) launch_cull(plan.groups[g].sa, sp);
  HIP_TRY(c, hipEventRecord(b.posed, sp));
  for (int l = 0; l < c->n_lanes; l++)
    if (b.lanes_used >> l & 1u) HIP_TRY(c, hipStreamWaitEvent(c->lane[l].stream, b.posed, 0));
  for (size_t g = 0; g < plan.groups.size(); g++) {
    const BatchPlan::Group& gr = plan.groups[g];
    hipStream_t st = c->lane[gr.lane].stream;
    const size_t e0 = kEvGroup0 + kEvPerGroup * g;
    if (b.timing == 1) mark(e0, st);
    if (!cull_in_pose(g)) launch_cull(gr.sa, st);
    if (b.timing >= 2) mark(e0, st);                 // (after the wait for the pose stage: set-up time only)
    // The set-up grid is sized from the previous batch's work lists (scaled to this group's streams); the group's list
    // length comes back with its counters, and a batch whose list outgrew the grid is run again (retire_oldest).
    // A group of the same index and size as in the last retired batch takes ITS OWN list length (work lists are not linear in
    // the streams: every chunk rounds its visible streams up to whole items, and visibility differs per stream -- a smaller
    // last group can need more than its share of the largest group's list); any other group the longest list scaled to its
    // streams plus one item per chunk for that rounding.
    uint32_t hint = 0;
    if (!worst_case_grid && c->items_hint && c->items_hint_streams > 0) {
      const uint32_t scaled = (uint32_t)(((uint64_t)c->items_hint * (uint64_t)gr.sa.group_size + (uint64_t)c->items_hint_streams - 1) / (uint64_t)c->items_hint_streams);
      // (its own length, but never below half of what the longest list makes per stream: a group whose cameras saw nearly
      // nothing last time would otherwise take a grid of a few dozen workgroups, and the robot moving into ITS view would cost
      // a re-run of everything in flight where the old max-based estimate covered it; idle workgroups of the floor end at once)
      if (g < c->group_items.size() && c->group_streams[g] == gr.sa.group_size) hint = std::max(std::max(c->group_items[g], scaled / 2u), 1u);
      else hint = scaled + (uint32_t)c->n_chunks;
    }
    const uint32_t grid = launch_setup(gr.sa, hint, false, st);
    b.setup_grid[g] = worst_case_grid ? 0xffffffffu : grid;
    if (b.timing >= 2) mark(e0 + 1, st);
    launch_clip(gr.sa, st);
    launch_bigrec(gr.sa, rt.tile.cover, st);      // appends the many-tile records the two kernels above listed (after the cover pass, if it is on)
    if (b.timing) mark(e0 + 2, st);
    // a residual batch: the group's rows of the table are contiguous and start from zero on every run (timed with the tile
    // kernel: ms_raster)
    if (rt.tile.out == TileOut::Residual)
      launch_zero_residual_rows(gr.ta.resid_table + (size_t)gr.ta.group_base * (size_t)gr.ta.n_labels * 8u,
                                (size_t)gr.ta.group_size * (size_t)gr.ta.n_labels * 8u, st);
    if (!launch_tile(gr.ta, rt.tile, st)) return c->fail(RTUF_ERR_STATE, "internal: the tile kernel has no variant %d", tile_variant_index(rt.tile));
    if (b.timing) mark(e0 + 3, st);
    // behind it: the outputs from the z-surface, then what reads the mask bits (a cloud batch: the group's points; a clearance
    // batch: the group's rows of the table) before the lane publishes its counters -- timed together as ms_compare
    if (rt.post == Post::Compare) launch_compare(gr.ca, st);
    if (rt.post == Post::Dilate) launch_dilate_compare(gr.da, st);
    if (rt.post == Post::Pad) launch_pad_compare(gr.pd, st);
    if (rt.scene) launch_scene_apply(gr.sc, st);      // the scene's verdict on top of the outputs or bits, before anything reads the bits
    if (rt.tail == Tail::Cloud) launch_cloud(gr.cl, st);
    if (rt.tail == Tail::Clearance) launch_clearance(gr.cr, st);
    if (rt.tail == Tail::Points) launch_points(gr.pt, st);      // (reads the plane the group's tile_render_kernel just wrote)
    if (b.timing && runs_behind_tile(rt)) mark(e0 + 4, st);
  }
  // every lane publishes the counter blocks of its own groups
  const int ng = (int)plan.groups.size();
  const PublishLimits lim = {c->capacity, c->fcapacity, c->big_capacity};
  for (int l = 0; l < c->n_lanes; l++) {
    if (!(b.lanes_used >> l & 1u)) continue;
    if (ng == 1) launch_publish_counters(b.d_counters, b.h_counters, 0, 1, 1, b.d_status, lim, c->lane[l].stream);
    else launch_publish_counters(b.d_counters, b.h_counters, l, c->n_lanes, (ng - l + c->n_lanes - 1) / c->n_lanes, b.d_status, lim, c->lane[l].stream);
    if (b.timing == 1) mark(kEvLaneEnd + l, c->lane[l].stream);
  }
  return RTUF_OK;
}

static bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1u)) == 0u; }

// ---- the steps of enqueue_batch, in the order it calls them (each is called from there and from nowhere else) ----
// The slot takes its route, its lanes and its timing mode.  A re-run keeps what its first run took, but for its lanes:
static void claim_lanes_and_timing(rtuf_context* c, rtuf_context::Batch& b, const Route& route, int n_groups, bool rerun)
{
  if (!rerun) {
    b.route = route; b.dilation = route.post == Post::Dilate ? (int)c->params.silhouette_dilation_px : 0;
    b.lanes_used = 0;      // (a batch that is not split takes one lane, the next such batch the other: below)
    // mode 3 = mode 2 on every eighth batch only (each event costs ~5 us of stream time)
    b.timing = c->timing == 3 ? ((c->timing_seq++ & 7u) == 0 ? 2 : 0) : c->timing;
  }
  // (a re-run after the launch group shrank may need every lane where the first run needed one)
  if (n_groups > 1) for (int l = 0; l < std::min(c->n_lanes, n_groups); l++) b.lanes_used |= 1u << l;
  else if (!rerun) { b.lanes_used = 1u << c->next_lane; c->next_lane = (c->next_lane + 1) % c->n_lanes; }
  c->last_slot = (int)(&b - &c->batch[0]);
}

// The batch takes the staged poses -- the camera and link rings, every model's joint ring -- and only what the host changed
// since the last batch crosses the bus, on `sp`, the stream of the pose stage (with on-device forward kinematics that is
// just the joint positions).
static int upload_staged_poses(rtuf_context* c, rtuf_context::Batch& b, int n, bool rerun, hipStream_t sp)
{
  const size_t L = (size_t)std::max(c->n_links, 1); const bool more = n > b.uploaded_streams;
  // (a re-run after a bin regrowth finds this slot's device copies as its first run left them; its dirty flags may
  // already belong to setter calls made since, for the batch that comes next)
  if (!rerun) {
    b.cam_idx = take_staged(c, c->cam_ring, b, [](const rtuf_context::Batch& o) { return o.cam_idx; });
    b.link_idx = take_staged(c, c->link_ring, b, [](const rtuf_context::Batch& o) { return o.link_idx; });
    c->h_cams = c->ring_cams[c->cam_ring.write]; c->h_link_tf = c->ring_link_tf[c->link_ring.write];
    if (b.dirty_cams || more) HIP_TRY(c, hipMemcpyAsync(b.d_cams, c->ring_cams[b.cam_idx], sizeof(Camera) * n, hipMemcpyHostToDevice, sp));
    if (b.dirty_link_tf || more) HIP_TRY(c, hipMemcpyAsync(b.d_link_tf, c->ring_link_tf[b.link_idx], sizeof(double) * 16 * L * n, hipMemcpyHostToDevice, sp));
    b.dirty_cams = b.dirty_link_tf = false;
  }
  if (c->dirty_mask || n > c->mask_uploaded_streams) HIP_TRY(c, hipMemcpyAsync(c->d_model_mask, c->h_model_mask, sizeof(uint64_t) * n, hipMemcpyHostToDevice, sp));
  c->dirty_mask = false;
  b.uploaded_streams = std::max(b.uploaded_streams, n); c->mask_uploaded_streams = std::max(c->mask_uploaded_streams, n);
  // on-device forward kinematics overwrites the link matrices (and camera) of the streams that use it
  for (HostModel& m : c->models) {
    Kinematics& k = m.kin;
    if (!k.n_frames || !k.any_enabled) continue;
    const size_t mi = (size_t)(&m - &c->models[0]);
    if (b.q_idx.size() < c->models.size()) b.q_idx.resize(c->models.size(), 0);
    if (!rerun) {
      if (k.dirty_q) {                       // this batch takes the staged joint positions ...
        k.q_live = k.q_write; k.q_carried = false; k.dirty_q = false;
        // ... and later writes go to a buffer no batch in flight reads (kMaxInflight + 1 buffers: one is always free)
        k.q_write = free_set(c, b, k.q_live, [mi](const rtuf_context::Batch& o) { return mi < o.q_idx.size() ? o.q_idx[mi] : -1; });
      }
      b.q_idx[mi] = k.q_live;
    }
    if (k.dirty_aux || n > k.aux_uploaded_streams) {
      HIP_TRY(c, hipMemcpyAsync(k.d_root, k.h_root, sizeof(double) * 12 * (size_t)n, hipMemcpyHostToDevice, sp));
      HIP_TRY(c, hipMemcpyAsync(k.d_enabled, k.h_enabled, (size_t)n, hipMemcpyHostToDevice, sp));
    }
    k.dirty_aux = false; k.aux_uploaded_streams = std::max(k.aux_uploaded_streams, n);
  }
  return RTUF_OK;
}

// What the argument blocks of one launch group are filled from: the batch, the group's streams, lane and counter block, and
// the constants of the shading that every comparing kernel repeats.
struct GroupFill {
  const rtuf_context* c; const rtuf_context::Batch& b; const BatchRequest& r; const Route& route; const rtuf_context::Lane& ln;
  Counters* counters; int base, size; size_t plane;      // the group's block, its streams [base, base + size) of the batch, pixels per plane
  float sc_num, sc_off; int fast_div;
};
// the fields every block repeats
extern "C++" {
template <typename Args> static void set_group(Args& a, const GroupFill& f) { a.group_base = f.base; a.group_size = f.size; a.width = f.c->width; a.height = f.c->height; }
template <typename Args> static void set_input(Args& a, const float* depth, const GroupFill& f) { a.depth = depth; a.io_u16 = f.r.u16 ? 1 : 0; }
template <typename Args> static void set_shading(Args& a, const GroupFill& f)
{
  a.max_diff = f.c->params.depth_distance_threshold; a.replace_value = f.c->params.filter_replace_value; a.sc_num = f.sc_num; a.sc_off = f.sc_off; a.fast_div = f.fast_div;
}
// (the set-up and the tile kernel: the lane's bins)
template <typename Args> static void set_bins(Args& a, const GroupFill& f)
{
  a.bins = f.ln.d_bins; a.bin_hdr = f.ln.d_bin_hdr; a.fbins = f.ln.d_fbins; a.fbin_count = f.ln.d_fbin_count; a.fcapacity = f.c->fcapacity; a.capacity = f.c->capacity;
  a.big_list = f.ln.d_big_list; a.bg = f.b.d_bg; a.counters = f.counters; a.tiles_x = f.c->tiles_x; a.tiles_y = f.c->tiles_y; a.flags = f.c->params.flags;
}
// (the kernels that take the compare kernel's place: the outputs from the lane's z-surface)
template <typename Args> static void set_post(Args& a, const GroupFill& f)
{
  set_group(a, f); set_input(a, f.r.depth, f); set_shading(a, f);
  a.zsurface = f.ln.d_zsurface; a.masked = f.r.masked; a.mask = f.r.mask; a.bits = f.r.bits; a.counters = f.counters;
}
}  // extern "C++"

static void fill_setup(SetupArgs& sa, const GroupFill& f)
{
  const rtuf_context* c = f.c;
  set_group(sa, f); set_bins(sa, f);
  sa.cverts = c->d_cverts; sa.ctris = c->d_ctris; sa.corder = c->d_corder; sa.chunks = c->d_chunks; sa.mvp = f.b.d_mvp; sa.model_mask = c->d_model_mask;
  sa.clip_list = f.ln.d_clip_list; sa.clip_spill = f.ln.d_clip_spill; sa.big_capacity = c->big_capacity; sa.clip_capacity = c->clip_capacity;
  sa.n_draws = c->n_draws; sa.bg_chunk = c->bg_chunk; sa.items = f.ln.d_items[c->last_slot]; sa.n_chunks = c->n_chunks;
}
static void fill_tile(TileArgs& ta, const GroupFill& f)
{
  const rtuf_context* c = f.c; const BatchRequest& r = f.r; const TileVariant& tv = f.route.tile;
  set_group(ta, f); set_bins(ta, f); set_input(ta, r.depth, f); set_shading(ta, f);
  ta.masked = r.masked; ta.mask = r.mask; ta.zsurface = f.ln.d_zsurface;
  ta.z_near = c->params.near_plane; ta.z_far = c->params.far_plane; ta.key_shift = c->key_shift;
  ta.bits = tv.out == TileOut::Bits ? r.bits : nullptr; ta.labels = r.labels;
  ta.order_labels = tv.labels || tv.out == TileOut::Residual ? c->d_order_labels : nullptr;      // a label plane beside the outputs, or the rows of a residual table
  if (f.route.post == Post::Pad) {
    // link padding: the "label" of a winner is its link slot, and the plane is the lane's own, laid out like the z-surface
    // (slot 0 = stream `base`) where the tile kernel indexes its label plane by batch stream: biased by the group's base
    ta.order_labels = c->d_order_slot;
    ta.labels = f.ln.d_slots - (ptrdiff_t)f.base * (ptrdiff_t)f.plane;
  }
  ta.order_thr = tv.thresh ? c->d_order_thr : nullptr;      // (allocated once, rewritten in place: a re-run finds the same table)
  ta.virtual_out = r.virt; ta.empty_value = r.empty_value;
  ta.resid_table = reinterpret_cast<unsigned long long*>(r.resid); ta.n_labels = r.n_labels;
}
static void fill_pad(PadArgs& pd, const GroupFill& f) { set_post(pd, f); pd.slots = f.ln.d_slots; pd.slot_pad = f.c->d_slot_pad; pd.focal = f.c->d_pad_focal; }
static void fill_dilate(DilateArgs& da, const GroupFill& f) { set_post(da, f); da.radius = f.b.dilation; }
// (no group fields: the compare kernel takes the group's planes as one run of pixels)
static void fill_compare(CompareArgs& ca, const GroupFill& f)
{
  const size_t first = (size_t)f.base * f.plane * (f.r.u16 ? sizeof(uint16_t) : sizeof(float));      // the group's first plane, in bytes
  set_input(ca, reinterpret_cast<const float*>(reinterpret_cast<const char*>(f.r.depth) + first), f); set_shading(ca, f);
  ca.zsurface = f.ln.d_zsurface; ca.masked = reinterpret_cast<float*>(reinterpret_cast<char*>(f.r.masked) + first);
  ca.mask = f.r.mask ? f.r.mask + (size_t)f.base * f.plane : nullptr; ca.n_pixels = (size_t)f.size * f.plane;
  ca.z_near = f.c->params.near_plane; ca.z_far = f.c->params.far_plane;
}
static void fill_scene(SceneArgs& sc, const GroupFill& f)
{
  const rtuf_context* c = f.c; const BatchRequest& r = f.r; const bool planes_out = r.kind == Kind::Filter;
  set_group(sc, f); set_input(sc, r.depth, f);
  sc.scene = c->d_scene; sc.streams = c->d_scene_streams; sc.replace_value = c->params.filter_replace_value;
  sc.masked = planes_out ? r.masked : nullptr; sc.mask = planes_out ? r.mask : nullptr; sc.bits = planes_out ? nullptr : r.bits;
  // 16-byte accesses: every stream's plane (the planes form) or row (the bits form) starts on a 16-byte boundary
  const size_t per_lane = r.u16 ? 8u : 4u;
  sc.wide = aligned(r.depth, 16) && (planes_out ? f.plane % per_lane == 0 && aligned(r.masked, 16) && aligned(r.mask, 8) : (size_t)c->width % per_lane == 0) ? 1 : 0;
}
static void fill_cloud(CloudArgs& cl, const GroupFill& f)
{
  const BatchRequest& r = f.r; uint32_t* const rows = f.b.cl_rows; set_group(cl, f); set_input(cl, r.depth, f);
  cl.bits = r.bits; cl.intr = f.c->d_cloud_intr; cl.points = r.points; cl.index = r.index; cl.counts = r.counts; cl.capacity = r.capacity;
  cl.row_count = rows; cl.row_start = rows ? rows + (size_t)f.c->max_streams * f.c->height : nullptr;
}
static void fill_clearance(ClearanceArgs& cr, const GroupFill& f)
{
  const rtuf_context* c = f.c; const BatchRequest& r = f.r;
  // (the spheres of labels below n_labels: the list is sorted by label)
  int used = 0, slots = 0;
  while (used < (int)c->clr_spheres.size() && (int)(c->clr_spheres[(size_t)used].label_slot & 0xffffu) < r.n_labels) used++;
  while (slots < (int)c->clr_slot_label.size() && (int)c->clr_slot_label[(size_t)slots] < r.n_labels) slots++;
  set_group(cr, f); set_input(cr, r.depth, f);
  cr.bits = r.bits; cr.intr = c->d_cloud_intr; cr.spheres = c->d_clr_spheres; cr.slot_label = c->d_clr_slot_label;
  cr.cams = f.b.d_cams; cr.link_tf = f.b.d_link_tf; cr.model_mask = c->d_model_mask; cr.posed = f.b.clr_posed;
  cr.table = reinterpret_cast<unsigned long long*>(r.clr); cr.max_distance = r.max_distance;
  cr.n_spheres = used; cr.n_slots = slots; cr.n_links = std::max(c->n_links, 1); cr.n_labels = r.n_labels;
}
static void fill_points(PointsArgs& pt, const GroupFill& f)
{
  const BatchRequest& r = f.r; set_group(pt, f);
  pt.points = r.pt_points; pt.counts = r.pt_counts; pt.virt = r.virt; pt.intr = f.c->d_point_intr; pt.tf = f.c->d_point_tf;
  pt.verdict = r.pt_verdict; pt.pixel = r.pt_pixel; pt.summary = r.pt_summary;
  pt.capacity = r.capacity; pt.radius = r.pt_radius; pt.threshold = f.c->params.depth_distance_threshold;
  pt.wide = (r.capacity & 3) == 0 && aligned(r.pt_points, 16) && aligned(r.pt_verdict, 4) && (!r.pt_pixel || aligned(r.pt_pixel, 16)) ? 1 : 0;
}

// Fills the plan of the batch in place, and writes nothing else: the forward kinematics of every model that has one, the pose
// stage, and per launch group the argument blocks of the kernels its route has.  What no kernel of the route reads stays zero,
// padding included (the plan is hashed byte-wise, and the captured graphs are found by that hash).
static void build_plan(const rtuf_context* c, const rtuf_context::Batch& b, const Route& route, int n_groups, int per_group, int lane0, BatchPlan& plan)
{
  const BatchRequest& r = b.rq;
  const int n = r.n, L = std::max(c->n_links, 1);
  plan.route = route;
  for (const HostModel& m : c->models) {
    const Kinematics& k = m.kin;
    if (!k.n_frames || !k.any_enabled) continue;
    FkArgs fa;
    memset(&fa, 0, sizeof fa);               // (padding too: the plan is hashed byte-wise)
    fa.parent = k.d_parent; fa.depth = k.d_depth; fa.max_depth = k.max_depth; fa.joint_type = k.d_type; fa.joint_origin = k.d_origin; fa.joint_axis = k.d_axis;
    fa.link_frame = k.d_link_frame; fa.link_offset = k.d_link_offset; fa.q = k.h_q[b.q_idx[(size_t)(&m - &c->models[0])]]; fa.root_tf = k.d_root;
    fa.enabled = k.d_enabled; fa.link_tf = b.d_link_tf; fa.cams = b.d_cams; fa.n_links_total = L; fa.camera_frame = k.camera_frame;
    fa.n_streams = n; fa.n_frames = k.n_frames; fa.n_links_model = (int)m.links.size(); fa.link_base = m.link_base;
    plan.fks.push_back(fa);
  }
  // to_linear_depth's constants exactly as the shader evaluates them (include/shaders/urdf_filter.frag:14-17), in float, and
  // whether the kernels' per-pixel division by z - off may run as its eight-instruction core (div_core)
  const float sc_num = shade_num(c->params.near_plane, c->params.far_plane), sc_off = shade_off(c->params.near_plane, c->params.far_plane);
  const int fast_div = fast_div_admitted(sc_num, sc_off);
  PoseArgs& pa = plan.pa;
  memset(&pa, 0, sizeof pa);
  pa.cams = b.d_cams; pa.link_tf = b.d_link_tf; pa.draws = c->d_draws; pa.mvp = b.d_mvp;
  pa.bg = b.d_bg; pa.counters = b.d_counters; pa.n_counters = n_groups; pa.status = b.d_status;
  pa.sc_num = sc_num; pa.sc_off = sc_off; pa.max_diff = c->params.depth_distance_threshold;
  pa.n_streams = n; pa.n_draws = c->n_draws; pa.n_links = L; pa.z_far = c->params.far_plane; pa.width = c->width; pa.height = c->height;
  for (int g = 0, base = 0; base < n; g++, base += per_group) {
    plan.groups.emplace_back();
    BatchPlan::Group& gr = plan.groups.back();
    memset(static_cast<void*>(&gr), 0, sizeof gr);
    gr.lane = n_groups == 1 ? lane0 : g % c->n_lanes;
    const GroupFill f = {c, b, r, route, c->lane[gr.lane], b.d_counters + g, base, std::min(per_group, n - base), (size_t)c->width * c->height, sc_num, sc_off, fast_div};
    fill_setup(gr.sa, f); fill_tile(gr.ta, f);
    if (route.post == Post::Compare) fill_compare(gr.ca, f);
    if (route.post == Post::Dilate) fill_dilate(gr.da, f);
    if (route.post == Post::Pad) fill_pad(gr.pd, f);
    if (route.scene) fill_scene(gr.sc, f);
    if (route.tail == Tail::Cloud) fill_cloud(gr.cl, f);
    if (route.tail == Tail::Clearance) fill_clearance(gr.cr, f);
    if (route.tail == Tail::Points) fill_points(gr.pt, f);
  }
}

// Launches the plan: kernel by kernel (issue_plan; the pose stage on `sp`), or -- use_graph -- as the replay of a hipGraph
// captured once for these argument blocks on `st`, the stream of the batch's one lane.
static int launch_plan(rtuf_context* c, rtuf_context::Batch& b, const BatchPlan& plan, bool use_graph, hipStream_t st, hipStream_t sp)
{
  b.setup_grid.assign(plan.groups.size(), 0xffffffffu);
  // host-plane batches: the lanes' first kernels wait for the upload of the planes
  if (b.rq.wait_upload)
    for (int l = 0; l < c->n_lanes; l++)
      if (b.lanes_used >> l & 1u) HIP_TRY(c, hipStreamWaitEvent(c->lane[l].stream, b.uploaded, 0));
  if (!use_graph) { c->side_used_plain = true; return issue_plan(c, b, plan, sp, false); }
  // Small batch: its ~8 launches, two event operations and the cross-stream wait cost the host more than the GPU
  // spends on the kernels.  Capture them once per batch slot (pose stage forked onto the side stream inside the
  // graph; the set-up grid is the worst case, so no list-length estimate is baked in) and replay with one call.
  const uint64_t h = plan.hash();
  hipGraphExec_t exec = nullptr;
  for (auto& g : b.graphs) if (g.exec && g.hash == h) exec = g.exec;
  // A capture that has to evict a LIVE entry of the slot's cache is what thrashing looks like (a caller that never repeats
  // an argument set: fresh output buffers every frame); filling free entries -- the ring of staging buffers, the cover
  // pass going on and off, a regrowth -- is not.  Judged over windows of 64 batches, so a burst long ago does not count.
  if (exec) c->graph_hits++;
  else { c->graph_misses++; if (b.graphs[b.graph_next].exec) c->graph_evictions++; }
  if (((c->graph_hits + c->graph_misses) & 63u) == 0u) {
    if (c->graph_evictions > 32) c->graphs_ok = false;       // more than half of the window's batches captured over a live entry
    c->graph_evictions = 0;
  }
  if (!exec && c->graphs_ok) {
    hipGraph_t graph = nullptr;
    // (the side stream joins the capture below: it must not still carry plain launches of an earlier batch)
    if (c->side_used_plain) { hipStreamSynchronize(c->side); c->side_used_plain = false; }
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
    if (e == hipSuccess) {
      if (!c->fork_ev) hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming);
      hipEventRecord(c->fork_ev, st);
      hipStreamWaitEvent(c->side, c->fork_ev, 0);
      const int rc = issue_plan(c, b, plan, c->side, true);
      e = hipStreamEndCapture(st, &graph);
      if (rc != RTUF_OK) e = hipErrorUnknown;
    }
    if (e == hipSuccess && graph) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (graph) hipGraphDestroy(graph);
    if (e != hipSuccess || !exec) {
      // no graphs on this runtime: fall back to plain launches for the life of the context
      (void)hipGetLastError();
      exec = nullptr; c->graphs_ok = false;
    } else {
      auto& slot = b.graphs[b.graph_next];
      b.graph_next = (b.graph_next + 1) % rtuf_context::Batch::kGraphs;
      if (slot.exec) hipGraphExecDestroy(slot.exec);       // (not in flight: a slot's batches are retired before it is reused)
      slot.exec = exec; slot.hash = h;
    }
  }
  if (!exec) return issue_plan(c, b, plan, st, false);       // (everything on the main stream, as the graph would have run it)
  HIP_TRY(c, hipGraphLaunch(exec, st));
  b.setup_grid.assign(plan.groups.size(), 0xffffffffu);          // worst-case grid: the work list always fits
  return RTUF_OK;
}

static int enqueue_batch(rtuf_context* c, rtuf_context::Batch& b, bool rerun)
{
  const BatchRequest& r = b.rq; const int n = r.n;
  // Launch groups: as many as the lanes' bins ask for, alternating between the lanes; a batch that is not split takes one
  // lane, the next such batch the other.
  const int n_groups = groups_for(c, n);
  const int per_group = (n + n_groups - 1) / n_groups;
  // (checked before anything in the context or the slot changes: a refused batch leaves both as they were)
  if (n_groups > c->max_groups)
    return c->fail(RTUF_ERR_STATE, "internal: %d launch groups for %d streams, but counter blocks for %d", n_groups, n, c->max_groups);
  if ((n + per_group - 1) / per_group != n_groups)
    return c->fail(RTUF_ERR_STATE, "internal: %d launch groups planned, %d made (the status word counts the former down)", n_groups, (n + per_group - 1) / per_group);
  // The kernels of this batch, decided here for as long as it lives; a re-run takes what its first run took.  (The call asked
  // check_route of the same facts: a combination without a route, or with a variant the launcher has no kernel for, is a bug.)
  const Route route = rerun ? b.route : route_of(route_facts(c, r));
  if (!route.ok() || !tile_variant_legal(route.tile))
    return c->fail(RTUF_ERR_STATE, "internal: no kernel route for a batch of kind %d (tile variant %d)", (int)r.kind, tile_variant_index(route.tile));
  claim_lanes_and_timing(c, b, route, n_groups, rerun);
  const int lane0 = __builtin_ctz(b.lanes_used);
  hipStream_t st = c->lane[lane0].stream;        // (graph replay: single-lane contexts only)
  const bool use_graph = c->graphs_ok && c->n_lanes == 1 && !b.timing && n <= kGraphMaxStreams && n_groups == 1;
  // the pose stage of this batch runs on the side stream, concurrent with the raster kernels of the batch before it
  // (graph replay: everything hangs off the main stream, the side stream is forked inside the graph)
  hipStream_t sp = use_graph ? st : c->side;
  { const int rc = upload_staged_poses(c, b, n, rerun, sp); if (rc != RTUF_OK) return rc; }
  BatchPlan plan;
  build_plan(c, b, route, n_groups, per_group, lane0, plan);
  b.n_groups = (int)plan.groups.size();          // (= n_groups: the plan has ceil(n / per_group) groups, checked above)
  if (may_write_zsurface(r)) c->last_lane = plan.groups.back().lane;
  { const int rc = launch_plan(c, b, plan, use_graph, st, sp); if (rc != RTUF_OK) return rc; }
  for (int l = 0; l < c->n_lanes; l++)
    if (b.lanes_used >> l & 1u) HIP_TRY(c, hipEventRecord(b.done[l], c->lane[l].stream));
  HIP_TRY(c, hipGetLastError());
  return RTUF_OK;
}

// Copies n planes of `stride` bytes between a packed device buffer and the caller's planes (kind: which way), on *stream --
// or, stream == nullptr, with the synchronous hipMemcpy.  Consecutive host planes go as one transfer; a plane whose host
// pointer is nullptr is skipped (byte masks only some streams asked for).
static int copy_planes(rtuf_context* c, const void* dev, void* const* host, int n, size_t stride, hipMemcpyKind kind, const hipStream_t* stream)
{
  for (int s = 0; s < n;) {
    if (!host[s]) { s++; continue; }
    int e = s + 1;
    while (e < n && host[e] && (char*)host[e] == (char*)host[e - 1] + stride) e++;
    void* const d = (char*)dev + (size_t)s * stride;
    void* const dst = kind == hipMemcpyHostToDevice ? d : host[s];
    const void* const src = kind == hipMemcpyHostToDevice ? host[s] : d;
    if (stream) HIP_TRY(c, hipMemcpyAsync(dst, src, (size_t)(e - s) * stride, kind, *stream));
    else HIP_TRY(c, hipMemcpy(dst, src, (size_t)(e - s) * stride, kind));
    s = e;
  }
  return RTUF_OK;
}

// Copies the results of a host-plane batch from the slot's staging (where the request points) to the caller's planes on the
// download stream, after the batch's kernels.  (Not the clouds: their download is synchronous, download_cloud.)
static int enqueue_download(rtuf_context* c, rtuf_context::Batch& b)
{
  const BatchRequest& r = b.rq;
  const size_t plane = (size_t)c->width * c->height;
  const size_t esz = r.u16 ? sizeof(uint16_t) : sizeof(float);
  for (int l = 0; l < c->n_lanes; l++)
    if (b.lanes_used >> l & 1u) HIP_TRY(c, hipStreamWaitEvent(c->d2h, b.done[l], 0));
  auto down = [&](const void* dev, const std::vector<void*>& host, size_t stride) { return copy_planes(c, dev, host.data(), r.n, stride, hipMemcpyDeviceToHost, &c->d2h); };
  int rc = RTUF_OK;
  switch (r.kind) {
    case Kind::Residual:                     // the table is all that comes back
      HIP_TRY(c, hipMemcpyAsync(b.h_table, r.resid, (size_t)r.n * (size_t)r.n_labels * sizeof(rtuf_link_residuals), hipMemcpyDeviceToHost, c->d2h));
      break;
    case Kind::Bits: rc = down(r.bits, b.h_out, rtuf_mask_bits_words(c->width, c->height) * sizeof(uint32_t)); break;
    case Kind::Render: rc = down(r.virt, b.h_out, plane * esz); break;
    case Kind::Filter:
      rc = down(r.masked, b.h_out, plane * esz);
      if (rc == RTUF_OK) rc = down(r.mask, b.h_mask, plane);
      break;
    case Kind::Cloud: case Kind::Clearance: case Kind::Points: break;
  }
  if (rc == RTUF_OK && r.labels) rc = down(r.labels, b.h_labels, plane * sizeof(uint16_t));
  if (rc != RTUF_OK) return rc;
  HIP_TRY(c, hipEventRecord(b.downloaded, c->d2h));
  return RTUF_OK;
}

// ---- the steps of retire_oldest ----
// What the launch groups of a batch counted, summed over groups and shards, and which of the context's lists that outgrew.
struct BatchTotals {
  unsigned long long tris_binned = 0, bin_entries = 0, clip_count = 0, frags = 0, occluded = 0, raster_atomics = 0, drawn_pixels = 0, work_items = 0;
  unsigned max_bin_fill = 0, max_fbin_fill = 0, clip_overflow = 0, uncovered = 0, max_big_fill = 0, cover_tiles = 0, exact_tiles = 0, zero_items = 0, max_items = 0;
  bool list_over = false;                    // some group's set-up grid was sized too small for its work list
  bool bin_over = false, big_over = false;   // (the clip list: clip_overflow)
  bool overflowed() const { return bin_over || clip_overflow || list_over || big_over; }
};
static BatchTotals sum_counters(rtuf_context* c, const rtuf_context::Batch& b)
{
  BatchTotals k;
#ifdef RTUF_LANECOUNT
  for (int i = 0; i < kLaneLoops; i++) c->lane_slots[i] = c->lane_live[i] = 0;
  for (int i = 0; i < kLaneRoleWords; i++) c->lane_roles[i] = 0;
  for (int g = 0; g < b.n_groups; g++)
    for (int sh = 0; sh < kCounterShards; sh++) {
      for (int i = 0; i < kLaneLoops; i++) { c->lane_slots[i] += b.h_counters[g].shard[sh].lane_slots[i]; c->lane_live[i] += b.h_counters[g].shard[sh].lane_live[i]; }
      for (int i = 0; i < kLaneRoleWords; i++) c->lane_roles[i] += b.h_counters[g].shard[sh].lane_roles[i];
    }
#endif
  for (int g = 0; g < b.n_groups; g++) {
    const Counters& cn = b.h_counters[g];
    k.work_items += cn.work.n_items; k.max_items = std::max(k.max_items, cn.work.n_items);
    k.list_over = k.list_over || cn.work.n_items > b.setup_grid[g];
    for (int i = 0; i < kCounterShards; i++) {
      const CounterShard& sh = cn.shard[i];
      k.tris_binned += sh.tris_binned; k.bin_entries += sh.bin_entries; k.clip_count += sh.clip_count;
      k.max_bin_fill = std::max(k.max_bin_fill, sh.max_bin_fill); k.clip_overflow |= sh.clip_overflow;
      k.max_fbin_fill = std::max(k.max_fbin_fill, sh.max_fbin_fill); k.frags += sh.frags; k.uncovered |= sh.uncovered;
      k.max_big_fill = std::max(k.max_big_fill, sh.max_big_fill); k.raster_atomics += sh.raster_atomics; k.drawn_pixels += sh.drawn_pixels;
      k.occluded += sh.occluded; k.cover_tiles += sh.cover_tiles; k.exact_tiles += sh.exact_tiles; k.zero_items += sh.zero_items;
    }
  }
  k.bin_over = k.max_bin_fill > c->capacity || k.max_fbin_fill > c->fcapacity; k.big_over = k.max_big_fill > c->big_capacity;
  return k;
}

// The totals become rtuf_stats and the hints that size the next batches' set-up grids (first_run: of the batch being retired).
static void publish_stats(rtuf_context* c, const rtuf_context::Batch& b, const BatchTotals& k, bool first_run)
{
  const int group_streams = (b.rq.n + b.n_groups - 1) / std::max(b.n_groups, 1);
  c->items_hint = k.max_items;               // sizes the next batches' set-up grids (the longest list of this batch's groups ...
  c->items_hint_streams = group_streams;     // ... of so many streams each)
  c->group_items.resize((size_t)b.n_groups); c->group_streams.resize((size_t)b.n_groups);
  for (int g = 0; g < b.n_groups; g++) {
    c->group_items[(size_t)g] = b.h_counters[g].work.n_items;
    c->group_streams[(size_t)g] = std::min(group_streams, b.rq.n - g * group_streams);
  }
  c->stats.triangles_submitted = (uint64_t)c->n_tris * (uint64_t)b.rq.n;
  c->stats.triangles_binned = k.tris_binned; c->stats.bin_entries = k.bin_entries; c->stats.triangles_clipped = k.clip_count;
  c->stats.max_bin_fill = k.max_bin_fill; c->stats.bin_capacity = c->capacity; c->stats.fragments_binned = k.frags; c->stats.max_fbin_fill = k.max_fbin_fill;
  c->stats.occluded_entries = k.occluded; c->stats.cover_tiles = k.cover_tiles; c->stats.exact_tiles = k.exact_tiles;
  c->stats.work_items = (uint32_t)std::min<unsigned long long>(k.work_items, 0xffffffffu); c->stats.zero_survivor_items = k.zero_items;
  c->stats.raster_atomics = k.raster_atomics; c->stats.drawn_pixels = k.drawn_pixels;
  c->stats.cover_pass = b.route.tile.cover ? 1u : 0u; c->stats.groups_last_batch = (uint32_t)b.n_groups;
  if (k.list_over) c->stats.regrowths++;
  // host mirror of the device status word (rtuf_batch_status_device): what the FIRST run of the batch being retired left there
  if (first_run) {
    c->stats.batch_status = (k.bin_over ? kStatusBinOverflow : 0u) | (k.clip_overflow ? kStatusClipOverflow : 0u) | (k.big_over ? kStatusBigOverflow : 0u) |
                            (k.list_over ? kStatusGridShort : 0u) | (k.uncovered ? kStatusUncovered : 0u);
    c->stats.batch_reruns = 0;
  }
}

// the timing events of a timed batch become ms_* and sum_ms_*
static void read_timing(rtuf_context* c, const rtuf_context::Batch& b)
{
  if (!b.timing || b.events.size() < (size_t)(kEvGroup0 + kEvPerGroup * b.n_groups)) return;
  // per launch group E0 .. E4 (see issue_plan).  With several lanes the kernels of different groups overlap: the sums
  // below add up per-launch durations, they are not wall time.
  const bool behind = runs_behind_tile(b.route);      // ms_compare: whatever ran behind the tile kernel
  auto el = [&](size_t i, size_t j) { float ms = 0; hipEventElapsedTime(&ms, b.events[i], b.events[j]); return ms; };
  c->stats.ms_pose = c->stats.ms_setup = c->stats.ms_clip = c->stats.ms_raster = c->stats.ms_compare = c->stats.ms_total = 0;
  for (int g = 0; g < b.n_groups; g++) {
    const size_t e0 = kEvGroup0 + kEvPerGroup * (size_t)g;
    if (b.timing == 1) c->stats.ms_setup += el(e0, e0 + 2);
    else { c->stats.ms_setup += el(e0, e0 + 1); c->stats.ms_clip += el(e0 + 1, e0 + 2); }
    c->stats.ms_raster += el(e0 + 2, e0 + 3); if (behind) c->stats.ms_compare += el(e0 + 3, e0 + 4);
  }
  if (b.timing == 1) {
    c->stats.ms_pose = el(kEvStart, kEvPoseEnd);
    for (int l = 0; l < c->n_lanes; l++)
      if (b.lanes_used >> l & 1u) c->stats.ms_total = std::max(c->stats.ms_total, el(kEvStart, kEvLaneEnd + l));
  }
  c->acc_ms[0] += c->stats.ms_pose; c->acc_ms[1] += c->stats.ms_setup; c->acc_ms[2] += c->stats.ms_raster;
  c->acc_ms[3] += c->stats.ms_compare; c->acc_ms[4] += c->stats.ms_total; c->acc_ms[5] += c->stats.ms_clip;
  c->stats.timed_batches = ++c->acc_batches;
  c->stats.sum_ms_pose = c->acc_ms[0]; c->stats.sum_ms_setup = c->acc_ms[1]; c->stats.sum_ms_raster = c->acc_ms[2];
  c->stats.sum_ms_compare = c->acc_ms[3]; c->stats.sum_ms_total = c->acc_ms[4]; c->stats.sum_ms_clip = c->acc_ms[5];
}

// The clean exit: nothing overflowed, the batch is done and its slot free.
static int retire_clean(rtuf_context* c, rtuf_context::Batch& b, const BatchTotals& k)
{
  if (b.host_io) HIP_TRY(c, hipEventSynchronize(b.downloaded));
  read_timing(c, b);
  if (b.route.tile.cover) {
    if (k.cover_tiles) c->cover_idle = 0;
    else if (++c->cover_idle >= 3) { c->cover_on = false; c->cover_sleep = 64; c->cover_idle = 2; }      // (idle = 2: one empty probe sends it back to sleep)
  } else if (--c->cover_sleep <= 0) {
    c->cover_on = true;
  }
  b.active = false; c->oldest = (c->oldest + 1) % kMaxInflight; c->pending--;      // the slot is free
  if (b.rq.kind == Kind::Cloud && k.uncovered)
    return c->fail(RTUF_ERR_STATE, "point cloud: a stream's background quad does not cover its whole image (non-standard projection), so the mask bits the cloud is "
                                   "built on are undefined there; there is no cloud form for this camera (filter with the full-plane calls and convert the masked plane)");
  if (b.rq.kind == Kind::Clearance && k.uncovered)
    return c->fail(RTUF_ERR_STATE, "link clearance: a stream's background quad does not cover its whole image (non-standard projection), so the "
                                   "mask bits the kept points are taken from are undefined there");
  if (b.rq.kind == Kind::Bits && k.uncovered)
    return c->fail(RTUF_ERR_STATE, "mask bits: a stream's background quad does not cover its whole image (non-standard projection), so "
                                   "masked depth != select(bit, replace, sensor) there; use the full-plane calls for this camera");
  return RTUF_OK;
}

// drops everything in flight (nothing of it can be run again) and hands the error on
static int drop_in_flight(rtuf_context* c, int rc) { for (auto& o : c->batch) o.active = false; c->pending = 0; return rc; }

// The overflow path: waits for the later batches too, enlarges what overflowed, and runs everything in flight again in order.
static int regrow_and_rerun(rtuf_context* c, const BatchTotals& k)
{
  sync_lanes(c);
  if (c->d2h) HIP_TRY(c, hipStreamSynchronize(c->d2h));
  if (k.bin_over) { const int rc = grow_bins(c, k.max_bin_fill, k.max_fbin_fill); if (rc != RTUF_OK) return drop_in_flight(c, rc); }
  if (k.clip_overflow) {
    const uint32_t larger = c->clip_capacity * 4;
    for (int l = 0; l < c->n_lanes; l++) {
      int rc = regrow(c, c->lane[l].d_clip_list, (size_t)larger * kCounterShards * sizeof(ClipItem), "clip list");
      if (rc == RTUF_OK && clip_spill_bytes(larger) != clip_spill_bytes(c->clip_capacity)) { rc = regrow(c, c->lane[l].d_clip_spill, clip_spill_bytes(larger), "clip spill area"); c->stats.regrowths--; }
      if (rc != RTUF_OK) return drop_in_flight(c, rc);
      if (l) c->stats.regrowths--;           // (one regrowth, however many lanes)
    }
    c->clip_capacity = larger;
  }
  if (k.big_over) {
    // (half as much again as this run asked for: poses move, and a list that just fits overflows on the next batch)
    uint32_t larger = c->big_capacity;
    while (larger < k.max_big_fill + k.max_big_fill / 2) larger *= 2;
    for (int l = 0; l < c->n_lanes; l++) {
      const int rc = regrow(c, c->lane[l].d_big_list, (size_t)larger * kCounterShards * sizeof(BigRec), "many-tile list");
      if (rc != RTUF_OK) return drop_in_flight(c, rc);
      if (l) c->stats.regrowths--;
    }
    c->big_capacity = larger;
  }
  const size_t tiles = (size_t)c->tiles_x * c->tiles_y;
  for (int l = 0; l < c->n_lanes; l++) {
    // (the arrays were sized for the launch group the context started with: at least the present one)
    launch_init_headers(c->lane[l].d_bin_hdr, (size_t)c->group * tiles, c->lane[l].stream);
    HIP_TRY(c, hipMemsetAsync(c->lane[l].d_fbin_count, 0, (size_t)c->group * tiles * sizeof(uint32_t), c->lane[l].stream));
  }
  // (a grid that was too short: the re-run takes the worst-case grid, which no list can outgrow -- the estimate that failed
  // once would size the same grid again)
  c->force_worst_grid = k.list_over; c->stats.batch_reruns++;
  int rc = RTUF_OK;
  for (int i = 0; i < c->pending && rc == RTUF_OK; i++) {
    rtuf_context::Batch& r = c->batch[(c->oldest + i) % kMaxInflight];
    rc = enqueue_batch(c, r, true);
    if (rc == RTUF_OK && r.host_io) rc = enqueue_download(c, r);
  }
  c->force_worst_grid = false;
  return rc == RTUF_OK ? rc : drop_in_flight(c, rc);
}

// Retires the oldest batch in flight: waits for it, reads its counters, and if a bin or the clip list
// overflowed, enlarges them and runs that batch and every later one again (their inputs are intact).
static int retire_oldest(rtuf_context* c)
{
  for (int attempt = 0; attempt < 8; attempt++) {
    rtuf_context::Batch& b = c->batch[c->oldest];
    if (!c->pending || !b.active) { c->pending = 0; return RTUF_OK; }
    for (int l = 0; l < c->n_lanes; l++)
      if (b.lanes_used >> l & 1u) HIP_TRY(c, hipEventSynchronize(b.done[l]));
    const BatchTotals k = sum_counters(c, b);
    publish_stats(c, b, k, attempt == 0);
    if (!k.overflowed()) return retire_clean(c, b, k);
    const int rc = regrow_and_rerun(c, k);
    if (rc != RTUF_OK) return rc;
  }
  return drop_in_flight(c, c->fail(RTUF_ERR_CAPACITY, "tile bins still overflow after regrowth"));
}

// ---- submission -----------------------------------------------------------------------
// streams 0 .. n - 1 have their intrinsics (table: the one the caller's kernels read, d_cloud_intr or d_point_intr; the setter writes both)
static int need_intrinsics(rtuf_context* c, int n, const void* table)
{
  for (int s = 0; s < n; s++)
    if (!table || !c->cloud_intr_set[(size_t)s]) return c->fail(RTUF_ERR_STATE, "stream %d has no cloud intrinsics (rtuf_set_cloud_intrinsics)", s);
  return RTUF_OK;
}

// max_streams bits planes (rtuf_mask_bits_words each): what a buffer of the library's own holds that a mask-bits batch writes
static size_t bits_planes_bytes(const rtuf_context* c) { return (size_t)c->max_streams * rtuf_mask_bits_words(c->width, c->height) * sizeof(uint32_t); }
static int ensure_bits_planes(rtuf_context* c, uint32_t*& p) { if (!p) HIP_TRY(c, dev_alloc(c, &p, bits_planes_bytes(c))); return RTUF_OK; }

// The calls of their own (learning a scene, the voxel inserts and carves) and some setters run a kernel on lane 0 and wait.
static int wait_lane0(rtuf_context* c) { HIP_TRY(c, hipStreamSynchronize(c->lane[0].stream)); return RTUF_OK; }
static int finish_on_lane0(rtuf_context* c) { const int rc = wait_lane0(c); if (rc == RTUF_OK) HIP_TRY(c, hipGetLastError()); return rc; }

// While link padding is in effect a margin in metres is projected with the stream's focal length: every stream of a batch needs
// its intrinsics (no rule of the route: asked before anything is staged or enqueued).
static int need_pad_intrinsics(rtuf_context* c, int n) { return c->pad_models > 0 ? need_intrinsics(c, n, c->d_cloud_intr) : RTUF_OK; }

static int check_u16_width(rtuf_context* c, bool u16) { return u16 && (c->width & 3) ? c->fail(RTUF_ERR_INVALID, "16UC1 path needs a width that is a multiple of 4") : RTUF_OK; }
// What every batch call checks first: the models are final, n is in range and the arrays the call cannot do without are there
// (have_args) and -- u16: the filter calls; the kinds that test something of their own first call check_u16_width after it -- the 16UC1 width.
static int check_batch_call(rtuf_context* c, int n, bool have_args, bool u16)
{
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (n <= 0 || n > c->max_streams || !have_args) return c->fail(RTUF_ERR_INVALID, "bad batch arguments (n=%d)", n);
  return check_u16_width(c, u16);
}

// What every filter call checks, with a label plane (labels: the caller's plane, or its array of planes) or without: the
// arguments, then the route, and only then the label table is built.
static int ensure_label_table(rtuf_context* c);
static int check_filter_call(rtuf_context* c, int n, bool have_args, const void* labels, bool u16)
{
  { const int rc = check_batch_call(c, n, have_args, u16); if (rc != RTUF_OK) return rc; }
  BatchRequest rq(Kind::Filter, n, u16);
  rq.labels = static_cast<uint16_t*>(const_cast<void*>(labels));
  { const int rc = check_route(c, rq); if (rc != RTUF_OK) return rc; }
  return labels ? ensure_label_table(c) : RTUF_OK;
}

// The slot of the next batch: once the ring has room for it (the oldest batches are retired as needed), the one behind the
// newest batch in flight.  Called once per batch, before anything of the slot is touched.
static int take_slot(rtuf_context* c, rtuf_context::Batch*& slot)
{
  if (c->broken) return c->fail(RTUF_ERR_STATE, "context unusable: a bin regrowth failed (%s)", c->error.c_str());
  hipSetDevice(c->device);
  // two-kernel mode and silhouette dilation keep one z-surface per lane: their batches do not overlap
  const int limit = uses_zsurface(c) ? 1 : kMaxInflight;
  while (c->pending >= limit) { const int rc = retire_oldest(c); if (rc != RTUF_OK) return rc; }
  slot = &c->batch[(c->oldest + c->pending) % kMaxInflight];
  return RTUF_OK;
}

// Enqueues the request in the slot take_slot gave: the slot keeps the record, and is in flight when this returns RTUF_OK.  A
// cloud batch gets the slot's own bits buffer and row scratch here, a clearance batch the bits buffer and its posed spheres.
static int submit_batch(rtuf_context* c, rtuf_context::Batch& b, const BatchRequest& rq)
{
  if (rq.kind == Kind::Cloud || rq.kind == Kind::Clearance) { const int rc = ensure_bits_planes(c, b.cl_bits); if (rc != RTUF_OK) return rc; }
  if (rq.kind == Kind::Cloud && rq.capacity && !b.cl_rows) HIP_TRY(c, dev_alloc(c, &b.cl_rows, 2u * (size_t)c->max_streams * (size_t)c->height * sizeof(uint32_t)));
  if (rq.kind == Kind::Clearance && b.clr_posed_have < c->clr_spheres.size()) {
    dev_free(c, b.clr_posed);
    b.clr_posed_have = 0;
    HIP_TRY(c, dev_alloc(c, &b.clr_posed, (size_t)c->max_streams * c->clr_spheres.size() * sizeof(float4)));
    b.clr_posed_have = c->clr_spheres.size();
  }
  if (rq.kind == Kind::Points && !b.pt_plane)
    HIP_TRY(c, dev_alloc(c, &b.pt_plane, (size_t)c->max_streams * c->width * c->height * sizeof(float)));
  if (uses_zsurface(c) && may_write_zsurface(rq))
    for (int l = 0; l < c->n_lanes; l++)
      if (!c->lane[l].d_zsurface) HIP_TRY(c, dev_alloc(c, &c->lane[l].d_zsurface, (size_t)c->group * c->width * c->height * sizeof(float)));
  if (c->pad_models > 0 && may_write_zsurface(rq))
    for (int l = 0; l < c->n_lanes; l++)
      if (!c->lane[l].d_slots) HIP_TRY(c, dev_alloc(c, &c->lane[l].d_slots, (size_t)c->group * c->width * c->height * sizeof(uint16_t)));
  b.rq = rq;
  if (rq.kind == Kind::Cloud || rq.kind == Kind::Clearance) b.rq.bits = b.cl_bits;
  if (rq.kind == Kind::Points) { b.rq.virt = b.pt_plane; b.rq.empty_value = INFINITY; }
  b.host_io = false;
  const int rc = enqueue_batch(c, b, false);
  if (rc == RTUF_OK) { b.active = true; c->pending++; }
  return rc;
}

// a batch on the caller's device buffers
static int submit_device(rtuf_context* c, const BatchRequest& rq)
{
  { const int rc = need_pad_intrinsics(c, rq.n); if (rc != RTUF_OK) return rc; }
  rtuf_context::Batch* b = nullptr;
  const int rc = take_slot(c, b);
  return rc != RTUF_OK ? rc : submit_batch(c, *b, rq);
}

static BatchRequest filter_request(int n, const void* d_depth, void* d_masked, uint8_t* d_mask, uint16_t* d_labels, bool u16)
{
  BatchRequest rq(Kind::Filter, n, u16);
  rq.depth = static_cast<const float*>(d_depth); rq.masked = static_cast<float*>(d_masked); rq.mask = d_mask; rq.labels = d_labels;
  return rq;
}
static BatchRequest bits_request(int n, const void* d_depth, uint32_t* d_bits, bool u16)
{
  BatchRequest rq(Kind::Bits, n, u16);
  rq.depth = static_cast<const float*>(d_depth); rq.bits = d_bits;
  return rq;
}

int rtuf_filter_batch_device(rtuf_context* c, int n, const float* d_depth, float* d_masked, uint8_t* d_mask)
{
  KIDS_NEXT(c, rtuf_filter_batch_device(k, n, d_depth, d_masked, d_mask));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_filter_call(c, n, d_depth && d_masked, nullptr, false);
  return rc != RTUF_OK ? rc : submit_device(c, filter_request(n, d_depth, d_masked, d_mask, nullptr, false));
}

int rtuf_filter_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth, uint16_t* d_masked, uint8_t* d_mask)
{
  KIDS_NEXT(c, rtuf_filter_batch_device_u16(k, n, d_depth, d_masked, d_mask));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_filter_call(c, n, d_depth && d_masked, nullptr, true);
  return rc != RTUF_OK ? rc : submit_device(c, filter_request(n, d_depth, d_masked, d_mask, nullptr, true));
}

// the mask-bits calls, and the learn-scene calls, whose batch is one
static int check_bits_call(rtuf_context* c, int n, const void* in, const void* out, bool u16)
{
  { const int rc = check_batch_call(c, n, in && out, false); if (rc != RTUF_OK) return rc; }
  if (c->width & 3) return c->fail(RTUF_ERR_INVALID, "mask-bits output needs a width that is a multiple of 4");
  return check_route(c, BatchRequest(Kind::Bits, n, u16));
}

size_t rtuf_mask_bits_words(int width, int height)
{
  return (width > 0 && height > 0) ? (size_t)height * (size_t)((width + 31) / 32) : 0;
}

int rtuf_filter_batch_device_bits(rtuf_context* c, int n, const float* d_depth, uint32_t* d_bits)
{
  KIDS_NEXT(c, rtuf_filter_batch_device_bits(k, n, d_depth, d_bits));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_bits_call(c, n, d_depth, d_bits, false);
  return rc != RTUF_OK ? rc : submit_device(c, bits_request(n, d_depth, d_bits, false));
}

int rtuf_filter_batch_device_bits_u16(rtuf_context* c, int n, const uint16_t* d_depth, uint32_t* d_bits)
{
  KIDS_NEXT(c, rtuf_filter_batch_device_bits_u16(k, n, d_depth, d_bits));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_bits_call(c, n, d_depth, d_bits, true);
  return rc != RTUF_OK ? rc : submit_device(c, bits_request(n, d_depth, d_bits, true));
}

// Host side of the mask-bits calls: masked depth / byte mask of one frame from its sensor plane and its mask bits,
// with the arithmetic of the kernels (a pure select; for 16UC1 the reference's two convertTo roundings, see
// metres_to_u16 in rtuf_kernels.hip).  No GPU involved.
int rtuf_expand_mask_bits(const void* depth_in, int is_u16, const uint32_t* bits, int width, int height, float replace_value,
                          void* masked_out, uint8_t* mask_out)
{
  if (!depth_in || !bits || width <= 0 || height <= 0 || (!masked_out && !mask_out)) return RTUF_ERR_INVALID;
  const int row_words = (width + 31) / 32;
  uint16_t rep16 = 0;
  if (is_u16) {
    const float v = replace_value * 1000.0f;
    if (v >= -2147483648.0f && v < 2147483648.0f) { const long r = lrintf(v); rep16 = (uint16_t)(r < 0 ? 0 : (r > 65535 ? 65535 : r)); }
  }
  for (int y = 0; y < height; y++) {
    const uint32_t* wrow = bits + (size_t)y * row_words;
    const size_t o = (size_t)y * width;
    for (int x = 0; x < width; x++) {
      const bool f = (wrow[x >> 5] >> (x & 31)) & 1u;
      if (mask_out) mask_out[o + x] = f ? 255 : 0;
      if (!masked_out) continue;
      if (is_u16) {
        const uint16_t u = static_cast<const uint16_t*>(depth_in)[o + x];
        uint16_t r = rep16;
        if (!f) {                              // float(u) * 0.001f * 1000.0f, rounded half to even and saturated, like the kernels
          const float m = (float)u * 0.001f;
          const float v = m * 1000.0f;
          const long q = lrintf(v);
          r = (uint16_t)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
        }
        static_cast<uint16_t*>(masked_out)[o + x] = r;
      } else {
        static_cast<float*>(masked_out)[o + x] = f ? replace_value : static_cast<const float*>(depth_in)[o + x];
      }
    }
  }
  return RTUF_OK;
}

int rtuf_sync(rtuf_context* c)
{
  if (!c) return RTUF_ERR_INVALID;
  if (!c->kids.empty()) {
    // every kid is synchronised even if one fails (the first failure is reported)
    int first_rc = RTUF_OK;
    c->order.clear();
    for (rtuf_context* k : c->kids) { const int rc = rtuf_sync(k); if (rc < 0 && first_rc == RTUF_OK) { first_rc = rc; c->error = k->error; } }
    return first_rc;
  }
  hipSetDevice(c->device);
  while (c->pending) { const int rc = retire_oldest(c); if (rc != RTUF_OK) return rc; }
  for (int l = 0; l < c->n_lanes; l++) HIP_TRY(c, hipStreamSynchronize(c->lane[l].stream));
  return RTUF_OK;
}

void* rtuf_stream(rtuf_context* c) { return (c && c->kids.empty() && c->n_lanes == 1) ? (void*)c->lane[0].stream : nullptr; }

int rtuf_batch_status_device(rtuf_context* c, const uint32_t** d_status)
{
  if (!c || !d_status) return RTUF_ERR_INVALID;
  if (!c->kids.empty()) c = c->kids[c->last_kid];
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  *d_status = c->batch[c->last_slot].d_status;
  return RTUF_OK;
}

int rtuf_order_stream_after_batches(rtuf_context* c, void* hip_stream)
{
  KIDS_ALL(c, rtuf_order_stream_after_batches(k, hip_stream));
  if (!c) return RTUF_ERR_INVALID;
  hipSetDevice(c->device);
  hipStream_t user = static_cast<hipStream_t>(hip_stream);
  for (const auto& b : c->batch) {
    if (!b.active) continue;
    for (int l = 0; l < c->n_lanes; l++)
      if (b.lanes_used >> l & 1u) HIP_TRY(c, hipStreamWaitEvent(user, b.done[l], 0));
    if (b.host_io && b.downloaded) HIP_TRY(c, hipStreamWaitEvent(user, b.downloaded, 0));
  }
  return RTUF_OK;
}

// ---- host planes -----------------------------------------------------------------------------------
// The reference's filter() takes a host buffer and leaves host results (src/urdf_filter.cpp:233-234,
// :729-735).  Here the planes of a batch go up on one copy stream and come back on another, so with two
// batches in flight the transfers of one overlap the kernels of the other; every slot has its own
// device staging.
// (copy streams beside the lanes as well: an upload queued behind a lane's kernels would hold up the next batch)
static int ensure_copy_streams(rtuf_context* c)
{
  if (c->h2d && c->d2h) return RTUF_OK;
  bool beside = true;
  sync_lanes(c);                      // (the probe times idle kernels: nothing else may be running; first host-plane call only)
  bool beside_up = true;
  if (!c->h2d) HIP_TRY(c, create_stream_beside(lane_streams(c), &c->h2d, &beside_up));
  if (!c->d2h) HIP_TRY(c, create_stream_beside(lane_streams(c), &c->d2h, &beside));
  c->stats.copy_streams_side_by_side = (beside && beside_up) ? 1u : 0u;
  return RTUF_OK;
}

// grow-only device staging of a slot: *ptr holds `have` units of bytes_per bytes and is replaced when `need` are asked for
static int ensure_staging(rtuf_context* c, char*& ptr, size_t& have, size_t need, size_t bytes_per)
{
  if (have >= need) return RTUF_OK;
  dev_free(c, ptr);
  have = 0;
  HIP_TRY(c, dev_alloc(c, &ptr, need * bytes_per));
  have = need;
  return RTUF_OK;
}

// The caller's side of a host-plane batch: n host pointers per array, nullptr for what the kind or the call does not have.
struct HostPlanes {
  const void* const* depth;          // sensor planes: go up (not Render)
  void* const* out;                  // masked / bits / virtual / points planes
  void* const* mask;                 // Filter: byte masks (nullptr, or any entry nullptr: not wanted)
  void* const* labels;               // Filter, Render
  void* const* index; uint32_t* counts;      // compacted Cloud
  rtuf_link_residuals* table;        // Residual
  rtuf_link_clearance* clr_table;    // Clearance
};

// the results of a host-plane cloud batch, synchronous: once the batch is retired -- re-runs included -- the organized planes
// come down whole; the compacted forms bring the counts down first and then only min(counts, capacity) entries per stream
static int download_cloud(rtuf_context* c, const BatchRequest& r, const HostPlanes& hp)
{
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }
  const size_t per = r.capacity ? (size_t)r.capacity : (size_t)c->width * c->height;      // entries per stream
  if (!r.capacity) return copy_planes(c, r.points, hp.out, r.n, per * 3u * sizeof(float), hipMemcpyDeviceToHost, nullptr);
  HIP_TRY(c, hipMemcpy(hp.counts, r.counts, (size_t)r.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < r.n; s++) {
    const size_t m = std::min<size_t>(hp.counts[s], per);
    if (!m) continue;
    HIP_TRY(c, hipMemcpy(hp.out[s], r.points + (size_t)s * per * 3u, m * 3u * sizeof(float), hipMemcpyDeviceToHost));
    if (hp.index) HIP_TRY(c, hipMemcpy(hp.index[s], r.index + (size_t)s * per, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return RTUF_OK;
}

// A batch of any kind on the caller's host planes: the slot's staging grows to the batch, the sensor planes go up on the upload
// stream (`uploaded`: the lanes' first kernels wait for it, enqueue_batch), the request -- it arrives with kind and scalars -- is
// pointed at the staging and submitted, and the results come back on the download stream (`downloaded`), the clouds synchronously.
static int submit_host_planes(rtuf_context* c, BatchRequest rq, const HostPlanes& hp)
{
  using B = rtuf_context::Batch;
  const int n = rq.n;
  for (int s = 0; s < n; s++)
    if ((hp.depth && !hp.depth[s]) || (hp.out && !hp.out[s]) || (hp.labels && !hp.labels[s]) || (hp.index && !hp.index[s]))
      return c->fail(RTUF_ERR_INVALID, "null plane for stream %d", s);
  { const int rc = need_pad_intrinsics(c, n); if (rc != RTUF_OK) return rc; }      // (before the planes are staged)
  B* slot = nullptr;
  { const int rc = take_slot(c, slot); if (rc != RTUF_OK) return rc; }
  B& b = *slot;
  { const int rc = ensure_copy_streams(c); if (rc != RTUF_OK) return rc; }
  const size_t plane = (size_t)c->width * c->height;
  const size_t per = rq.capacity ? (size_t)rq.capacity : plane;      // cloud entries per stream
  // what the kind stages, in units of `bytes`; 0 units: not staged.  (A mask-bits batch stages masked / mask planes it never
  // writes, as it always has: rtuf_stats.device_bytes counts them, and the masked pointer is in its argument blocks.)
  const bool planes_out = rq.kind == Kind::Filter || rq.kind == Kind::Bits, cloud = rq.kind == Kind::Cloud;
  const struct { int st; size_t need, bytes; } staged[] = {
    {B::kStDepth, hp.depth ? (size_t)n : 0, plane * sizeof(float)},
    {B::kStMasked, planes_out ? (size_t)n : 0, plane * sizeof(float)}, {B::kStMask, planes_out ? (size_t)n : 0, plane},
    {B::kStBits, rq.kind == Kind::Bits ? (size_t)n : 0, rtuf_mask_bits_words(c->width, c->height) * sizeof(uint32_t)},
    {B::kStVirtual, rq.kind == Kind::Render ? (size_t)n : 0, plane * sizeof(float)},
    {B::kStLabels, hp.labels ? (size_t)n : 0, plane * sizeof(uint16_t)},
    {B::kStTable, rq.kind == Kind::Residual ? (size_t)n * (size_t)rq.n_labels : 0, sizeof(rtuf_link_residuals)},
    {B::kStClearance, rq.kind == Kind::Clearance ? (size_t)n * (size_t)rq.n_labels : 0, sizeof(rtuf_link_clearance)},
    {B::kStPoints, cloud ? (size_t)n * per * 3u : 0, sizeof(float)}, {B::kStIndex, hp.index ? (size_t)n * per : 0, sizeof(uint32_t)}};
  for (const auto& s : staged) { const int rc = ensure_staging(c, b.st[s.st].p, b.st[s.st].have, s.need, s.bytes); if (rc != RTUF_OK) return rc; }
  if (cloud && rq.capacity && !b.st_counts) HIP_TRY(c, dev_alloc(c, &b.st_counts, (size_t)c->max_streams * sizeof(uint32_t)));
  if (hp.depth && !b.uploaded) HIP_TRY(c, hipEventCreateWithFlags(&b.uploaded, hipEventDisableTiming));
  if (!b.downloaded) HIP_TRY(c, hipEventCreateWithFlags(&b.downloaded, hipEventDisableTiming));
  if (hp.depth) {
    const int rc = copy_planes(c, b.st[B::kStDepth].p, const_cast<void* const*>(hp.depth), n, plane * (rq.u16 ? sizeof(uint16_t) : sizeof(float)), hipMemcpyHostToDevice, &c->h2d);
    if (rc != RTUF_OK) return rc;
    HIP_TRY(c, hipEventRecord(b.uploaded, c->h2d));
    rq.depth = reinterpret_cast<const float*>(b.st[B::kStDepth].p); rq.wait_upload = true;
  }
  // the caller's arrays may be gone when a re-run downloads again: the slot keeps the pointers
  bool any_mask = false;
  b.h_out.clear(); b.h_labels.clear();
  if (hp.out) b.h_out.assign(hp.out, hp.out + n);
  if (hp.labels) b.h_labels.assign(hp.labels, hp.labels + n);
  b.h_mask.assign((size_t)n, nullptr);
  if (hp.mask) for (int s = 0; s < n; s++) { b.h_mask[s] = hp.mask[s]; any_mask |= hp.mask[s] != nullptr; }
  b.h_table = hp.table;
  auto at = [&](int st) { return b.st[st].p; };
  if (hp.labels) rq.labels = reinterpret_cast<uint16_t*>(at(B::kStLabels));
  switch (rq.kind) {
    case Kind::Filter: rq.masked = reinterpret_cast<float*>(at(B::kStMasked)); rq.mask = any_mask ? reinterpret_cast<uint8_t*>(at(B::kStMask)) : nullptr; break;
    case Kind::Bits: rq.bits = reinterpret_cast<uint32_t*>(at(B::kStBits)); rq.masked = reinterpret_cast<float*>(at(B::kStMasked)); break;      // (masked: unused, but part of the argument blocks since the first mask-bits call)
    case Kind::Render: rq.virt = reinterpret_cast<float*>(at(B::kStVirtual)); break;
    case Kind::Residual: rq.resid = reinterpret_cast<rtuf_link_residuals*>(at(B::kStTable)); break;
    case Kind::Cloud:
      rq.points = reinterpret_cast<float*>(at(B::kStPoints));
      rq.index = hp.index ? reinterpret_cast<uint32_t*>(at(B::kStIndex)) : nullptr; rq.counts = rq.capacity ? b.st_counts : nullptr;
      break;
    case Kind::Clearance: rq.clr = reinterpret_cast<rtuf_link_clearance*>(at(B::kStClearance)); break;
    case Kind::Points: break;      // (never here: the host form stages for itself, rtuf_points_batch)
  }
  { const int rc = submit_batch(c, b, rq); if (rc != RTUF_OK) return rc; }
  if (cloud) return download_cloud(c, rq, hp);
  if (rq.kind == Kind::Clearance) {          // synchronous, as the clouds: the table comes down once the batch is retired, re-runs included
    const int rc = rtuf_sync(c);
    if (rc != RTUF_OK) return rc;
    HIP_TRY(c, hipMemcpy(hp.clr_table, rq.clr, (size_t)n * (size_t)rq.n_labels * sizeof(rtuf_link_clearance), hipMemcpyDeviceToHost));
    return RTUF_OK;
  }
  b.host_io = true;
  return enqueue_download(c, b);
}

// the filter and mask-bits calls on host planes (out: masked planes or bits; labels_out: nullptr unless want_labels)
static int filter_host_planes(rtuf_context* c, Kind kind, int n, const void* const* depth_in, void* const* out, void* const* mask_out,
                              uint16_t* const* labels_out, bool want_labels, bool u16)
{
  int rc = kind == Kind::Bits ? check_batch_call(c, n, depth_in && out, u16)      // (a 16UC1 call names the 16UC1 width rule, as it always has)
                              : check_filter_call(c, n, depth_in && out && (!want_labels || labels_out), labels_out, u16);
  if (rc == RTUF_OK && kind == Kind::Bits) rc = check_bits_call(c, n, depth_in, out, u16);
  if (rc != RTUF_OK) return rc;
  HostPlanes hp{};
  hp.depth = depth_in; hp.out = out; hp.mask = mask_out; hp.labels = reinterpret_cast<void* const*>(labels_out);
  return submit_host_planes(c, BatchRequest(kind, n, u16), hp);
}

int rtuf_filter_batch_async(rtuf_context* c, int n, const float* const* depth_in, float* const* masked_out,
                            uint8_t* const* mask_out)
{
  KIDS_NEXT(c, rtuf_filter_batch_async(k, n, depth_in, masked_out, mask_out));
  if (!c) return RTUF_ERR_INVALID;
  return filter_host_planes(c, Kind::Filter, n, reinterpret_cast<const void* const*>(depth_in), reinterpret_cast<void* const*>(masked_out),
                            reinterpret_cast<void* const*>(mask_out), nullptr, false, false);
}

int rtuf_filter_batch_u16_async(rtuf_context* c, int n, const uint16_t* const* depth_in, uint16_t* const* masked_out,
                                uint8_t* const* mask_out)
{
  KIDS_NEXT(c, rtuf_filter_batch_u16_async(k, n, depth_in, masked_out, mask_out));
  if (!c) return RTUF_ERR_INVALID;
  return filter_host_planes(c, Kind::Filter, n, reinterpret_cast<const void* const*>(depth_in), reinterpret_cast<void* const*>(masked_out),
                            reinterpret_cast<void* const*>(mask_out), nullptr, false, true);
}

int rtuf_filter_batch_bits_async(rtuf_context* c, int n, const float* const* depth_in, uint32_t* const* bits_out)
{
  KIDS_NEXT(c, rtuf_filter_batch_bits_async(k, n, depth_in, bits_out));
  if (!c) return RTUF_ERR_INVALID;
  return filter_host_planes(c, Kind::Bits, n, reinterpret_cast<const void* const*>(depth_in), reinterpret_cast<void* const*>(bits_out), nullptr, nullptr, false, false);
}

int rtuf_filter_batch_bits_u16_async(rtuf_context* c, int n, const uint16_t* const* depth_in, uint32_t* const* bits_out)
{
  KIDS_NEXT(c, rtuf_filter_batch_bits_u16_async(k, n, depth_in, bits_out));
  if (!c) return RTUF_ERR_INVALID;
  return filter_host_planes(c, Kind::Bits, n, reinterpret_cast<const void* const*>(depth_in), reinterpret_cast<void* const*>(bits_out), nullptr, nullptr, false, true);
}

int rtuf_filter_batch(rtuf_context* c, int n, const float* const* depth_in, float* const* masked_out,
                      uint8_t* const* mask_out)
{
  const int rc = rtuf_filter_batch_async(c, n, depth_in, masked_out, mask_out);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

int rtuf_filter_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_in, uint16_t* const* masked_out,
                          uint8_t* const* mask_out)
{
  const int rc = rtuf_filter_batch_u16_async(c, n, depth_in, masked_out, mask_out);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

// ---- link labels -----------------------------------------------------------------------------------
// The tile kernel's depth keys carry the winning triangle's draw order; the table draw order -> label turns it into the
// label of the link the triangle belongs to.  Built on the host from every draw's link and the models' labels.
static int ensure_label_table(rtuf_context* c)
{
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (c->d_order_labels && !c->labels_dirty) return RTUF_OK;
  std::vector<uint16_t> link_label((size_t)c->n_links, 0);
  for (const HostModel& m : c->models)
    for (size_t l = 0; l < m.links.size(); l++) {
      if (!m.labels.empty()) { link_label[(size_t)m.link_base + l] = m.labels[l]; continue; }
      const int def = 1 + m.link_base + (int)l;
      if (def > 65535) return c->fail(RTUF_ERR_CAPACITY, "link %d: default labels are limited to 65535 links (set them with rtuf_set_link_labels)", def - 1);
      link_label[(size_t)m.link_base + l] = (uint16_t)def;
    }
  c->max_label = 0;
  for (const uint16_t lab : link_label) c->max_label = std::max(c->max_label, (uint32_t)lab);
  std::vector<uint16_t> table((size_t)c->n_tris + 1, 0);
  for (size_t d = 0, first = 1; d < c->draw_link.size(); d++) {
    const uint16_t lab = link_label[c->draw_link[d]];
    for (size_t o = first; o <= c->draw_last_order[d]; o++) table[o] = lab;
    first = (size_t)c->draw_last_order[d] + 1;
  }
  hipSetDevice(c->device);
  if (!c->d_order_labels) HIP_TRY(c, dev_alloc(c, &c->d_order_labels, table.size() * sizeof(uint16_t)));
  // (no batch in flight reads the table: rtuf_set_link_labels waits for them, and a new table has never been read)
  HIP_TRY(c, hipMemcpy(c->d_order_labels, table.data(), table.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  c->labels_dirty = false;
  return RTUF_OK;
}

int rtuf_set_link_labels(rtuf_context* c, int model, const uint16_t* labels, int n_links)
{
  KIDS_ALL(c, rtuf_set_link_labels(k, model, labels, n_links));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  HostModel& m = c->models[model];
  if (!labels || n_links != (int)m.links.size()) return c->fail(RTUF_ERR_INVALID, "model %d has %d links (got %d labels)", model, (int)m.links.size(), n_links);
  WAIT_IF_PENDING(c);
  m.labels.assign(labels, labels + n_links);
  c->labels_dirty = true;
  c->clr_dirty = true;                       // (a sphere takes its link's label when the next clearance batch is enqueued)
  return ensure_label_table(c);
}

int rtuf_filter_batch_device_labels(rtuf_context* c, int n, const float* d_depth, float* d_masked, uint8_t* d_mask, uint16_t* d_labels)
{
  KIDS_NEXT(c, rtuf_filter_batch_device_labels(k, n, d_depth, d_masked, d_mask, d_labels));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_filter_call(c, n, d_depth && d_masked && d_labels, d_labels, false);
  return rc != RTUF_OK ? rc : submit_device(c, filter_request(n, d_depth, d_masked, d_mask, d_labels, false));
}

int rtuf_filter_batch_device_u16_labels(rtuf_context* c, int n, const uint16_t* d_depth, uint16_t* d_masked, uint8_t* d_mask, uint16_t* d_labels)
{
  KIDS_NEXT(c, rtuf_filter_batch_device_u16_labels(k, n, d_depth, d_masked, d_mask, d_labels));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_filter_call(c, n, d_depth && d_masked && d_labels, d_labels, true);
  return rc != RTUF_OK ? rc : submit_device(c, filter_request(n, d_depth, d_masked, d_mask, d_labels, true));
}

static int filter_batch_labels_async(rtuf_context* c, int n, const void* const* depth_in, void* const* masked_out, uint8_t* const* mask_out,
                                     uint16_t* const* labels_out, bool u16)
{
  KIDS_NEXT(c, filter_batch_labels_async(k, n, depth_in, masked_out, mask_out, labels_out, u16));
  if (!c) return RTUF_ERR_INVALID;
  return filter_host_planes(c, Kind::Filter, n, depth_in, masked_out, reinterpret_cast<void* const*>(mask_out), labels_out, true, u16);
}

int rtuf_filter_batch_labels(rtuf_context* c, int n, const float* const* depth_in, float* const* masked_out, uint8_t* const* mask_out,
                             uint16_t* const* labels_out)
{
  const int rc = filter_batch_labels_async(c, n, reinterpret_cast<const void* const*>(depth_in), reinterpret_cast<void* const*>(masked_out),
                                           mask_out, labels_out, false);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

int rtuf_filter_batch_u16_labels(rtuf_context* c, int n, const uint16_t* const* depth_in, uint16_t* const* masked_out, uint8_t* const* mask_out,
                                 uint16_t* const* labels_out)
{
  const int rc = filter_batch_labels_async(c, n, reinterpret_cast<const void* const*>(depth_in), reinterpret_cast<void* const*>(masked_out),
                                           mask_out, labels_out, true);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

// ---- per-link depth thresholds -----------------------------------------------------------------------
// The same draw order the labels use, turned into the threshold of the winner's link: the table draw order -> threshold,
// built on the host from every draw's link and the models' thresholds (the global one where a model has none).
static int build_thresh_table(rtuf_context* c)
{
  std::vector<float> link_thr((size_t)c->n_links, c->params.depth_distance_threshold);
  int with = 0;
  for (const HostModel& m : c->models) {
    if (m.thresholds.empty()) continue;
    with++;
    for (size_t l = 0; l < m.links.size(); l++) link_thr[(size_t)m.link_base + l] = m.thresholds[l];
  }
  std::vector<float> table((size_t)c->n_tris + 1, c->params.depth_distance_threshold);
  for (size_t d = 0, first = 1; d < c->draw_link.size(); d++) {
    const float t = link_thr[c->draw_link[d]];
    for (size_t o = first; o <= c->draw_last_order[d]; o++) table[o] = t;
    first = (size_t)c->draw_last_order[d] + 1;
  }
  hipSetDevice(c->device);
  if (!c->d_order_thr) HIP_TRY(c, dev_alloc(c, &c->d_order_thr, table.size() * sizeof(float)));
  // (no batch in flight reads the table: every caller waited for them, and a new table has never been read)
  HIP_TRY(c, hipMemcpy(c->d_order_thr, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
  c->thresh_models = with;
  return RTUF_OK;
}

int rtuf_set_link_thresholds(rtuf_context* c, int model, const float* depth_distance_threshold, int n_links)
{
  KIDS_ALL(c, rtuf_set_link_thresholds(k, model, depth_distance_threshold, n_links));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  HostModel& m = c->models[model];
  if (!depth_distance_threshold || n_links != (int)m.links.size())
    return c->fail(RTUF_ERR_INVALID, "model %d has %d links (got %d thresholds)", model, (int)m.links.size(), n_links);
  WAIT_IF_PENDING(c);
  std::vector<float> keep = m.thresholds;
  m.thresholds.assign(depth_distance_threshold, depth_distance_threshold + n_links);      // (a model without links stays without)
  const int rc = build_thresh_table(c);
  if (rc != RTUF_OK) m.thresholds = keep;
  return rc;
}

int rtuf_clear_link_thresholds(rtuf_context* c, int model)
{
  KIDS_ALL(c, rtuf_clear_link_thresholds(k, model));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  WAIT_IF_PENDING(c);
  HostModel& m = c->models[model];
  if (m.thresholds.empty()) return RTUF_OK;
  std::vector<float> keep;
  keep.swap(m.thresholds);
  if (c->thresh_models == 1) { c->thresh_models = 0; return RTUF_OK; }      // the last one: the plain kernels from here on
  const int rc = build_thresh_table(c);
  if (rc != RTUF_OK) m.thresholds.swap(keep);
  return rc;
}

// ---- link padding --------------------------------------------------------------------------------------
// The draw order once more, turned into the winner's link slot (1 + its context-global number; 0: the background quad), and
// the slots' paddings: the tile kernel writes the slot of every pixel's winner beside the z-surface, pad_compare_kernel reads
// both (rtuf_device.h, PadArgs).  Padding is in effect while some model holds a non-zero value.
static int build_pad_tables(rtuf_context* c)
{
  std::vector<float> slot_pad((size_t)c->n_links + 1, 0.0f);
  int with = 0;
  for (const HostModel& m : c->models) {
    bool any = false;
    for (size_t l = 0; l < m.padding.size(); l++) { slot_pad[1 + (size_t)m.link_base + l] = m.padding[l]; any = any || m.padding[l] > 0.0f; }
    with += any ? 1 : 0;
  }
  hipSetDevice(c->device);
  if (!c->d_order_slot) {
    std::vector<uint16_t> table((size_t)c->n_tris + 1, 0);
    for (size_t d = 0, first = 1; d < c->draw_link.size(); d++) {
      for (size_t o = first; o <= c->draw_last_order[d]; o++) table[o] = (uint16_t)(1u + c->draw_link[d]);
      first = (size_t)c->draw_last_order[d] + 1;
    }
    HIP_TRY(c, dev_alloc(c, &c->d_order_slot, table.size() * sizeof(uint16_t)));
    HIP_TRY(c, hipMemcpy(c->d_order_slot, table.data(), table.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  if (!c->d_slot_pad) HIP_TRY(c, dev_alloc(c, &c->d_slot_pad, slot_pad.size() * sizeof(float)));
  if (!c->d_pad_focal) {
    c->focal.resize((size_t)c->max_streams, 0.0f);
    HIP_TRY(c, dev_alloc(c, &c->d_pad_focal, (size_t)c->max_streams * sizeof(float)));
    HIP_TRY(c, hipMemcpy(c->d_pad_focal, c->focal.data(), (size_t)c->max_streams * sizeof(float), hipMemcpyHostToDevice));
  }
  // (no batch in flight reads the table: every caller waited for them, and a new table has never been read)
  HIP_TRY(c, hipMemcpy(c->d_slot_pad, slot_pad.data(), slot_pad.size() * sizeof(float), hipMemcpyHostToDevice));
  c->pad_models = with;
  return RTUF_OK;
}

int rtuf_set_link_padding(rtuf_context* c, int model, const float* padding_m, int n_links)
{
  KIDS_ALL(c, rtuf_set_link_padding(k, model, padding_m, n_links));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  HostModel& m = c->models[model];
  if (!padding_m || n_links != (int)m.links.size())
    return c->fail(RTUF_ERR_INVALID, "model %d has %d links (got %d paddings)", model, (int)m.links.size(), n_links);
  for (int l = 0; l < n_links; l++)
    if (!(std::isfinite(padding_m[l]) && padding_m[l] >= 0.0f)) return c->fail(RTUF_ERR_INVALID, "link %d: the padding must be finite and >= 0 (got %g)", l, (double)padding_m[l]);
  if (c->n_links > 65534) return c->fail(RTUF_ERR_INVALID, "link padding is limited to 65534 links in the context (it has %d)", c->n_links);
  WAIT_IF_PENDING(c);
  std::vector<float> keep = m.padding;
  m.padding.assign(padding_m, padding_m + n_links);      // (a model without links stays without)
  const int rc = build_pad_tables(c);
  if (rc != RTUF_OK) m.padding = keep;
  return rc;
}

int rtuf_clear_link_padding(rtuf_context* c, int model)
{
  KIDS_ALL(c, rtuf_clear_link_padding(k, model));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  WAIT_IF_PENDING(c);
  HostModel& m = c->models[model];
  if (m.padding.empty()) return RTUF_OK;
  std::vector<float> keep;
  keep.swap(m.padding);
  const int rc = build_pad_tables(c);
  if (rc != RTUF_OK) m.padding.swap(keep);
  return rc;
}

// ---- scene planes ---------------------------------------------------------------------------------------
// include/rtuf.h, SCENE PLANES.  The planes, the streams' table and the scratch live in the context and keep their addresses
// from the first call that needs them until the last touched stream is cleared; the batches find the scene through their
// route (RouteFacts::scene: some stream has filtering enabled) and their SceneArgs.
static int check_scene_range(rtuf_context* c, int first, int n)
{
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (first < 0 || n <= 0 || first > c->max_streams || n > c->max_streams - first)
    return c->fail(RTUF_ERR_INVALID, "bad stream range [%d, %d) (max_streams = %d)", first, first + n, c->max_streams);
  return RTUF_OK;
}

static int ensure_scene(rtuf_context* c)
{
  if (c->d_scene) return RTUF_OK;
  hipSetDevice(c->device);
  const size_t plane = (size_t)c->width * c->height;
  c->scene_streams.assign((size_t)c->max_streams, SceneStream{0.0f, 0.0f, 0u, 0u});
  c->scene_touched.assign((size_t)c->max_streams, 0);
  c->scene_enabled = 0;
  HIP_TRY(c, dev_alloc(c, &c->d_scene_streams, (size_t)c->max_streams * sizeof(SceneStream)));
  HIP_TRY(c, dev_alloc(c, &c->d_scene, (size_t)c->max_streams * plane * sizeof(float)));
  HIP_TRY(c, hipMemcpy(c->d_scene_streams, c->scene_streams.data(), (size_t)c->max_streams * sizeof(SceneStream), hipMemcpyHostToDevice));
  launch_fill_f32(c->d_scene, (size_t)c->max_streams * plane, INFINITY, c->lane[0].stream);
  return wait_lane0(c);
}

// (no batch in flight reads the table: every caller waited for them)
static int upload_scene_streams(rtuf_context* c)
{
  int on = 0;
  for (const SceneStream& s : c->scene_streams) on += s.enabled ? 1 : 0;
  HIP_TRY(c, hipMemcpy(c->d_scene_streams, c->scene_streams.data(), c->scene_streams.size() * sizeof(SceneStream), hipMemcpyHostToDevice));
  c->scene_enabled = on;
  return RTUF_OK;
}

int rtuf_set_scene_planes(rtuf_context* c, int first, int n, const float* const* planes)
{
  KIDS_ALL(c, rtuf_set_scene_planes(k, first, n, planes));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_scene_range(c, first, n); if (rc != RTUF_OK) return rc; }
  if (!planes) return c->fail(RTUF_ERR_INVALID, "null plane array");
  for (int s = 0; s < n; s++) if (!planes[s]) return c->fail(RTUF_ERR_INVALID, "null plane for stream %d", first + s);
  WAIT_IF_PENDING(c);
  { const int rc = ensure_scene(c); if (rc != RTUF_OK) return rc; }
  const size_t plane = (size_t)c->width * c->height;
  const int rc = copy_planes(c, c->d_scene + (size_t)first * plane, reinterpret_cast<void* const*>(const_cast<float* const*>(planes)), n, plane * sizeof(float),
                             hipMemcpyHostToDevice, nullptr);
  if (rc == RTUF_OK) for (int s = 0; s < n; s++) c->scene_touched[(size_t)(first + s)] = 1;
  return rc;
}

int rtuf_set_scene_planes_device(rtuf_context* c, int first, int n, const float* d_planes)
{
  KIDS_ALL(c, rtuf_set_scene_planes_device(k, first, n, d_planes));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_scene_range(c, first, n); if (rc != RTUF_OK) return rc; }
  if (!d_planes) return c->fail(RTUF_ERR_INVALID, "null plane array");
  WAIT_IF_PENDING(c);
  { const int rc = ensure_scene(c); if (rc != RTUF_OK) return rc; }
  const size_t plane = (size_t)c->width * c->height;
  HIP_TRY(c, hipMemcpy(c->d_scene + (size_t)first * plane, d_planes, (size_t)n * plane * sizeof(float), hipMemcpyDeviceToDevice));
  for (int s = 0; s < n; s++) c->scene_touched[(size_t)(first + s)] = 1;
  return RTUF_OK;
}

int rtuf_get_scene_planes(rtuf_context* c, int first, int n, float* const* out)
{
  KIDS_ONE(c, 0, rtuf_get_scene_planes(k, first, n, out));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_scene_range(c, first, n); if (rc != RTUF_OK) return rc; }
  if (!out) return c->fail(RTUF_ERR_INVALID, "null plane array");
  for (int s = 0; s < n; s++) if (!out[s]) return c->fail(RTUF_ERR_INVALID, "null plane for stream %d", first + s);
  WAIT_IF_PENDING(c);
  const size_t plane = (size_t)c->width * c->height;
  if (!c->d_scene) {                     // never set, never learned: unknown everywhere
    for (int s = 0; s < n; s++) std::fill(out[s], out[s] + plane, INFINITY);
    return RTUF_OK;
  }
  hipSetDevice(c->device);
  return copy_planes(c, c->d_scene + (size_t)first * plane, reinterpret_cast<void* const*>(out), n, plane * sizeof(float), hipMemcpyDeviceToHost, nullptr);
}

int rtuf_get_scene_planes_device(rtuf_context* c, int first, int n, float* d_out)
{
  KIDS_ONE(c, 0, rtuf_get_scene_planes_device(k, first, n, d_out));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_scene_range(c, first, n); if (rc != RTUF_OK) return rc; }
  if (!d_out) return c->fail(RTUF_ERR_INVALID, "null plane array");
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  const size_t plane = (size_t)c->width * c->height;
  if (!c->d_scene) {
    launch_fill_f32(d_out, (size_t)n * plane, INFINITY, c->lane[0].stream);
    return wait_lane0(c);
  }
  HIP_TRY(c, hipMemcpy(d_out, c->d_scene + (size_t)first * plane, (size_t)n * plane * sizeof(float), hipMemcpyDeviceToDevice));
  return RTUF_OK;
}

int rtuf_set_scene_margins(rtuf_context* c, int first, int n, const float* abs_rel)
{
  KIDS_ALL(c, rtuf_set_scene_margins(k, first, n, abs_rel));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_scene_range(c, first, n); if (rc != RTUF_OK) return rc; }
  for (int s = 0; abs_rel && s < n; s++) {
    const float a = abs_rel[2 * s], r = abs_rel[2 * s + 1];
    if (!(std::isfinite(a) && a >= 0.0f)) return c->fail(RTUF_ERR_INVALID, "stream %d: the scene margin must be finite and >= 0 (got %g)", first + s, (double)a);
    if (!(r >= 0.0f && r < 1.0f)) return c->fail(RTUF_ERR_INVALID, "stream %d: the relative scene margin must lie in [0, 1) (got %g)", first + s, (double)r);
  }
  WAIT_IF_PENDING(c);
  if (!abs_rel && !c->d_scene) return RTUF_OK;      // nothing was ever enabled
  { const int rc = ensure_scene(c); if (rc != RTUF_OK) return rc; }
  const std::vector<SceneStream> keep = c->scene_streams;
  for (int s = 0; s < n; s++) {
    SceneStream& ss = c->scene_streams[(size_t)(first + s)];
    if (abs_rel) { ss.abs_m = abs_rel[2 * s]; ss.rel = abs_rel[2 * s + 1]; ss.enabled = 1u; c->scene_touched[(size_t)(first + s)] = 1; }
    else ss.enabled = 0u;
  }
  const int rc = upload_scene_streams(c);
  if (rc != RTUF_OK) c->scene_streams = keep;
  return rc;
}

int rtuf_clear_scene(rtuf_context* c, int first, int n)
{
  KIDS_ALL(c, rtuf_clear_scene(k, first, n));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_scene_range(c, first, n); if (rc != RTUF_OK) return rc; }
  WAIT_IF_PENDING(c);
  if (!c->d_scene) return RTUF_OK;
  hipSetDevice(c->device);
  const size_t plane = (size_t)c->width * c->height;
  for (int s = 0; s < n; s++) { c->scene_streams[(size_t)(first + s)] = SceneStream{0.0f, 0.0f, 0u, 0u}; c->scene_touched[(size_t)(first + s)] = 0; }
  bool any = false;
  for (uint8_t t : c->scene_touched) any = any || t != 0;
  if (!any) {
    // the last touched stream: as if the context had never held a scene
    dev_free(c, c->d_scene); dev_free(c, c->d_scene_streams); dev_free(c, c->d_scene_bits); dev_free(c, c->d_scene_stage);
    c->scene_streams.clear(); c->scene_touched.clear(); c->scene_enabled = 0;
    return RTUF_OK;
  }
  launch_fill_f32(c->d_scene + (size_t)first * plane, (size_t)n * plane, INFINITY, c->lane[0].stream);
  { const int rc = wait_lane0(c); if (rc != RTUF_OK) return rc; }
  return upload_scene_streams(c);
}

// ---- what the calls of their own share (learning a scene, the voxel inserts and carves) ------------------------
// Behind the call's own checks -- a refused call retires, allocates and copies nothing -- the host-plane forms retire what is in
// flight and bring the caller's sensor planes up into a stage of the context's, allocated on first use: [max_streams][H][W]
// floats and, summary, [max_streams][4] words behind them.
static int stage_host_planes(rtuf_context* c, float*& stage, bool summary, int n, const void* const* depth_in, bool u16)
{
  for (int s = 0; s < n; s++) if (!depth_in[s]) return c->fail(RTUF_ERR_INVALID, "null plane for stream %d", s);
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }
  hipSetDevice(c->device);
  const size_t plane = (size_t)c->width * c->height;
  if (!stage) HIP_TRY(c, dev_alloc(c, &stage, (size_t)c->max_streams * (plane + (summary ? 4u : 0u)) * sizeof(float)));
  return copy_planes(c, stage, const_cast<void* const*>(depth_in), n, plane * (u16 ? sizeof(uint16_t) : sizeof(float)), hipMemcpyHostToDevice, nullptr);
}
// the summary behind the planes of such a stage (nullptr: the caller wants none), and its way down
static uint32_t* summary_behind(const rtuf_context* c, float* stage, const uint32_t* wanted) { return wanted ? reinterpret_cast<uint32_t*>(stage + (size_t)c->max_streams * c->width * c->height) : nullptr; }
static int download_summary(rtuf_context* c, float* stage, int n, uint32_t* out)
{
  if (out) HIP_TRY(c, hipMemcpy(out, summary_behind(c, stage, out), (size_t)n * 4u * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTUF_OK;
}

// The robot's mask bits of the call's planes: a mask-bits batch like any other but for its output, `bits` -- a buffer of the
// context's, allocated on first use -- and, robot_only, its route (never the scene); rtuf_sync retires it, re-runs after an
// overflow included, before anything reads the bits.  The caller has retired what was in flight.
static int own_bits_pass(rtuf_context* c, uint32_t*& bits, int n, const void* d_depth, bool u16, bool robot_only)
{
  { const int rc = ensure_bits_planes(c, bits); if (rc != RTUF_OK) return rc; }
  BatchRequest rq = bits_request(n, d_depth, bits, u16);
  rq.robot_only = robot_only;
  { const int rc = submit_device(c, rq); if (rc != RTUF_OK) return rc; }
  return rtuf_sync(c);
}

// Learning: the robot's bits (own_bits_pass) are final before the planes are touched.
static int learn_scene_device(rtuf_context* c, int n, const void* d_depth, bool u16)
{
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }
  { const int rc = ensure_scene(c); if (rc != RTUF_OK) return rc; }
  { const int rc = own_bits_pass(c, c->d_scene_bits, n, d_depth, u16, true); if (rc != RTUF_OK) return rc; }
  SceneLearnArgs la;
  la.depth = static_cast<const float*>(d_depth); la.bits = c->d_scene_bits; la.scene = c->d_scene; la.n_streams = n; la.width = c->width; la.height = c->height; la.io_u16 = u16 ? 1 : 0;
  launch_scene_learn(la, c->lane[0].stream);
  { const int rc = finish_on_lane0(c); if (rc != RTUF_OK) return rc; }
  for (int s = 0; s < n; s++) c->scene_touched[(size_t)s] = 1;
  return RTUF_OK;
}

// the other pipelines take the planes the first one learned (state is replicated)
static int learn_scene_kids(rtuf_context* c, int n, int rc)
{
  if (rc < 0) { c->error = c->kids[0]->error; return rc; }
  for (size_t i = 1; i < c->kids.size(); i++) {
    const int rk = rtuf_set_scene_planes_device(c->kids[i], 0, n, c->kids[0]->d_scene);
    if (rk < 0) { c->error = c->kids[i]->error; return rk; }
  }
  return rc;
}

static int learn_scene_host(rtuf_context* c, int n, const void* const* depth_in, bool u16)
{
  { const int rc = check_bits_call(c, n, depth_in, depth_in, u16); if (rc != RTUF_OK) return rc; }
  { const int rc = stage_host_planes(c, c->d_scene_stage, false, n, depth_in, u16); if (rc != RTUF_OK) return rc; }
  return learn_scene_device(c, n, c->d_scene_stage, u16);
}

int rtuf_learn_scene_batch_device(rtuf_context* c, int n, const float* d_depth)
{
  if (c && !c->kids.empty()) return learn_scene_kids(c, n, rtuf_learn_scene_batch_device(c->kids[0], n, d_depth));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_bits_call(c, n, d_depth, d_depth, false);
  return rc != RTUF_OK ? rc : learn_scene_device(c, n, d_depth, false);
}

int rtuf_learn_scene_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth)
{
  if (c && !c->kids.empty()) return learn_scene_kids(c, n, rtuf_learn_scene_batch_device_u16(c->kids[0], n, d_depth));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_bits_call(c, n, d_depth, d_depth, true);
  return rc != RTUF_OK ? rc : learn_scene_device(c, n, d_depth, true);
}

int rtuf_learn_scene_batch(rtuf_context* c, int n, const float* const* depth_in)
{
  if (c && !c->kids.empty()) return learn_scene_kids(c, n, rtuf_learn_scene_batch(c->kids[0], n, depth_in));
  if (!c) return RTUF_ERR_INVALID;
  return learn_scene_host(c, n, reinterpret_cast<const void* const*>(depth_in), false);
}

int rtuf_learn_scene_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_in)
{
  if (c && !c->kids.empty()) return learn_scene_kids(c, n, rtuf_learn_scene_batch_u16(c->kids[0], n, depth_in));
  if (!c) return RTUF_ERR_INVALID;
  return learn_scene_host(c, n, reinterpret_cast<const void* const*>(depth_in), true);
}

// ---- virtual depth ---------------------------------------------------------------------------------
// A render batch is a batch like any other (Kind::Render) whose tile kernel stores the winners' virtual depth instead of
// comparing a sensor plane with it.  Parameters of the compare do not enter, and the z-surface is never used.
// (labels: the caller's label plane or its array of planes, or nullptr)
static int check_render_call(rtuf_context* c, int n, const void* out, const void* labels, bool u16)
{
  { const int rc = check_batch_call(c, n, out != nullptr, u16); if (rc != RTUF_OK) return rc; }
  BatchRequest rq(Kind::Render, n, u16);
  rq.labels = static_cast<uint16_t*>(const_cast<void*>(labels));
  { const int rc = check_route(c, rq); if (rc != RTUF_OK) return rc; }
  return labels ? ensure_label_table(c) : RTUF_OK;
}

static BatchRequest render_request(int n, void* d_virtual, uint16_t* d_labels, float empty_value, bool u16)
{
  BatchRequest rq(Kind::Render, n, u16);
  rq.virt = static_cast<float*>(d_virtual); rq.labels = d_labels; rq.empty_value = empty_value;
  return rq;
}

int rtuf_render_batch_device(rtuf_context* c, int n, float* d_virtual, uint16_t* d_labels, float empty_value)
{
  KIDS_NEXT(c, rtuf_render_batch_device(k, n, d_virtual, d_labels, empty_value));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_render_call(c, n, d_virtual, d_labels, false);
  return rc != RTUF_OK ? rc : submit_device(c, render_request(n, d_virtual, d_labels, empty_value, false));
}

int rtuf_render_batch_device_u16(rtuf_context* c, int n, uint16_t* d_virtual, uint16_t* d_labels, float empty_value)
{
  KIDS_NEXT(c, rtuf_render_batch_device_u16(k, n, d_virtual, d_labels, empty_value));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_render_call(c, n, d_virtual, d_labels, true);
  return rc != RTUF_OK ? rc : submit_device(c, render_request(n, d_virtual, d_labels, empty_value, true));
}

// host planes: the batch renders into the slot's device staging, the planes come back on the download stream
static int render_batch_async(rtuf_context* c, int n, void* const* virtual_out, uint16_t* const* labels_out, float empty_value, bool u16)
{
  KIDS_NEXT(c, render_batch_async(k, n, virtual_out, labels_out, empty_value, u16));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_render_call(c, n, virtual_out, labels_out, u16); if (rc != RTUF_OK) return rc; }
  BatchRequest rq(Kind::Render, n, u16);
  rq.empty_value = empty_value;
  HostPlanes hp{};
  hp.out = virtual_out; hp.labels = reinterpret_cast<void* const*>(labels_out);
  return submit_host_planes(c, rq, hp);
}

int rtuf_render_batch(rtuf_context* c, int n, float* const* virtual_out, uint16_t* const* labels_out, float empty_value)
{
  const int rc = render_batch_async(c, n, reinterpret_cast<void* const*>(virtual_out), labels_out, empty_value, false);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

int rtuf_render_batch_u16(rtuf_context* c, int n, uint16_t* const* virtual_out, uint16_t* const* labels_out, float empty_value)
{
  const int rc = render_batch_async(c, n, reinterpret_cast<void* const*>(virtual_out), labels_out, empty_value, true);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

// ---- link residual tables ----------------------------------------------------------------------------
// A residual batch is a batch like any other (Kind::Residual) whose tile kernel stores no plane: it classifies every pixel
// against the sensor plane and sums the classes per label into the caller's table.  Per-link thresholds are honoured, the
// two-kernel flag and the replace value do not enter, and the z-surface is never used.
static int check_residuals_call(rtuf_context* c, int n, const void* in, const void* table, int n_labels, bool u16)
{
  { const int rc = check_batch_call(c, n, in && table, false); if (rc != RTUF_OK) return rc; }
  if (n_labels < 1) return c->fail(RTUF_ERR_INVALID, "a residual table needs at least one row per stream (n_labels=%d)", n_labels);
  { const int rc = check_u16_width(c, u16); if (rc != RTUF_OK) return rc; }
  { const int rc = check_route(c, BatchRequest(Kind::Residual, n, u16)); if (rc != RTUF_OK) return rc; }
  { const int rc = ensure_label_table(c); if (rc != RTUF_OK) return rc; }
  if (c->max_label >= (uint32_t)n_labels) return c->fail(RTUF_ERR_INVALID, "a link has label %u: the table needs n_labels > %u (got %d)", c->max_label, c->max_label, n_labels);
  return RTUF_OK;
}

static BatchRequest residual_request(int n, const void* d_depth, rtuf_link_residuals* d_table, int n_labels, bool u16)
{
  BatchRequest rq(Kind::Residual, n, u16);
  rq.depth = static_cast<const float*>(d_depth); rq.resid = d_table; rq.n_labels = n_labels;
  return rq;
}

int rtuf_link_residuals_batch_device(rtuf_context* c, int n, const float* d_depth, rtuf_link_residuals* d_table, int n_labels)
{
  KIDS_NEXT(c, rtuf_link_residuals_batch_device(k, n, d_depth, d_table, n_labels));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_residuals_call(c, n, d_depth, d_table, n_labels, false);
  return rc != RTUF_OK ? rc : submit_device(c, residual_request(n, d_depth, d_table, n_labels, false));
}

int rtuf_link_residuals_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth, rtuf_link_residuals* d_table, int n_labels)
{
  KIDS_NEXT(c, rtuf_link_residuals_batch_device_u16(k, n, d_depth, d_table, n_labels));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_residuals_call(c, n, d_depth, d_table, n_labels, true);
  return rc != RTUF_OK ? rc : submit_device(c, residual_request(n, d_depth, d_table, n_labels, true));
}

// host planes: planes up into the slot's staging, the table back from its device copy on the download stream
static int link_residuals_batch_async(rtuf_context* c, int n, const void* const* depth_in, rtuf_link_residuals* table_out, int n_labels, bool u16)
{
  KIDS_NEXT(c, link_residuals_batch_async(k, n, depth_in, table_out, n_labels, u16));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_residuals_call(c, n, depth_in, table_out, n_labels, u16); if (rc != RTUF_OK) return rc; }
  BatchRequest rq(Kind::Residual, n, u16);
  rq.n_labels = n_labels;
  HostPlanes hp{};
  hp.depth = depth_in; hp.table = table_out;
  return submit_host_planes(c, rq, hp);
}

int rtuf_link_residuals_batch(rtuf_context* c, int n, const float* const* depth_in, rtuf_link_residuals* table_out, int n_labels)
{
  const int rc = link_residuals_batch_async(c, n, reinterpret_cast<const void* const*>(depth_in), table_out, n_labels, false);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

int rtuf_link_residuals_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_mm_in, rtuf_link_residuals* table_out, int n_labels)
{
  const int rc = link_residuals_batch_async(c, n, reinterpret_cast<const void* const*>(depth_mm_in), table_out, n_labels, true);
  return rc != RTUF_OK ? rc : rtuf_sync(c);
}

// ---- filtered point clouds ---------------------------------------------------------------------------
// A cloud batch (Kind::Cloud) is a mask-bits batch on the slot's own bits buffer whose launch groups run the cloud kernels
// behind their tile / dilate kernel (issue_plan).  RTUF_FLAG_TWO_KERNEL does not enter: the fused bits route is taken.
int rtuf_set_cloud_intrinsics(rtuf_context* c, int first, int n, const double* fx_fy_cx_cy)
{
  KIDS_ALL(c, rtuf_set_cloud_intrinsics(k, first, n, fx_fy_cx_cy));
  if (!c) return RTUF_ERR_INVALID;
  if (!fx_fy_cx_cy || first < 0 || n <= 0 || n > c->max_streams || first > c->max_streams - n) return c->fail(RTUF_ERR_INVALID, "bad stream range (first=%d, n=%d)", first, n);
  std::vector<CloudIntrinsics> h((size_t)n);
  for (int s = 0; s < n; s++) {
    const double fx = fx_fy_cx_cy[4 * s], fy = fx_fy_cx_cy[4 * s + 1];
    if (!(std::isfinite(fx) && fx > 0.0) || !(std::isfinite(fy) && fy > 0.0))
      return c->fail(RTUF_ERR_INVALID, "stream %d: fx and fy must be finite and > 0 (got %g, %g)", first + s, fx, fy);
    h[(size_t)s] = {(float)(1.0 / fx), (float)(1.0 / fy), (float)fx_fy_cx_cy[4 * s + 2], (float)fx_fy_cx_cy[4 * s + 3]};
  }
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  // link padding projects a margin with the larger focal length (never under-stated); its device copy exists once padding was set
  c->focal.resize((size_t)c->max_streams, 0.0f);
  for (int s = 0; s < n; s++) c->focal[(size_t)(first + s)] = (float)std::max(fx_fy_cx_cy[4 * s], fx_fy_cx_cy[4 * s + 1]);
  if (c->d_pad_focal) HIP_TRY(c, hipMemcpy(c->d_pad_focal + first, c->focal.data() + first, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  if (!c->d_cloud_intr) {
    HIP_TRY(c, dev_alloc(c, &c->d_cloud_intr, (size_t)c->max_streams * sizeof(CloudIntrinsics)));
    c->cloud_intr_set.assign((size_t)c->max_streams, 0);
  }
  HIP_TRY(c, hipMemcpy(c->d_cloud_intr + first, h.data(), (size_t)n * sizeof(CloudIntrinsics), hipMemcpyHostToDevice));
  // point list batches project with the focal lengths themselves: fx, fy rounded to float, beside kx, ky
  std::vector<PointIntrinsics> hp((size_t)n);
  for (int s = 0; s < n; s++) hp[(size_t)s] = {(float)fx_fy_cx_cy[4 * s], (float)fx_fy_cx_cy[4 * s + 1], (float)fx_fy_cx_cy[4 * s + 2], (float)fx_fy_cx_cy[4 * s + 3]};
  if (!c->d_point_intr) {
    HIP_TRY(c, dev_alloc(c, &c->d_point_intr, (size_t)c->max_streams * sizeof(PointIntrinsics)));
    HIP_TRY(c, hipMemset(c->d_point_intr, 0, (size_t)c->max_streams * sizeof(PointIntrinsics)));
  }
  HIP_TRY(c, hipMemcpy(c->d_point_intr + first, hp.data(), (size_t)n * sizeof(PointIntrinsics), hipMemcpyHostToDevice));
  std::fill(c->cloud_intr_set.begin() + first, c->cloud_intr_set.begin() + first + n, (uint8_t)1);
  return RTUF_OK;
}

static int check_cloud_call(rtuf_context* c, int n, const void* in, const void* points, const void* counts, int capacity, bool compact)
{
  { const int rc = check_batch_call(c, n, in && points && (!compact || counts), false); if (rc != RTUF_OK) return rc; }
  if (c->width & 3) return c->fail(RTUF_ERR_INVALID, "point clouds are built on the mask bits: they need a width that is a multiple of 4");
  if (compact && (capacity < 1 || (long long)capacity > (long long)c->width * c->height))
    return c->fail(RTUF_ERR_INVALID, "capacity = %d: 1 .. width * height (%lld)", capacity, (long long)c->width * c->height);
  { const int rc = check_route(c, BatchRequest(Kind::Cloud, n, false)); if (rc != RTUF_OK) return rc; }      // (16UC1 or not: no refusal asks)
  return need_intrinsics(c, n, c->d_cloud_intr);
}

// device planes of the organized form: its kernel loads four sensor values at once (16 bytes of f32, 8 bytes of 16UC1) and stores 16-byte
// vectors of points
static int check_cloud_alignment(rtuf_context* c, const void* d_depth, const void* d_points, bool u16)
{
  if (!aligned(d_points, 16)) return c->fail(RTUF_ERR_INVALID, "d_points must be 16-byte aligned");
  if (!aligned(d_depth, u16 ? 8 : 16)) return c->fail(RTUF_ERR_INVALID, "d_depth must be %d-byte aligned", u16 ? 8 : 16);
  return RTUF_OK;
}

// (capacity 0: the organized form)
static BatchRequest cloud_request(int n, const void* d_depth, float* d_points, uint32_t* d_index, uint32_t* d_counts, int capacity, bool u16)
{
  BatchRequest rq(Kind::Cloud, n, u16);
  rq.depth = static_cast<const float*>(d_depth); rq.points = d_points; rq.index = d_index; rq.counts = d_counts; rq.capacity = capacity;
  return rq;
}

int rtuf_cloud_batch_device(rtuf_context* c, int n, const float* d_depth, float* d_points)
{
  KIDS_NEXT(c, rtuf_cloud_batch_device(k, n, d_depth, d_points));
  if (!c) return RTUF_ERR_INVALID;
  int rc = check_cloud_call(c, n, d_depth, d_points, nullptr, 0, false);
  if (rc == RTUF_OK) rc = check_cloud_alignment(c, d_depth, d_points, false);
  return rc != RTUF_OK ? rc : submit_device(c, cloud_request(n, d_depth, d_points, nullptr, nullptr, 0, false));
}

int rtuf_cloud_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth, float* d_points)
{
  KIDS_NEXT(c, rtuf_cloud_batch_device_u16(k, n, d_depth, d_points));
  if (!c) return RTUF_ERR_INVALID;
  int rc = check_cloud_call(c, n, d_depth, d_points, nullptr, 0, false);
  if (rc == RTUF_OK) rc = check_cloud_alignment(c, d_depth, d_points, true);
  return rc != RTUF_OK ? rc : submit_device(c, cloud_request(n, d_depth, d_points, nullptr, nullptr, 0, true));
}

int rtuf_cloud_compact_batch_device(rtuf_context* c, int n, const float* d_depth, float* d_points, uint32_t* d_index, uint32_t* d_counts, int capacity)
{
  KIDS_NEXT(c, rtuf_cloud_compact_batch_device(k, n, d_depth, d_points, d_index, d_counts, capacity));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_cloud_call(c, n, d_depth, d_points, d_counts, capacity, true);
  return rc != RTUF_OK ? rc : submit_device(c, cloud_request(n, d_depth, d_points, d_index, d_counts, capacity, false));
}

int rtuf_cloud_compact_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth, float* d_points, uint32_t* d_index, uint32_t* d_counts, int capacity)
{
  KIDS_NEXT(c, rtuf_cloud_compact_batch_device_u16(k, n, d_depth, d_points, d_index, d_counts, capacity));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_cloud_call(c, n, d_depth, d_points, d_counts, capacity, true);
  return rc != RTUF_OK ? rc : submit_device(c, cloud_request(n, d_depth, d_points, d_index, d_counts, capacity, true));
}

// host planes, synchronous (download_cloud)
static int cloud_host_batch(rtuf_context* c, int n, const void* const* depth_in, float* const* points_out, uint32_t* const* index_out,
                            uint32_t* counts_out, int capacity, bool compact, bool u16)
{
  KIDS_NEXT(c, cloud_host_batch(k, n, depth_in, points_out, index_out, counts_out, capacity, compact, u16));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_cloud_call(c, n, depth_in, points_out, counts_out, capacity, compact); if (rc != RTUF_OK) return rc; }
  HostPlanes hp{};
  hp.depth = depth_in; hp.out = reinterpret_cast<void* const*>(points_out);
  hp.index = compact ? reinterpret_cast<void* const*>(index_out) : nullptr; hp.counts = counts_out;
  BatchRequest rq(Kind::Cloud, n, u16);
  rq.capacity = compact ? capacity : 0;
  return submit_host_planes(c, rq, hp);
}

int rtuf_cloud_batch(rtuf_context* c, int n, const float* const* depth_in, float* const* points_out)
{
  return cloud_host_batch(c, n, reinterpret_cast<const void* const*>(depth_in), points_out, nullptr, nullptr, 0, false, false);
}

int rtuf_cloud_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_mm_in, float* const* points_out)
{
  return cloud_host_batch(c, n, reinterpret_cast<const void* const*>(depth_mm_in), points_out, nullptr, nullptr, 0, false, true);
}

int rtuf_cloud_compact_batch(rtuf_context* c, int n, const float* const* depth_in, float* const* points_out, uint32_t* const* index_out,
                             uint32_t* counts_out, int capacity)
{
  return cloud_host_batch(c, n, reinterpret_cast<const void* const*>(depth_in), points_out, index_out, counts_out, capacity, true, false);
}

int rtuf_cloud_compact_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_mm_in, float* const* points_out, uint32_t* const* index_out,
                                 uint32_t* counts_out, int capacity)
{
  return cloud_host_batch(c, n, reinterpret_cast<const void* const*>(depth_mm_in), points_out, index_out, counts_out, capacity, true, true);
}

// ---- point list batches ------------------------------------------------------------------------------
// A points batch (Kind::Points) is a render batch into the slot's own float plane (empty pixels +inf) whose launch groups run
// the points kernel behind their tile_render_kernel (issue_plan): no sensor plane is read, no image plane returned.
static int ensure_point_transforms(rtuf_context* c)
{
  if (c->d_point_tf) return RTUF_OK;
  c->point_tf.assign((size_t)c->max_streams, PointTransform{});
  HIP_TRY(c, dev_alloc(c, &c->d_point_tf, (size_t)c->max_streams * sizeof(PointTransform)));
  HIP_TRY(c, hipMemset(c->d_point_tf, 0, (size_t)c->max_streams * sizeof(PointTransform)));
  return RTUF_OK;
}

int rtuf_set_point_transforms(rtuf_context* c, int first, int n, const double* optical_from_points)
{
  KIDS_ALL(c, rtuf_set_point_transforms(k, first, n, optical_from_points));
  if (!c) return RTUF_ERR_INVALID;
  if (first < 0 || n <= 0 || n > c->max_streams || first > c->max_streams - n) return c->fail(RTUF_ERR_INVALID, "bad stream range (first=%d, n=%d)", first, n);
  if (optical_from_points)
    for (int s = 0; s < n; s++)
      for (int col = 0; col < 4; col++)
        for (int r = 0; r < 3; r++)
          if (!std::isfinite(optical_from_points[16 * s + 4 * col + r]) || !std::isfinite((float)optical_from_points[16 * s + 4 * col + r]))
            return c->fail(RTUF_ERR_INVALID, "stream %d: the point transform has a non-finite entry (row %d, column %d)", first + s, r, col);
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  if (!optical_from_points && !c->d_point_tf) return RTUF_OK;      // (none was ever set: nothing to take back)
  { const int rc = ensure_point_transforms(c); if (rc != RTUF_OK) return rc; }
  for (int s = 0; s < n; s++) {
    PointTransform t{};
    if (optical_from_points) {
      for (int i = 0; i < 16; i++) t.m[i] = (i & 3) == 3 ? 0.0f : (float)optical_from_points[16 * s + i];
      t.on = 1u;
    }
    c->point_tf[(size_t)(first + s)] = t;
  }
  HIP_TRY(c, hipMemcpy(c->d_point_tf + first, c->point_tf.data() + first, (size_t)n * sizeof(PointTransform), hipMemcpyHostToDevice));
  return RTUF_OK;
}

static int check_points_call(rtuf_context* c, int n, bool have_args, long long capacity, int radius)
{
  { const int rc = check_batch_call(c, n, have_args, false); if (rc != RTUF_OK) return rc; }
  if (capacity < 1 || capacity > (long long)kMaxPointsCapacity) return c->fail(RTUF_ERR_INVALID, "capacity = %lld: 1 .. %d", capacity, kMaxPointsCapacity);
  if (radius < 0 || radius > kMaxPointsRadius) return c->fail(RTUF_ERR_INVALID, "radius_px = %d: 0 .. %d", radius, kMaxPointsRadius);
  { const int rc = check_route(c, BatchRequest(Kind::Points, n, false)); if (rc != RTUF_OK) return rc; }
  { const int rc = need_intrinsics(c, n, c->d_point_intr); if (rc != RTUF_OK) return rc; }
  return ensure_point_transforms(c);
}

static BatchRequest points_request(int n, const float* d_points, const uint32_t* d_counts, int capacity, int radius, uint8_t* d_verdict,
                                   uint32_t* d_pixel, uint32_t* d_summary)
{
  BatchRequest rq(Kind::Points, n, false);
  rq.pt_points = d_points; rq.pt_counts = d_counts; rq.capacity = capacity; rq.pt_radius = radius;
  rq.pt_verdict = d_verdict; rq.pt_pixel = d_pixel; rq.pt_summary = d_summary;
  return rq;
}

int rtuf_points_batch_device(rtuf_context* c, int n, const float* d_points, const uint32_t* d_counts, int capacity, int radius_px,
                             uint8_t* d_verdict, uint32_t* d_pixel, uint32_t* d_summary)
{
  KIDS_NEXT(c, rtuf_points_batch_device(k, n, d_points, d_counts, capacity, radius_px, d_verdict, d_pixel, d_summary));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_points_call(c, n, d_points && d_counts && d_verdict, capacity, radius_px);
  return rc != RTUF_OK ? rc : submit_device(c, points_request(n, d_points, d_counts, capacity, radius_px, d_verdict, d_pixel, d_summary));
}

// host lists, synchronous: the lists go up into one block of the context's (points, counts, verdicts, pixels, summary; every
// part on a 16-byte boundary), the batch runs on it with capacity = the largest count, and min(count, capacity) = count
// entries per stream come down once the batch is retired, re-runs included
int rtuf_points_batch(rtuf_context* c, int n, const float* const* points_in, const uint32_t* counts, int radius_px,
                      uint8_t* const* verdict_out, uint32_t* const* pixel_out, uint32_t* summary_out)
{
  KIDS_NEXT(c, rtuf_points_batch(k, n, points_in, counts, radius_px, verdict_out, pixel_out, summary_out));
  if (!c) return RTUF_ERR_INVALID;
  long long cap = 1;
  if (counts && n > 0 && n <= c->max_streams) for (int s = 0; s < n; s++) cap = std::max<long long>(cap, (long long)counts[s]);
  { const int rc = check_points_call(c, n, points_in && counts && verdict_out, cap, radius_px); if (rc != RTUF_OK) return rc; }
  for (int s = 0; s < n; s++)
    if (counts[s] && (!points_in[s] || !verdict_out[s] || (pixel_out && !pixel_out[s]))) return c->fail(RTUF_ERR_INVALID, "null list for stream %d", s);
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }      // (the block may still be read by an earlier call's batch)
  hipSetDevice(c->device);
  const size_t capacity = (size_t)((cap + 3) & ~3ll);                // (a multiple of 4: the kernel's wide path)
  auto up16 = [](size_t b) { return (b + 15u) & ~(size_t)15u; };
  const size_t o_points = 0, o_counts = o_points + up16((size_t)n * capacity * 3u * sizeof(float)), o_verdict = o_counts + up16((size_t)n * sizeof(uint32_t));
  const size_t o_pixel = o_verdict + up16((size_t)n * capacity), o_summary = o_pixel + up16(pixel_out ? (size_t)n * capacity * sizeof(uint32_t) : 0);
  const size_t bytes = o_summary + up16((size_t)n * 4u * sizeof(uint32_t));
  { const int rc = ensure_staging(c, c->d_pt_stage, c->pt_stage_bytes, bytes, 1); if (rc != RTUF_OK) return rc; }
  char* const d = c->d_pt_stage;
  for (int s = 0; s < n; s++)
    if (counts[s]) HIP_TRY(c, hipMemcpy(d + o_points + (size_t)s * capacity * 3u * sizeof(float), points_in[s], (size_t)counts[s] * 3u * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d + o_counts, counts, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  {
    const int rc = submit_device(c, points_request(n, reinterpret_cast<const float*>(d + o_points), reinterpret_cast<const uint32_t*>(d + o_counts), (int)capacity, radius_px,
                                                   reinterpret_cast<uint8_t*>(d + o_verdict), pixel_out ? reinterpret_cast<uint32_t*>(d + o_pixel) : nullptr,
                                                   reinterpret_cast<uint32_t*>(d + o_summary)));
    if (rc != RTUF_OK) return rc;
  }
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }
  for (int s = 0; s < n; s++) {
    if (!counts[s]) continue;
    HIP_TRY(c, hipMemcpy(verdict_out[s], d + o_verdict + (size_t)s * capacity, (size_t)counts[s], hipMemcpyDeviceToHost));
    if (pixel_out) HIP_TRY(c, hipMemcpy(pixel_out[s], d + o_pixel + (size_t)s * capacity * sizeof(uint32_t), (size_t)counts[s] * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  if (summary_out) HIP_TRY(c, hipMemcpy(summary_out, d + o_summary, (size_t)n * 4u * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTUF_OK;
}

// ---- voxel occupancy grids ---------------------------------------------------------------------------
// An insert is no batch kind: like learning a scene it is a call of its own that retires what is in flight, runs an ordinary
// mask-bits batch into a buffer of the context (plane form), retires that too -- re-runs after a bin regrowth included, so the
// grid never sees provisional bits -- and then runs one kernel on lane 0 and waits for it.  With several pipelines the grid
// lives in the first one: the front retires every pipeline (a list may be the output of a batch in any of them) and hands on.
#define KIDS_FIRST_RETIRED(c, expr)                                                        \
  if ((c) && !(c)->kids.empty()) {                                                         \
    { const int rs_ = rtuf_sync(c); if (rs_ != RTUF_OK) return rs_; }                      \
    rtuf_context* k = (c)->kids[0];                                                        \
    const int rc_ = (expr);                                                                \
    if (rc_ < 0) (c)->error = k->error;                                                    \
    return rc_;                                                                            \
  }

static void free_voxel_grid(rtuf_context* c)
{
  dev_free(c, c->d_vox_bits); dev_free(c, c->d_vox_counts);
  dev_free(c, c->d_vox_free); dev_free(c, c->d_vox_inv);
  c->vox_grid = VoxelGrid{}; c->vox_voxels = 0; c->vox_words = 0;
}

static int clear_voxel_grid(rtuf_context* c)
{
  launch_voxel_clear(c->d_vox_bits, (c->vox_words + 3u) & ~(size_t)3u, c->lane[0].stream);
  if (c->d_vox_counts) launch_voxel_clear(c->d_vox_counts, (c->vox_voxels + 3u) & ~(size_t)3u, c->lane[0].stream);
  if (c->d_vox_free) launch_voxel_clear(c->d_vox_free, (c->vox_words + 3u) & ~(size_t)3u, c->lane[0].stream);
  return finish_on_lane0(c);
}

int rtuf_set_voxel_grid(rtuf_context* c, const double* origin, double voxel_size, const int* dims, int with_counts)
{
  KIDS_ONE(c, 0, rtuf_set_voxel_grid(k, origin, voxel_size, dims, with_counts));
  if (!c) return RTUF_ERR_INVALID;
  if (!dims) {
    WAIT_IF_PENDING(c);
    hipSetDevice(c->device);
    free_voxel_grid(c);
    return RTUF_OK;
  }
  if (!origin) return c->fail(RTUF_ERR_INVALID, "null origin");
  long long total = 1;
  for (int r = 0; r < 3; r++) {
    if (dims[r] < 1 || dims[r] > kMaxVoxelDim) return c->fail(RTUF_ERR_INVALID, "voxel grid: dims[%d] = %d: 1 .. %d", r, dims[r], kMaxVoxelDim);
    total *= dims[r];
    if (!std::isfinite(origin[r]) || !std::isfinite((float)origin[r])) return c->fail(RTUF_ERR_INVALID, "voxel grid: origin[%d] is not finite", r);
  }
  if (total > (long long)kMaxVoxels) return c->fail(RTUF_ERR_INVALID, "voxel grid: %lld voxels, at most %u", total, kMaxVoxels);
  const float size = (float)voxel_size, inv = 1.0f / size;
  if (!(std::isfinite(size) && size > 0.0f && std::isfinite(inv)))
    return c->fail(RTUF_ERR_INVALID, "voxel grid: voxel_size must be finite and > 0 as a float, and so must its reciprocal (got %g)", voxel_size);
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  // (the new arrays first: a failed allocation leaves the grid that is there)
  const size_t words = ((size_t)total + 31u) / 32u;
  uint32_t* bits = nullptr; uint32_t* counts = nullptr;
  HIP_TRY(c, dev_alloc(c, &bits, ((words + 3u) & ~(size_t)3u) * sizeof(uint32_t)));
  if (with_counts) {
    const hipError_t e = dev_alloc(c, &counts, (((size_t)total + 3u) & ~(size_t)3u) * sizeof(uint32_t));
    if (e != hipSuccess) { dev_free(c, bits); HIP_TRY(c, e); }
  }
  free_voxel_grid(c);
  c->d_vox_bits = bits; c->d_vox_counts = counts;
  c->vox_grid = VoxelGrid{(float)origin[0], (float)origin[1], (float)origin[2], inv, dims[0], dims[1], dims[2]};
  c->vox_voxels = (size_t)total; c->vox_words = words; c->vox_size = size;
  return clear_voxel_grid(c);
}

int rtuf_set_voxel_transforms(rtuf_context* c, int first, int n, const double* world_from_optical)
{
  KIDS_ONE(c, 0, rtuf_set_voxel_transforms(k, first, n, world_from_optical));
  if (!c) return RTUF_ERR_INVALID;
  if (first < 0 || n <= 0 || n > c->max_streams || first > c->max_streams - n) return c->fail(RTUF_ERR_INVALID, "bad stream range (first=%d, n=%d)", first, n);
  if (world_from_optical)
    for (int s = 0; s < n; s++)
      for (int col = 0; col < 4; col++)
        for (int r = 0; r < 3; r++)
          if (!std::isfinite(world_from_optical[16 * s + 4 * col + r]) || !std::isfinite((float)world_from_optical[16 * s + 4 * col + r]))
            return c->fail(RTUF_ERR_INVALID, "stream %d: the voxel transform has a non-finite entry (row %d, column %d)", first + s, r, col);
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  if (!world_from_optical && !c->d_vox_tf) return RTUF_OK;      // (none was ever set: nothing to take back)
  if (!c->d_vox_tf) {
    c->vox_tf.assign((size_t)c->max_streams, PointTransform{});
    HIP_TRY(c, dev_alloc(c, &c->d_vox_tf, (size_t)c->max_streams * sizeof(PointTransform)));
    HIP_TRY(c, hipMemset(c->d_vox_tf, 0, (size_t)c->max_streams * sizeof(PointTransform)));
  }
  for (int s = 0; s < n; s++) {
    PointTransform t{};
    if (world_from_optical) {
      for (int i = 0; i < 16; i++) t.m[i] = (i & 3) == 3 ? 0.0f : (float)world_from_optical[16 * s + i];
      t.on = 1u;
    }
    c->vox_tf[(size_t)(first + s)] = t;
  }
  HIP_TRY(c, hipMemcpy(c->d_vox_tf + first, c->vox_tf.data() + first, (size_t)n * sizeof(PointTransform), hipMemcpyHostToDevice));
  // voxel free space: the inverses of the streams that changed (a matrix that cannot be inverted is refused by the carve)
  c->vox_inv.resize((size_t)c->max_streams, PointTransform{});
  c->vox_inv_ok.resize((size_t)c->max_streams, (uint8_t)1);
  for (int s = first; s < first + n; s++) {
    PointTransform inv{};
    c->vox_inv_ok[(size_t)s] = 1;
    if (c->vox_tf[(size_t)s].on) {
      inv.on = 1u;
      c->vox_inv_ok[(size_t)s] = voxel_inverse_transform(c->vox_tf[(size_t)s].m, inv.m) ? 1 : 0;
    }
    c->vox_inv[(size_t)s] = inv;
  }
  if (c->d_vox_inv) HIP_TRY(c, hipMemcpy(c->d_vox_inv + first, c->vox_inv.data() + first, (size_t)n * sizeof(PointTransform), hipMemcpyHostToDevice));
  return RTUF_OK;
}

static int need_voxel_grid(rtuf_context* c) { return c->d_vox_bits ? RTUF_OK : c->fail(RTUF_ERR_STATE, "the context has no voxel grid (rtuf_set_voxel_grid)"); }

int rtuf_voxel_clear(rtuf_context* c)
{
  KIDS_ONE(c, 0, rtuf_voxel_clear(k));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  return clear_voxel_grid(c);
}

int rtuf_voxel_grid_device(rtuf_context* c, const uint32_t** d_bits, const uint32_t** d_counts, size_t* n_voxels)
{
  KIDS_ONE(c, 0, rtuf_voxel_grid_device(k, d_bits, d_counts, n_voxels));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  if (d_counts && !c->d_vox_counts) return c->fail(RTUF_ERR_STATE, "the voxel grid has no counts (rtuf_set_voxel_grid: with_counts)");
  if (d_bits) *d_bits = c->d_vox_bits;
  if (d_counts) *d_counts = c->d_vox_counts;
  if (n_voxels) *n_voxels = c->vox_voxels;
  return RTUF_OK;
}

int rtuf_get_voxel_grid(rtuf_context* c, uint32_t* bits_out, uint32_t* counts_out)
{
  KIDS_ONE(c, 0, rtuf_get_voxel_grid(k, bits_out, counts_out));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  if (counts_out && !c->d_vox_counts) return c->fail(RTUF_ERR_STATE, "the voxel grid has no counts (rtuf_set_voxel_grid: with_counts)");
  hipSetDevice(c->device);
  if (bits_out) HIP_TRY(c, hipMemcpy(bits_out, c->d_vox_bits, c->vox_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (counts_out) HIP_TRY(c, hipMemcpy(counts_out, c->d_vox_counts, c->vox_voxels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTUF_OK;
}

static void voxel_grid_args(const rtuf_context* c, VoxelArgs& va, int n, uint32_t* d_summary)
{
  const VoxelGrid& g = c->vox_grid;
  va.ox = g.ox; va.oy = g.oy; va.oz = g.oz; va.inv = g.inv; va.nx = g.nx; va.ny = g.ny; va.nz = g.nz;
  va.grid_bits = c->d_vox_bits; va.grid_counts = c->d_vox_counts; va.world_tf = c->d_vox_tf;
  va.summary = d_summary; va.n_streams = n;
}
static int run_voxel_insert(rtuf_context* c, const VoxelArgs& va) { launch_voxel_insert(va, c->lane[0].stream); return finish_on_lane0(c); }

// what a plane insert checks before anything is retired or written: the mask-bits calls' conditions, the grid, the intrinsics
static int check_voxel_call(rtuf_context* c, int n, const void* in, bool u16)
{
  { const int rc = check_bits_call(c, n, in, in, u16); if (rc != RTUF_OK) return rc; }
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  return need_intrinsics(c, n, c->d_cloud_intr);
}

static int voxel_insert_device(rtuf_context* c, int n, const void* d_depth, uint32_t* d_summary, bool u16)
{
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }
  { const int rc = own_bits_pass(c, c->d_vox_mask_bits, n, d_depth, u16, false); if (rc != RTUF_OK) return rc; }
  VoxelArgs va{}; voxel_grid_args(c, va, n, d_summary);
  va.depth = static_cast<const float*>(d_depth); va.bits = c->d_vox_mask_bits; va.intr = c->d_cloud_intr;
  va.width = c->width; va.height = c->height; va.io_u16 = u16 ? 1 : 0; va.wide = (c->width & 3) == 0 && aligned(d_depth, u16 ? 8 : 16) ? 1 : 0;
  return run_voxel_insert(c, va);
}

static int voxel_insert_host(rtuf_context* c, int n, const void* const* depth_in, uint32_t* summary_out, bool u16)
{
  { const int rc = check_voxel_call(c, n, depth_in, u16); if (rc != RTUF_OK) return rc; }
  { const int rc = stage_host_planes(c, c->d_vox_stage, true, n, depth_in, u16); if (rc != RTUF_OK) return rc; }
  { const int rc = voxel_insert_device(c, n, c->d_vox_stage, summary_behind(c, c->d_vox_stage, summary_out), u16); if (rc != RTUF_OK) return rc; }
  return download_summary(c, c->d_vox_stage, n, summary_out);
}

int rtuf_voxel_insert_batch_device(rtuf_context* c, int n, const float* d_depth, uint32_t* d_summary)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_insert_batch_device(k, n, d_depth, d_summary));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_voxel_call(c, n, d_depth, false);
  return rc != RTUF_OK ? rc : voxel_insert_device(c, n, d_depth, d_summary, false);
}

int rtuf_voxel_insert_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth, uint32_t* d_summary)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_insert_batch_device_u16(k, n, d_depth, d_summary));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_voxel_call(c, n, d_depth, true);
  return rc != RTUF_OK ? rc : voxel_insert_device(c, n, d_depth, d_summary, true);
}

int rtuf_voxel_insert_batch(rtuf_context* c, int n, const float* const* depth_in, uint32_t* summary_out)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_insert_batch(k, n, depth_in, summary_out));
  if (!c) return RTUF_ERR_INVALID;
  return voxel_insert_host(c, n, reinterpret_cast<const void* const*>(depth_in), summary_out, false);
}

int rtuf_voxel_insert_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_mm_in, uint32_t* summary_out)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_insert_batch_u16(k, n, depth_mm_in, summary_out));
  if (!c) return RTUF_ERR_INVALID;
  return voxel_insert_host(c, n, reinterpret_cast<const void* const*>(depth_mm_in), summary_out, true);
}

int rtuf_voxel_insert_points_device(rtuf_context* c, int n, const float* d_points, const uint32_t* d_counts, int capacity, const uint8_t* d_verdict,
                                    uint32_t* d_summary)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_insert_points_device(k, n, d_points, d_counts, capacity, d_verdict, d_summary));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_batch_call(c, n, d_points && d_counts, false); if (rc != RTUF_OK) return rc; }
  if (capacity < 1 || capacity > kMaxPointsCapacity) return c->fail(RTUF_ERR_INVALID, "capacity = %d: 1 .. %d", capacity, kMaxPointsCapacity);
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }      // (the list may be the output of a batch in flight)
  hipSetDevice(c->device);
  VoxelArgs va{}; voxel_grid_args(c, va, n, d_summary);
  va.points = d_points; va.counts = d_counts; va.verdict = d_verdict; va.point_tf = c->d_point_tf; va.capacity = capacity;
  va.wide = aligned(d_points, 16) && aligned(d_verdict, 4) && (capacity & 3) == 0 ? 1 : 0;
  return run_voxel_insert(c, va);
}

// ---- voxel free space ----------------------------------------------------------------------------------
// A carve is no batch kind either: it retires what is in flight (the planes may be a batch's output), runs one kernel on lane 0
// of the first pipeline and waits for it.  No mask-bits batch runs, so any width is accepted.
static int ensure_voxel_free(rtuf_context* c)
{
  if (c->d_vox_free) return RTUF_OK;
  const size_t words = (c->vox_words + 3u) & ~(size_t)3u;
  HIP_TRY(c, dev_alloc(c, &c->d_vox_free, words * sizeof(uint32_t)));
  launch_voxel_clear(c->d_vox_free, words, c->lane[0].stream);
  return finish_on_lane0(c);
}

// what a carve checks before anything is retired or written
static int check_carve_call(rtuf_context* c, int n, const void* in, double margin, int radius_px)
{
  { const int rc = check_batch_call(c, n, in != nullptr, false); if (rc != RTUF_OK) return rc; }
  if (radius_px < 0 || radius_px > kMaxCarveRadius) return c->fail(RTUF_ERR_INVALID, "radius_px = %d: 0 .. %d", radius_px, kMaxCarveRadius);
  if (!(std::isfinite(margin) && margin >= 0.0 && std::isfinite((float)margin)))
    return c->fail(RTUF_ERR_INVALID, "the carve margin must be finite and >= 0, as a float too (got %g)", margin);
  for (int s = 0; s < n; s++)
    if (!c->vox_inv_ok.empty() && !c->vox_inv_ok[(size_t)s])
      return c->fail(RTUF_ERR_INVALID, "stream %d: its voxel transform cannot be inverted (rtuf_set_voxel_transforms)", s);
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  return need_intrinsics(c, n, c->d_point_intr);
}

static int voxel_carve_device(rtuf_context* c, int n, const void* d_depth, double margin, int radius_px, uint32_t* d_summary, bool u16)
{
  { const int rc = rtuf_sync(c); if (rc != RTUF_OK) return rc; }
  hipSetDevice(c->device);
  { const int rc = ensure_voxel_free(c); if (rc != RTUF_OK) return rc; }
  if (c->d_vox_tf && !c->d_vox_inv) {
    HIP_TRY(c, dev_alloc(c, &c->d_vox_inv, (size_t)c->max_streams * sizeof(PointTransform)));
    HIP_TRY(c, hipMemcpy(c->d_vox_inv, c->vox_inv.data(), (size_t)c->max_streams * sizeof(PointTransform), hipMemcpyHostToDevice));
  }
  const VoxelGrid& g = c->vox_grid;
  VoxelCarveArgs va{};
  va.ox = g.ox; va.oy = g.oy; va.oz = g.oz; va.size = c->vox_size; va.nx = g.nx; va.ny = g.ny; va.nz = g.nz;
  va.n_voxels = (uint32_t)c->vox_voxels; va.free_bits = c->d_vox_free; va.inv_tf = c->d_vox_inv; va.intr = c->d_point_intr;
  va.depth = static_cast<const float*>(d_depth); va.summary = d_summary; va.margin = (float)margin; va.radius = radius_px;
  va.width = c->width; va.height = c->height; va.io_u16 = u16 ? 1 : 0; va.n_streams = n;
  launch_voxel_carve(va, c->lane[0].stream);
  return finish_on_lane0(c);
}

static int voxel_carve_host(rtuf_context* c, int n, const void* const* depth_in, double margin, int radius_px, uint32_t* summary_out, bool u16)
{
  { const int rc = check_carve_call(c, n, depth_in, margin, radius_px); if (rc != RTUF_OK) return rc; }
  { const int rc = stage_host_planes(c, c->d_vox_stage, true, n, depth_in, u16); if (rc != RTUF_OK) return rc; }
  { const int rc = voxel_carve_device(c, n, c->d_vox_stage, margin, radius_px, summary_behind(c, c->d_vox_stage, summary_out), u16); if (rc != RTUF_OK) return rc; }
  return download_summary(c, c->d_vox_stage, n, summary_out);
}

int rtuf_voxel_carve_batch_device(rtuf_context* c, int n, const float* d_depth, double margin, int radius_px, uint32_t* d_summary)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_carve_batch_device(k, n, d_depth, margin, radius_px, d_summary));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_carve_call(c, n, d_depth, margin, radius_px);
  return rc != RTUF_OK ? rc : voxel_carve_device(c, n, d_depth, margin, radius_px, d_summary, false);
}

int rtuf_voxel_carve_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth_mm, double margin, int radius_px, uint32_t* d_summary)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_carve_batch_device_u16(k, n, d_depth_mm, margin, radius_px, d_summary));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_carve_call(c, n, d_depth_mm, margin, radius_px);
  return rc != RTUF_OK ? rc : voxel_carve_device(c, n, d_depth_mm, margin, radius_px, d_summary, true);
}

int rtuf_voxel_carve_batch(rtuf_context* c, int n, const float* const* depth_in, double margin, int radius_px, uint32_t* summary_out)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_carve_batch(k, n, depth_in, margin, radius_px, summary_out));
  if (!c) return RTUF_ERR_INVALID;
  return voxel_carve_host(c, n, reinterpret_cast<const void* const*>(depth_in), margin, radius_px, summary_out, false);
}

int rtuf_voxel_carve_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_mm_in, double margin, int radius_px, uint32_t* summary_out)
{
  KIDS_FIRST_RETIRED(c, rtuf_voxel_carve_batch_u16(k, n, depth_mm_in, margin, radius_px, summary_out));
  if (!c) return RTUF_ERR_INVALID;
  return voxel_carve_host(c, n, reinterpret_cast<const void* const*>(depth_mm_in), margin, radius_px, summary_out, true);
}

int rtuf_voxel_free_device(rtuf_context* c, const uint32_t** d_free_bits, size_t* n_voxels)
{
  KIDS_ONE(c, 0, rtuf_voxel_free_device(k, d_free_bits, n_voxels));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  { const int rc = ensure_voxel_free(c); if (rc != RTUF_OK) return rc; }
  if (d_free_bits) *d_free_bits = c->d_vox_free;
  if (n_voxels) *n_voxels = c->vox_voxels;
  return RTUF_OK;
}

int rtuf_get_voxel_free(rtuf_context* c, uint32_t* free_out)
{
  KIDS_ONE(c, 0, rtuf_get_voxel_free(k, free_out));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = need_voxel_grid(c); if (rc != RTUF_OK) return rc; }
  WAIT_IF_PENDING(c);
  hipSetDevice(c->device);
  { const int rc = ensure_voxel_free(c); if (rc != RTUF_OK) return rc; }
  if (free_out) HIP_TRY(c, hipMemcpy(free_out, c->d_vox_free, c->vox_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTUF_OK;
}

// ---- link clearance tables ---------------------------------------------------------------------------
// A clearance batch (Kind::Clearance) is a mask-bits batch on the slot's own bits buffer, as a cloud batch is, whose launch
// groups run the clearance kernels behind their tile / dilate kernel (issue_plan).  The spheres live on the host per model
// (rtuf_set_link_spheres) and go to the device sorted by the label their link has when the batch is enqueued.
static int build_clearance_spheres(rtuf_context* c, std::vector<ClearanceSphere>& out, std::vector<uint32_t>& slot_label)
{
  out.clear(); slot_label.clear();
  uint32_t id = 0;
  for (size_t mi = 0; mi < c->models.size(); mi++) {
    const HostModel& m = c->models[mi];
    for (size_t i = 0; i < m.sph_link.size(); i++, id++) {
      const int l = m.sph_link[i];
      const int label = m.labels.empty() ? 1 + m.link_base + l : (int)m.labels[(size_t)l];
      if (label > 65535) return c->fail(RTUF_ERR_CAPACITY, "link %d: default labels are limited to 65535 links (set them with rtuf_set_link_labels)", label - 1);
      if (!label) continue;                  // spheres of label 0 are ignored
      const float* q = &m.sph_xyzr[4 * i];
      out.push_back({q[0], q[1], q[2], q[3], (uint32_t)(m.link_base + l), (uint32_t)mi, (uint32_t)label, id});
    }
  }
  std::stable_sort(out.begin(), out.end(), [](const ClearanceSphere& a, const ClearanceSphere& b) { return a.label_slot < b.label_slot; });
  for (ClearanceSphere& sp : out) {
    if (slot_label.empty() || slot_label.back() != sp.label_slot) slot_label.push_back(sp.label_slot);
    sp.label_slot |= (uint32_t)(slot_label.size() - 1) << 16;
  }
  if (slot_label.size() > (size_t)kMaxClearanceLabels)
    return c->fail(RTUF_ERR_INVALID, "the link spheres carry %d distinct non-zero labels (at most %d)", (int)slot_label.size(), kMaxClearanceLabels);
  return RTUF_OK;
}

int rtuf_set_link_spheres(rtuf_context* c, int model, const int32_t* link, const float* xyzr, int n_spheres)
{
  KIDS_ALL(c, rtuf_set_link_spheres(k, model, link, xyzr, n_spheres));
  if (!c) return RTUF_ERR_INVALID;
  if (!c->finalized) return c->fail(RTUF_ERR_STATE, "call rtuf_finalize_models first");
  if (model < 0 || model >= (int)c->models.size()) return c->fail(RTUF_ERR_INVALID, "bad model id %d", model);
  if (n_spheres < 0 || (n_spheres > 0 && (!link || !xyzr))) return c->fail(RTUF_ERR_INVALID, "bad sphere list (n_spheres=%d)", n_spheres);
  HostModel& m = c->models[model];
  size_t total = (size_t)n_spheres;
  for (const HostModel& o : c->models) if (&o != &m) total += o.sph_link.size();
  if (total > (size_t)kMaxClearanceSpheres) return c->fail(RTUF_ERR_INVALID, "%zu spheres in the context (at most %d)", total, kMaxClearanceSpheres);
  for (int i = 0; i < n_spheres; i++) {
    const float* q = xyzr + 4 * (size_t)i;
    if (link[i] < 0 || link[i] >= (int)m.links.size()) return c->fail(RTUF_ERR_INVALID, "sphere %d: model %d has no link %d", i, model, (int)link[i]);
    if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) return c->fail(RTUF_ERR_INVALID, "sphere %d: the centre is not finite", i);
    if (!(std::isfinite(q[3]) && q[3] >= 0.0f)) return c->fail(RTUF_ERR_INVALID, "sphere %d: the radius must be finite and >= 0 (got %g)", i, (double)q[3]);
  }
  WAIT_IF_PENDING(c);
  std::vector<int32_t> old_link(link, link + n_spheres);
  std::vector<float> old_xyzr(xyzr, xyzr + 4 * (size_t)n_spheres);
  old_link.swap(m.sph_link); old_xyzr.swap(m.sph_xyzr);
  std::vector<ClearanceSphere> sorted; std::vector<uint32_t> slots;
  const int rc = build_clearance_spheres(c, sorted, slots);
  if (rc != RTUF_OK) { old_link.swap(m.sph_link); old_xyzr.swap(m.sph_xyzr); return rc; }      // (a refused list changes nothing)
  c->clr_dirty = true;
  return RTUF_OK;
}

// the device copy of the sorted spheres, as the labels stand now (no batch in flight reads it while it is dirty: the setters
// that make it so wait for the batches in flight, and a clearance batch is enqueued only behind this)
static int ensure_clearance_spheres(rtuf_context* c)
{
  if (!c->clr_dirty && c->d_clr_spheres) return RTUF_OK;
  std::vector<ClearanceSphere> sorted; std::vector<uint32_t> slots;
  { const int rc = build_clearance_spheres(c, sorted, slots); if (rc != RTUF_OK) return rc; }
  hipSetDevice(c->device);
  if (!c->d_clr_spheres) HIP_TRY(c, dev_alloc(c, &c->d_clr_spheres, (size_t)kMaxClearanceSpheres * sizeof(ClearanceSphere)));
  if (!c->d_clr_slot_label) HIP_TRY(c, dev_alloc(c, &c->d_clr_slot_label, (size_t)kMaxClearanceLabels * sizeof(uint32_t)));
  if (!sorted.empty()) HIP_TRY(c, hipMemcpy(c->d_clr_spheres, sorted.data(), sorted.size() * sizeof(ClearanceSphere), hipMemcpyHostToDevice));
  if (!slots.empty()) HIP_TRY(c, hipMemcpy(c->d_clr_slot_label, slots.data(), slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->clr_spheres.swap(sorted); c->clr_slot_label.swap(slots);
  c->clr_dirty = false;
  return RTUF_OK;
}

// (no width rule: the tile and dilate kernels pack the bits of any width, and the clearance kernels read single pixels)
static int check_clearance_call(rtuf_context* c, int n, const void* in, const void* table, int n_labels, float max_distance)
{
  { const int rc = check_batch_call(c, n, in && table, false); if (rc != RTUF_OK) return rc; }
  if (n_labels < 1) return c->fail(RTUF_ERR_INVALID, "a clearance table needs at least one row per stream (n_labels=%d)", n_labels);
  if (!(max_distance > 0.0f)) return c->fail(RTUF_ERR_INVALID, "max_distance must be > 0 (+inf is allowed; got %g)", (double)max_distance);
  { const int rc = check_route(c, BatchRequest(Kind::Clearance, n, false)); if (rc != RTUF_OK) return rc; }      // (16UC1 or not: no refusal asks)
  { const int rc = need_intrinsics(c, n, c->d_cloud_intr); if (rc != RTUF_OK) return rc; }
  return ensure_clearance_spheres(c);
}

static BatchRequest clearance_request(int n, const void* d_depth, rtuf_link_clearance* d_table, int n_labels, float max_distance, bool u16)
{
  BatchRequest rq(Kind::Clearance, n, u16);
  rq.depth = static_cast<const float*>(d_depth); rq.clr = d_table; rq.n_labels = n_labels; rq.max_distance = max_distance;
  return rq;
}

static int link_clearance_device(rtuf_context* c, int n, const void* d_depth, rtuf_link_clearance* d_table, int n_labels, float max_distance, bool u16)
{
  KIDS_NEXT(c, link_clearance_device(k, n, d_depth, d_table, n_labels, max_distance, u16));
  if (!c) return RTUF_ERR_INVALID;
  const int rc = check_clearance_call(c, n, d_depth, d_table, n_labels, max_distance);
  if (rc != RTUF_OK) return rc;
  if ((uintptr_t)d_table & 7u) return c->fail(RTUF_ERR_INVALID, "d_table must be 8-byte aligned");
  return submit_device(c, clearance_request(n, d_depth, d_table, n_labels, max_distance, u16));
}

int rtuf_link_clearance_batch_device(rtuf_context* c, int n, const float* d_depth, rtuf_link_clearance* d_table, int n_labels, float max_distance)
{
  return link_clearance_device(c, n, d_depth, d_table, n_labels, max_distance, false);
}

int rtuf_link_clearance_batch_device_u16(rtuf_context* c, int n, const uint16_t* d_depth, rtuf_link_clearance* d_table, int n_labels, float max_distance)
{
  return link_clearance_device(c, n, d_depth, d_table, n_labels, max_distance, true);
}

// host planes, synchronous: planes up, table down
static int link_clearance_host(rtuf_context* c, int n, const void* const* depth_in, rtuf_link_clearance* table_out, int n_labels, float max_distance, bool u16)
{
  KIDS_NEXT(c, link_clearance_host(k, n, depth_in, table_out, n_labels, max_distance, u16));
  if (!c) return RTUF_ERR_INVALID;
  { const int rc = check_clearance_call(c, n, depth_in, table_out, n_labels, max_distance); if (rc != RTUF_OK) return rc; }
  BatchRequest rq(Kind::Clearance, n, u16);
  rq.n_labels = n_labels; rq.max_distance = max_distance;
  HostPlanes hp{};
  hp.depth = depth_in; hp.clr_table = table_out;
  return submit_host_planes(c, rq, hp);
}

int rtuf_link_clearance_batch(rtuf_context* c, int n, const float* const* depth_in, rtuf_link_clearance* table_out, int n_labels, float max_distance)
{
  return link_clearance_host(c, n, reinterpret_cast<const void* const*>(depth_in), table_out, n_labels, max_distance, false);
}

int rtuf_link_clearance_batch_u16(rtuf_context* c, int n, const uint16_t* const* depth_mm_in, rtuf_link_clearance* table_out, int n_labels, float max_distance)
{
  return link_clearance_host(c, n, reinterpret_cast<const void* const*>(depth_mm_in), table_out, n_labels, max_distance, true);
}

int rtuf_wait_oldest(rtuf_context* c)
{
  if (!c) return RTUF_ERR_INVALID;
  if (!c->kids.empty()) {
    if (c->order.empty()) return RTUF_OK;
    rtuf_context* k = c->kids[c->order.front()];
    c->order.pop_front();
    const int rc = rtuf_wait_oldest(k);
    if (rc < 0) c->error = k->error;
    return rc;
  }
  hipSetDevice(c->device);
  return c->pending ? retire_oldest(c) : RTUF_OK;
}

int rtuf_host_alloc(rtuf_context* c, size_t bytes, void** out)
{
  KIDS_ONE(c, 0, rtuf_host_alloc(k, bytes, out));
  if (!c || !out || !bytes) return RTUF_ERR_INVALID;
  hipSetDevice(c->device);
  void* p = nullptr;
  HIP_TRY(c, hipHostMalloc(&p, bytes));
  c->pinned.push_back(p);
  *out = p;
  return RTUF_OK;
}

int rtuf_host_free(rtuf_context* c, void* p)
{
  if (!c) return RTUF_ERR_INVALID;
  if (!c->kids.empty()) {
    if (!p) return RTUF_OK;
    const int rc = rtuf_sync(c);           // no transfer of any pipeline may still target the block
    if (rc < 0) return rc;
    KIDS_ONE(c, 0, rtuf_host_free(k, p));
  }
  if (!p) return RTUF_OK;
  hipSetDevice(c->device);
  auto it = std::find(c->pinned.begin(), c->pinned.end(), p);
  if (it == c->pinned.end()) return c->fail(RTUF_ERR_INVALID, "not a block of rtuf_host_alloc");
  const int rc = rtuf_sync(c);          // no transfer may still target the block
  if (rc != RTUF_OK) return rc;
  c->pinned.erase(it);
  HIP_TRY(c, hipHostFree(p));
  return RTUF_OK;
}

int rtuf_filter(rtuf_context* c, const unsigned char* buffer, const double* projection, int width, int height)
{
  if (c && !c->kids.empty()) {
    // the single-stream call runs on the first pipeline; its projection is a setter like any other (all pipelines)
    if (projection) { const int rc_ = rtuf_set_camera(c, 0, projection, nullptr, nullptr); if (rc_ < 0) return rc_; }
    KIDS_ONE(c, 0, rtuf_filter(k, buffer, nullptr, width, height));
  }
  if (!c || !buffer) return RTUF_ERR_INVALID;
  if (width != c->width || height != c->height)
    return c->fail(RTUF_ERR_INVALID, "image size %dx%d differs from the context's %dx%d (the reference re-runs initGL here; create a new context instead)",
                   width, height, c->width, c->height);
  if (projection) { const int rc = rtuf_set_camera(c, 0, projection, nullptr, nullptr); if (rc != RTUF_OK) return rc; }
  const size_t plane = (size_t)width * height;
  c->single_masked.resize(plane);
  c->single_mask.resize(plane);
  const float* in = reinterpret_cast<const float*>(buffer);
  float* mo = c->single_masked.data();
  uint8_t* mk = c->single_mask.data();
  return rtuf_filter_batch(c, 1, &in, &mo, &mk);
}

const float* rtuf_get_masked_depth(const rtuf_context* c) { if (c && !c->kids.empty()) c = c->kids[0]; return (c && !c->single_masked.empty()) ? c->single_masked.data() : nullptr; }
const uint8_t* rtuf_get_mask(const rtuf_context* c) { if (c && !c->kids.empty()) c = c->kids[0]; return (c && !c->single_mask.empty()) ? c->single_mask.data() : nullptr; }

int rtuf_get_stats(rtuf_context* c, rtuf_stats* out)
{
  if (!c || !out) return RTUF_ERR_INVALID;
  if (!c->kids.empty()) {
    // counters and last-batch times of the pipeline that ran last (cover_pass, cover_tiles, work_items ... are that
    // pipeline's: each decides about its cover pass on its own); event sums, regrowths, memory and graph counts over all pipelines
    *out = c->kids[c->last_kid]->stats;
    out->bin_capacity = c->kids[c->last_kid]->capacity;
    out->raster_lanes = (uint32_t)c->kids[c->last_kid]->n_lanes; out->launch_group = (uint32_t)c->kids[c->last_kid]->group;
    out->counter_blocks = (uint32_t)c->kids[c->last_kid]->max_groups;
    out->regrowths = 0; out->timed_batches = 0; out->device_bytes = 0;
    out->graphs_enabled = 1u; out->graph_hits = out->graph_misses = 0; out->lanes_side_by_side = c->lanes_share_queue ? 0u : 1u;
    for (const rtuf_context* k : c->kids) { out->device_bytes += k->device_bytes; out->graphs_enabled &= k->graphs_ok ? 1u : 0u; out->graph_hits += k->graph_hits; out->graph_misses += k->graph_misses; }
    out->sum_ms_pose = out->sum_ms_setup = out->sum_ms_raster = out->sum_ms_compare = out->sum_ms_total = out->sum_ms_clip = 0;
    for (const rtuf_context* k : c->kids) {
      out->regrowths += k->stats.regrowths; out->timed_batches += k->stats.timed_batches;
      out->sum_ms_pose += k->stats.sum_ms_pose; out->sum_ms_setup += k->stats.sum_ms_setup; out->sum_ms_raster += k->stats.sum_ms_raster;
      out->sum_ms_compare += k->stats.sum_ms_compare; out->sum_ms_total += k->stats.sum_ms_total; out->sum_ms_clip += k->stats.sum_ms_clip;
    }
    return RTUF_OK;
  }
  *out = c->stats;
  out->bin_capacity = c->capacity;
  out->device_bytes = c->device_bytes;
  out->raster_lanes = (uint32_t)c->n_lanes; out->launch_group = (uint32_t)c->group;
  out->counter_blocks = (uint32_t)c->max_groups;
  out->graphs_enabled = c->graphs_ok ? 1u : 0u; out->graph_hits = c->graph_hits; out->graph_misses = c->graph_misses;
  out->lanes_side_by_side = c->lanes_share_queue ? 0u : 1u;
  return RTUF_OK;
}

#ifdef RTUF_LANECOUNT
// instrumented builds only (scripts/lane_util.sh): lane slots issued / lanes live per instrumented loop, last retired batch
int rtuf_debug_lane_counts(rtuf_context* c, unsigned long long* slots, unsigned long long* live, int n)
{
  if (!c || !slots || !live) return RTUF_ERR_INVALID;
  if (!c->kids.empty()) c = c->kids[c->last_kid];
  for (int i = 0; i < n && i < kLaneLoops; i++) { slots[i] = c->lane_slots[i]; live[i] = c->lane_live[i]; }
  return kLaneLoops;
}
// ... and which wave did the work (scripts/wave_roles.sh): 4 words per loop (trips with a live lane, by wave role), then
// kRoleTables tables of 4 x 4 (role against SIMD) for the set-up kernel and as many for the tile kernel
int rtuf_debug_wave_roles(rtuf_context* c, unsigned long long* words, int n)
{
  if (!c || !words) return RTUF_ERR_INVALID;
  if (!c->kids.empty()) c = c->kids[c->last_kid];
  for (int i = 0; i < n && i < kLaneRoleWords; i++) words[i] = c->lane_roles[i];
  return kLaneRoleWords;
}
#endif

int rtuf_enable_timing(rtuf_context* c, int on)
{
  KIDS_ALL(c, rtuf_enable_timing(k, on));
  if (!c) return RTUF_ERR_INVALID;
  c->timing = on < 0 ? 0 : (on > 3 ? 1 : on);
  c->timing_seq = 0;
  for (double& v : c->acc_ms) v = 0;
  c->acc_batches = 0;
  return RTUF_OK;
}

int rtuf_debug_read_zsurface(rtuf_context* c, int n, float* host_out)
{
  KIDS_ONE(c, c->last_kid, rtuf_debug_read_zsurface(k, n, host_out));
  if (!c || !host_out) return RTUF_ERR_INVALID;
  const float* zs = c->lane[c->last_lane].d_zsurface;
  if (!(c->params.flags & RTUF_FLAG_TWO_KERNEL) || !zs) return c->fail(RTUF_ERR_STATE, "z-surface exists only in two-kernel mode");
  if (n <= 0 || n > c->group) return c->fail(RTUF_ERR_INVALID, "z-surface holds the last launch group (at most %d streams)", c->group);
  hipSetDevice(c->device);
  sync_lanes(c);
  HIP_TRY(c, hipMemcpy(host_out, zs, (size_t)n * c->width * c->height * sizeof(float), hipMemcpyDeviceToHost));
  return RTUF_OK;
}

}  // extern "C"
