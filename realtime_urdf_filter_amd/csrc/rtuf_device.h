// rtuf_device.h -- device-side data layout shared by the HIP kernels and the host API.
//
// HBM layout (all arrays owned by one rtuf_context, one GPU):
//   static geometry, uploaded once by rtuf_finalize_models()
//     chunks Chunk[C]    <= 256 triangles of ONE draw call (a compact patch: Morton order of the
//                        centroids) + the <= 256 distinct vertices they use + bounding box   64 B / chunk
//     cverts float4[Vc]  object-space positions, grouped per chunk        16 B / vertex
//     ctris  u32[T]      3 x 10-bit chunk-local vertex ids                 4 B / triangle
//                        (draw-order sequence numbers in corder, parallel to ctris; 0 = background)
//     draws  Draw[D]     link id + the glScalef/glTranslatef of the draw
//   per frame, per stream s (slot within the batch)
//     cams   Camera[N]   projection / camera_offset_inv / camera_tf as f64
//     link_tf f64[N][L][16]                                         (two slots: one per batch in flight)
//     mvp    f32[N][D][16]  written by pose_kernel;  bg BgInfo[N];  items WorkItem[] written by cull_kernel (one list per raster lane)
//     depth  f32[N][H][W] in, masked f32[N][H][W] + mask u8[N][H][W] out
//     pt_plane f32[max_streams][H][W]  point list batches only, one per batch slot: the virtual depth the slot's batch renders
//                                      and its points kernel reads (empty pixels +inf)
//   rasteriser working set of ONE RASTER LANE (a context has one to three: a lane is a HIP stream plus the arrays below; the
//   launch groups of a batch alternate between the lanes, so one group's set-up runs under the other's tile kernel),
//   per stream g of the launch group and screen tile
//     bin_hdr   BinHeader[G][tiles]   records binned from the front (small boxes) and from the back of the bin, and the tile's
//                                     cover (nearest triangle that covers the WHOLE tile): 16 bytes, one scalar load in the tile kernel
//     bins      PackedTri[G][tiles][capacity]  (32 B records: small boxes from the front, larger from the back)
//     fbin_count u32[G][tiles], fbins Frag[G][tiles][fcapacity]    (pixels of small triangles, 8 B; top bit of the count: the
//                                                                    record bin holds a near record, see KeyFmt)
//     clip_list ClipItem[shards][clip_capacity]   triangles that cross a frustum plane (set-up kernel -> clip kernel)
//     big_list  BigRec[shards][big_capacity]      records over more than 4 tiles (set-up / clip kernel -> bigrec_kernel)
//     zsurface  f32[G][H][W]                       two-kernel mode, silhouette dilation and link padding only
//     slots     u16[G][H][W]                       link padding only: the link slot of every pixel's winner, beside the z-surface
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtuf_routes.h"

namespace rtuf {

// Timing experiments (scripts/ablate_*.sh) skip work and produce WRONG images.  They exist only in a library
// built with -DRTUF_ABLATE (lib/variants/librtuf_ablate.so); the product library contains none of that code and
// rtuf_create / rtuf_set_params reject the flag bits.
#ifdef RTUF_ABLATE
#define RTUF_ABL(flags, bits) (((flags) & (bits)) != 0u)
#else
#define RTUF_ABL(flags, bits) false
#endif

#ifndef RTUF_TILE_W
#define RTUF_TILE_W 64
#endif
#ifndef RTUF_TILE_H
#define RTUF_TILE_H 32
#endif
constexpr int kTileW = RTUF_TILE_W;      // screen tile of one raster workgroup (LDS: 8 B per pixel; 64x32 = 16 KB)
constexpr int kTileH = RTUF_TILE_H;
constexpr int kBlock = 256;
#ifndef RTUF_TILE_THREADS
#define RTUF_TILE_THREADS 256
#endif
constexpr int kTileThreads = RTUF_TILE_THREADS;   // threads of a tile workgroup
#ifndef RTUF_MAX_CHUNK_VERTS
#define RTUF_MAX_CHUNK_VERTS 256
#endif
constexpr int kMaxChunkVerts = RTUF_MAX_CHUNK_VERTS;     // unique vertices per set-up chunk (one per lane; LDS: 24 B each per stream)
#ifndef RTUF_STREAMS_PER_BLOCK
#define RTUF_STREAMS_PER_BLOCK 3
#endif
constexpr int kStreamsPerBlock = RTUF_STREAMS_PER_BLOCK;     // streams a set-up workgroup loops over per chunk

// Bias of the 20-bit snapped coordinates in a PackedTri.  In-frustum vertices snap to [-128, W*256 + 128]; the
// clipper's interpolation is rounded, so its vertices may land a few units outside (seen: -129): 1024 leaves room
// on both sides (2048*256 + 128 + 2*1024 < 2^20).
constexpr int kCoordBias = 1024;

struct alignas(16) TriRec {     // 64 B: one rasterisable triangle inside one tile bin
  int32_t A[3];                 // edge i is inside  <=>  A[i]*px + B[i]*py + C[i] > 0
  int32_t B[3];
  int32_t C[3];
  float a0, dzdx, dzdy;         // z(px,py) = fma(dzdy, py, fma(dzdx, px, a0))
  uint32_t bbx;                 // x0 | x1 << 16   (inclusive pixel bounds)
  uint32_t bby;                 // y0 | y1 << 16
  uint32_t order;               // draw-order sequence number of the source triangle
  uint32_t pad;
};
static_assert(sizeof(TriRec) == 64, "TriRec must be 64 bytes");

struct alignas(16) PackedTri {  // 32 B: what a triangle bin stores; the tile kernel rebuilds TriRec from it
  unsigned long long v01;       // (x0+bias) | (y0+bias) << 20 | (x1+bias) << 40   snapped 1/256-px coordinates,
  unsigned long long v12;       // (y1+bias) | (x2+bias) << 20 | (y2+bias) << 40   already oriented (area > 0)
  float a0, dzdx, dzdy;         // z plane
  uint32_t order;               // draw-order key (29 bits) | kNearBit
};
static_assert(sizeof(PackedTri) == 32, "PackedTri must be 32 bytes");
// Set in PackedTri.order when the record may produce a window z <= 0.5 somewhere in its box (geometry within about twice
// the near distance of the camera), where the float z the shader sees is finer than the 24-bit depth: only such records
// are looked at by the tile kernel's exact-z pass.
constexpr uint32_t kNearBit = 1u << 31;
constexpr uint32_t kOrderMask = (1u << 29) - 1u;

// A record whose bounding box touches more than kCoopTiles tiles is not appended to its bins by the lane that made it
// (a wave with a run of wall triangles would append hundreds of (record, tile) pairs one record after the other while
// the rest of the GPU idles): set-up and clip kernel put it on a list, bigrec_kernel gives every list entry a wave.
struct alignas(16) BigRec {
  PackedTri pk;
  uint32_t slot;                // stream slot within the in-flight group
  uint32_t pad[3];
};
static_assert(sizeof(BigRec) == 48, "BigRec is three 16-byte stores");

// 8 B: one covered pixel of a small (<= 4x4 pixel centres, single tile) triangle, ready for the depth
// test:  z24 << 40 | order << kFragPosBits | position in the tile (y * kTileW + x).
// Fragments carry no z plane, so triangles that may win with window z <= 0.5 (where the float z the
// shader sees is finer than 24 bits) are never resolved to fragments; they stay records.
constexpr int kFragPosBits = 11;
constexpr uint32_t kMaxOrder = (1u << (40 - kFragPosBits)) - 1u;    // draw-order keys must fit 29 bits
static_assert(kTileW * kTileH <= (1 << kFragPosBits), "tile positions must fit the fragment's position field");
static_assert(kMaxOrder == kOrderMask, "records and fragments carry the same 29-bit draw-order keys");
struct alignas(8) Frag { unsigned long long v; };
static_assert(sizeof(Frag) == 8, "Frag must be 8 bytes");

// Per-bin header: the two fill counters of the record bin and the tile's cover -- the nearest triangle that covers the whole
// tile (bigrec_kernel<0>): largest 24-bit depth it has there << 32 | its index in big_list; kNoCover = none.
constexpr unsigned long long kNoCover = ~0ull;
struct alignas(16) BinHeader {
  uint32_t count[2];             // records binned from the front (boxes of at most kFrontArea pixel centres) / from the back
  unsigned long long cover;
};
static_assert(sizeof(BinHeader) == 16, "one scalar load, one store");

struct Chunk {                  // <= 256 consecutive triangles of one draw + their vertex list
  uint32_t tri_begin;           // into ctris
  uint32_t tri_count;
  uint32_t vert_begin;          // into cverts
  uint32_t vert_count;          // <= kMaxChunkVerts
  uint32_t draw;
  uint32_t model;
  uint32_t reserved;
  uint32_t pad;
  float center[3];              // object-space bounding box of the chunk's vertices: centre ...
  uint32_t pad1;
  float half[3];                // ... and half extents
  uint32_t pad2;
};

struct Draw {
  uint32_t link;                // global link index (row of link_tf)
  uint32_t pre_op;              // RTUF_OP_*
  float op[3];
  uint32_t model;
  uint32_t pad[2];
};

struct Camera {
  double projection[16];
  double offset_inv[16];
  double cam_tf[16];
  double shift[2];              // camera_tx_, camera_ty_ (src/urdf_filter.cpp:607-611): applied by the forward-kinematics
                                // kernels when they derive cam_tf from a robot frame; a host-supplied cam_tf has them applied already
};

struct alignas(16) ClipItem {   // one triangle that crosses a frustum plane; self-contained, so the clip
  uint32_t slot;                // kernel's loads depend on nothing but the item (stream slot within the group)
  uint32_t draw;
  uint32_t vert_begin;          // of the triangle's chunk, into cverts
  uint32_t packed;              // 3 x 10-bit chunk-local vertex ids
  uint32_t order;               // draw-order key (0 = background quad)
  uint32_t pad[3];
};

// Device-side statistics / overflow detection.  One hot word would serialise every workgroup at
// a single L2 atomic unit (~12 ns per atomic), so everything is sharded over kCounterShards
// cache-line-sized slots that the host sums after the batch.
#ifndef RTUF_COUNTER_SHARDS
#define RTUF_COUNTER_SHARDS 64
#endif
constexpr int kCounterShards = RTUF_COUNTER_SHARDS;
constexpr int kLaneLoops = 48;           // instrumented loops (and histogram buckets) of a -DRTUF_LANECOUNT build
// (same build) per loop four words, then per kernel (set-up, tile) kRoleTables tables of 4 x 4, then two words: see
// CounterShard::lane_roles
constexpr int kRoleTables = 2;
constexpr int kLaneRoleWords = 4 * kLaneLoops + 2 * kRoleTables * 16 + 2;
struct alignas(128) CounterShard {
  unsigned long long tris_binned;
  unsigned long long bin_entries;
  unsigned int clip_count;      // entries in this shard's segment of clip_list
  unsigned int max_bin_fill;
  unsigned int clip_overflow;
  unsigned int max_fbin_fill;
  unsigned long long frags;
  unsigned int uncovered;       // mask-bits output only: some pixel was reached by no fragment (see rtuf_filter_batch_bits*)
  unsigned int big_count;       // entries in this shard's segment of big_list (reset per in-flight group)
  unsigned int max_big_fill;    // largest big_count of the batch's groups (overflow detection)
  unsigned int cover_tiles;     // tiles whose initial depth keys came from a whole-cover triangle (statistics)
  unsigned int exact_tiles;     // tiles that ran the exact-z pass (statistics)
  unsigned int zero_items;      // set-up work items (chunk x <= 3 streams) none of whose triangles survived (statistics)
  unsigned long long occluded;  // (record, tile) pairs not appended because they lie behind a whole-cover triangle (statistics)
  unsigned long long raster_atomics;   // RTUF_COUNT builds only: depth tests issued by the tile kernel (LDS atomics)
  unsigned long long drawn_pixels;     // RTUF_COUNT builds only: pixels whose final key is not the background's
  unsigned int pad[10];
#ifdef RTUF_LANECOUNT
  // Lane-utilisation builds (scripts/lane_util.sh; never the product): per instrumented loop the lane slots its trips
  // issued (64 per wave and trip) and the lanes that were live in them, see kLane* in rtuf_kernels.hip.
  unsigned long long lane_slots[kLaneLoops];
  unsigned long long lane_live[kLaneLoops];
  // ... and which wave does the work: per loop and wave index within the workgroup (modulo 4) the trips with a live lane;
  // then, in shard 0 only, per kernel two tables of 4 x 4 -- waves started, by wave index and hardware SIMD, on the whole chip
  // and on one CU -- and per kernel the id (+ 1) of that CU
  unsigned long long lane_roles[kLaneRoleWords];
#endif
};
#ifndef RTUF_LANECOUNT
static_assert(sizeof(CounterShard) == 128, "CounterShard must be one 128-byte line");
#endif
struct alignas(128) WorkCount {
  unsigned int n_items;         // length of the launch group's work list (cull_kernel)
  unsigned int grid;            // work items the group's set-up launch covered (written by the set-up kernel itself: the batch's
                                // last kernel compares the two on the device, see BatchStatus)
  unsigned int pad[30];
};
struct Counters { CounterShard shard[kCounterShards]; WorkCount work; };

// One set-up workgroup's job: a chunk and up to kStreamsPerBlock stream slots (of the in-flight
// group) whose frustum the chunk's bounding sphere touches; 0xffff = unused.  Written by cull_kernel.
struct alignas(32) WorkItem {
  uint32_t chunk;
  uint32_t tri_begin;           // copies of the chunk's fields: the set-up workgroup needs no Chunk load
  uint32_t vert_begin;
  uint32_t reserved;
  uint32_t draw;
  uint16_t tri_count, vert_count;
  uint16_t slot[4];
};
static_assert(sizeof(WorkItem) == 32, "WorkItem is two 16-byte loads");
// Upper bound of the work items one chunk can produce for a launch group of `group` streams: cull_kernel
// compacts the visible streams per block of kBlock stream slots and rounds EACH block's count up to whole
// items, so a group of more than kBlock streams can need more than ceil(group / kStreamsPerBlock).  Sizes the
// items array and the set-up kernel's worst-case grid.
inline int max_items_per_chunk(int group)
{
  int n = 0;
  for (int first = 0; first < group; first += kBlock) {
    const int in_block = group - first < kBlock ? group - first : kBlock;
    n += (in_block + kStreamsPerBlock - 1) / kStreamsPerBlock;
  }
  return n;
}

// Per stream: what the background quad (src/urdf_filter.cpp:589-597) amounts to, computed once per batch
// by pose_kernel so that the tile kernel's workgroups do no per-stream arithmetic of their own.
struct alignas(16) BgInfo {
  float z;                      // window z of the quad when it is a constant full-screen plane
  uint32_t mode;                // 1 = constant full-screen plane (analytic), 0 = draw it as geometry
  float thr;                    // compare threshold of that depth: sensor > thr <=> filtered
  uint32_t z24;                 // its 24-bit depth-buffer value
};

// Device-resident status word of a batch slot (rtuf_batch_status_device): the low 16 bits count the launch groups of the batch
// that have not finished yet (set by pose_kernel, the first kernel of a batch; every group's publish_counters workgroup, the
// last kernel of its lane, takes one off), the bits above say why the batch's planes are NOT final -- a working buffer was too
// small, and the host will run the batch again when it retires it.  0 <=> every group finished and nothing overflowed.
constexpr uint32_t kStatusPendingMask = 0xffffu;
constexpr uint32_t kStatusBinOverflow = 1u << 16;     // a record or fragment bin was fuller than its capacity
constexpr uint32_t kStatusClipOverflow = 1u << 17;    // the clip list was too short
constexpr uint32_t kStatusBigOverflow = 1u << 18;     // the many-tile list was too short
constexpr uint32_t kStatusGridShort = 1u << 19;       // the set-up grid did not cover the work list
constexpr uint32_t kStatusUncovered = 1u << 20;       // mask-bits output: a pixel no fragment reached (retiring the batch fails)

// kernel argument blocks (passed by value) and host-callable launchers (rtuf_kernels.hip)
struct PoseArgs {
  const Camera* cams;        // [n_streams]
  const double* link_tf;     // [n_streams][n_links][16]
  const Draw* draws;         // [n_draws]
  float* mvp;                // [n_streams][n_draws + 1][16]
  BgInfo* bg;                // [n_streams]
  float sc_num, sc_off, max_diff;   // to_linear_depth constants (host-computed, see shade_consts) and the threshold
  Counters* counters;        // [n_counters]: one block per launch group of the batch, zeroed by this kernel
  int n_counters;
  uint32_t* status;          // the batch slot's status word: set to n_counters (launch groups still to finish) by this kernel
  int n_streams, n_draws, n_links;
  float z_far;
  int width, height;
};

struct SetupArgs {
  const float4* cverts;          // chunk-local vertex lists (object space)
  const uint32_t* ctris;         // 3 x 10-bit chunk-local vertex ids per triangle
  const uint32_t* corder;        // draw-order sequence number per triangle (>= 1; 0 = background quad), parallel to ctris
  const Chunk* chunks;
  const float* mvp;              // [n_streams][n_draws + 1][16]
  const uint64_t* model_mask;    // [n_streams] bit m set: stream renders model m
  const BgInfo* bg;              // [n_streams]
  PackedTri* bins;               // [G][tiles][capacity]   triangles that are not resolved to fragments
  BinHeader* bin_hdr;            // [G][tiles]
  Frag* fbins;                   // [G][tiles][fcapacity]  covered pixels of the small (<= 4x4, single-tile) boxes
  uint32_t* fbin_count;          // [G][tiles]
  uint32_t fcapacity;
  ClipItem* clip_list;
  float4* clip_spill;            // clip kernel: polygon vertices beyond the eight per thread that live in LDS
  BigRec* big_list;              // [kCounterShards][big_capacity]  many-tile records, appended to their bins by bigrec_kernel
  uint32_t big_capacity;         // per shard segment
  WorkItem* items;               // [n_chunks * ceil(group / kStreamsPerBlock)] visible (chunk, streams) jobs of this group
  Counters* counters;
  int n_chunks;
  int group_base;                // first stream slot of this in-flight group
  int group_size;
  int n_draws;
  int width, height, tiles_x, tiles_y;
  uint32_t capacity;
  uint32_t clip_capacity;        // per shard segment
  uint32_t bg_chunk;             // index of the background-quad chunk
  uint32_t flags;                // rtuf_params.flags
};

struct TileArgs {
  const PackedTri* bins;
  BinHeader* bin_hdr;            // [G][tiles], reset to "nothing binned, no cover" by this kernel after use
  const Frag* fbins;
  uint32_t* fbin_count;          // reset to 0 by this kernel after use
  uint32_t fcapacity;
  const float* depth;            // [n][H][W]   (f32 metres) or, with io_u16, uint16 millimetres
  float* masked;                 // [n][H][W]   same element type as depth
  uint8_t* mask;                 // [n][H][W] or nullptr
  uint32_t* bits;                // mask-only output: [n][H][ceil(W/32)] words, pixel x = bit x % 32 of word x / 32; masked / mask unused
  float* zsurface;               // [G][H][W]  (two-kernel mode)
  const BgInfo* bg;              // [n]
  Counters* counters;
  const BigRec* big_list;        // the record a bin's cover entry points to
  int group_base, group_size;
  int width, height, tiles_x, tiles_y;
  uint32_t capacity;
  uint32_t flags;
  float z_near, z_far, max_diff, replace_value;
  float sc_num, sc_off;          // z_near*z_far/(z_near-z_far) and z_far/(z_far-z_near) in float, as the shader computes them
  int io_u16;                    // 16UC1 in/out fused into the kernel (src/urdf_filter.cpp:287-288, :309-312)
  int key_shift;                 // depth keys: draw order << key_shift in the low word, the float z's low bits below it (KeyFmt)
  int fast_div;                  // the threshold's division may run without its scaling / fix-up instructions (host: fast_div_admitted, rtuf_numerics.h)
  // Which kernel reads the fields below is the launch's TileVariant (rtuf_routes.h), never their nullness.
  // link labels (appended: the fields above keep their kernarg offsets): variants with `labels` (tile_labels_kernel & co.)
  uint16_t* labels;              // [n][H][W] link label of every pixel's winner, 8-byte aligned; nullptr = none
  const uint16_t* order_labels;  // [n_tris + 1] label of every draw order (entry 0, background / no fragment: 0)
  // per-link depth thresholds (appended): variants with `thresh` (tile_thresh_kernel, tile_resid_kernel; never the z-surface route)
  const float* order_thr;        // [n_tris + 1] threshold of every draw order's link (entry 0, the background quad: max_diff)
  // virtual depth planes (appended): TileOut::Render (tile_render_kernel); depth, masked, mask, bits unused.
  float* virtual_out;            // [n][H][W] virtual depth of every pixel's winner (f32 metres or, with io_u16, uint16 millimetres)
  float empty_value;             // ... and what a pixel holds where the background quad won or nothing was drawn
  // link residual tables (appended): TileOut::Residual (tile_resid_kernel); masked, mask, bits, labels unused; order_labels is
  // always set, order_thr as for a filter batch.
  unsigned long long* resid_table;   // [n][n_labels] rows of eight 64-bit sums (rtuf_link_residuals), zeroed before the kernel
  int n_labels;
};

struct CompareArgs {
  const float* depth;     // group base
  const float* zsurface;  // group base
  float* masked;
  uint8_t* mask;          // may be nullptr
  size_t n_pixels;        // multiple of 4 handled vectorised, tail scalar
  float z_near, z_far, max_diff, replace_value;
  float sc_num, sc_off;
  int io_u16;
  int fast_div;
};

// Silhouette dilation (rtuf_params.silhouette_dilation_px > 0): dilate_compare_kernel takes the place of compare_kernel.  Per
// pixel it shades with z' = the smallest non-NaN z-surface value of the (2r+1)^2 window around it, clipped to the stream's
// image (NaN when the window holds none), and writes the same outputs the compare kernel or the bit-packed tile kernel would.
constexpr int kMaxDilation = 16;
struct DilateArgs {
  const float* depth;     // [n][H][W] sensor planes (f32 metres or, with io_u16, uint16 millimetres): the whole batch
  const float* zsurface;  // [G][H][W] the lane's z-surface (slot 0 = stream group_base)
  float* masked;          // [n][H][W] same element type as depth; unused with bits
  uint8_t* mask;          // [n][H][W] or nullptr; unused with bits
  uint32_t* bits;         // mask-only output (rtuf_mask_bits_words layout) or nullptr
  Counters* counters;     // the launch group's block: BITS sets a shard's `uncovered`
  int group_base, group_size;
  int width, height;
  int radius;             // 1 .. kMaxDilation
  float max_diff, replace_value;
  float sc_num, sc_off;
  int io_u16;
  int fast_div;
};

// Link padding (include/rtuf.h, LINK PADDING; rtuf_set_link_padding): pad_compare_kernel takes the place of compare_kernel.
// The tile kernel left the z-surface and, in its label plane, the link slot of every pixel's winner (0: background or nothing
// drawn, else 1 + the context-global link).  A source pixel q spreads its z over the disc of R2(q) = link_padding_reach2
// (rtuf_numerics.h) around it; per pixel the kernel shades with the smallest z that reaches it (NaN when none does) and
// writes the outputs dilate_compare_kernel would.
struct PadArgs {
  const float* depth;     // [n][H][W] sensor planes (f32 metres or, with io_u16, uint16 millimetres): the whole batch
  const float* zsurface;  // [G][H][W] the lane's z-surface (slot 0 = stream group_base)
  const uint16_t* slots;  // [G][H][W] the lane's link slot plane, laid out like the z-surface
  const float* slot_pad;  // [n_links + 1] padding of every link slot in metres (entry 0: 0)
  const float* focal;     // [max_streams] (float)max(fx, fy) of every stream
  float* masked;          // [n][H][W] same element type as depth; unused with bits
  uint8_t* mask;          // [n][H][W] or nullptr; unused with bits
  uint32_t* bits;         // mask-only output (rtuf_mask_bits_words layout) or nullptr
  Counters* counters;     // the launch group's block: BITS sets a shard's `uncovered`
  int group_base, group_size;
  int width, height;
  float max_diff, replace_value;
  float sc_num, sc_off;
  int io_u16;
  int fast_div;
};

// Filtered point clouds (include/rtuf.h, FILTERED POINT CLOUDS): the cloud kernels of one launch group.  They run behind the
// group's tile (or dilate) kernel on its lane and read the mask bits that kernel wrote; streams are batch-absolute.
struct CloudIntrinsics;
struct CloudArgs {
  const float* depth;            // [n][H][W] sensor planes (f32 metres or, with io_u16, uint16 millimetres): the whole batch
  const uint32_t* bits;          // [n][H][ceil(W/32)] mask bits of the batch (the library's buffer of the batch slot)
  const CloudIntrinsics* intr;   // [max_streams] kx, ky, cx, cy
  float* points;                 // organized: [n][H][W][3]; compacted: [n][capacity][3]
  uint32_t* index;               // compacted: [n][capacity] v * W + u of every entry, or nullptr
  uint32_t* counts;              // compacted: [n] kept pixels of every stream (the full number)
  uint32_t* row_count;           // compacted: [n][H] kept pixels of every row (scratch of the batch slot)
  uint32_t* row_start;           // compacted: [n][H] exclusive scan of row_count per stream (scratch of the batch slot)
  int group_base, group_size;
  int width, height;
  int capacity;                  // compacted: entries per stream; 0: the organized form
  int io_u16;
};

// Link clearance tables (include/rtuf.h, LINK CLEARANCE TABLES): the clearance kernels of one launch group.  Like the cloud
// kernels they run behind the group's tile (or dilate) kernel on its lane and read the mask bits it wrote; streams are
// batch-absolute.  The context's spheres are sorted by label (label 0 left out); a batch uses the first n_spheres of them,
// those whose label is below n_labels.
constexpr int kMaxClearanceSpheres = 4096;   // spheres of a context
constexpr int kMaxClearanceLabels = 256;     // distinct non-zero labels among them (the label slots of a workgroup's LDS rows)
constexpr int kClearanceTrip = 1024;         // spheres staged in LDS at a time
struct alignas(16) ClearanceSphere {         // one sphere as rtuf_set_link_spheres gave it
  float x, y, z, r;                          // centre in the link's vertex frame, radius
  uint32_t link;                             // global link index (row of link_tf)
  uint32_t model;
  uint32_t label_slot;                       // label | slot << 16: slot = rank of the label among the distinct labels in use
  uint32_t id;                               // context-global id: model order, then list order
};
static_assert(sizeof(ClearanceSphere) == 32, "two 16-byte loads");
struct ClearanceArgs {
  const float* depth;            // [n][H][W] sensor planes (f32 metres or, with io_u16, uint16 millimetres): the whole batch
  const uint32_t* bits;          // [n][H][ceil(W/32)] mask bits of the batch (the library's buffer of the batch slot)
  const CloudIntrinsics* intr;   // [max_streams] kx, ky, cx, cy
  const ClearanceSphere* spheres;// [n_spheres] sorted by label
  const uint32_t* slot_label;    // [n_slots] the label of every slot
  const Camera* cams;            // [n]
  const double* link_tf;         // [n][n_links][16]
  const uint64_t* model_mask;    // [n]
  float4* posed;                 // [max_streams][kMaxClearanceSpheres slots used: n_spheres]: camera-frame centre and radius; radius -1: not of this stream
  unsigned long long* table;     // [n][n_labels] rows of 16 bytes: while the batch runs {key, count, 0}, then rtuf_link_clearance
  int n_spheres, n_slots, n_links, n_labels;
  int group_base, group_size;
  int width, height;
  float max_distance;
  int io_u16;
};

// Point list batches (include/rtuf.h, POINT LIST BATCHES): the points kernel of one launch group.  It runs behind the group's
// tile_render_kernel on its lane and reads the virtual depth plane that kernel wrote (the batch slot's own, float, empty
// pixels +inf); streams are batch-absolute.  PointTransform: the 12 used entries of a stream's column-major matrix as floats
// (m[4 * c + r]; the last row is not read), on = 0: the stream takes its points as given.
struct PointIntrinsics;
struct alignas(16) PointTransform { float m[16]; uint32_t on; uint32_t pad[3]; };
constexpr int kMaxPointsRadius = 4;
constexpr int kMaxPointsCapacity = 1 << 24;
constexpr int kPointsPerThread = 4;
struct PointsArgs {
  const float* points;           // [n][capacity][3]
  const uint32_t* counts;        // [n], on the device: stream s judges entries j < min(counts[s], capacity)
  const float* virt;             // [max_streams][H][W] the slot's virtual depth plane
  const PointIntrinsics* intr;   // [max_streams] fx, fy, cx, cy
  const PointTransform* tf;      // [max_streams]
  uint8_t* verdict;              // [n][capacity]
  uint32_t* pixel;               // [n][capacity] v * W + u, 0xffffffff for a point that is not judged; or nullptr
  uint32_t* summary;             // [n][4] kept, filtered, outside, min(count, capacity); or nullptr.  Zeroed in front of the kernel
  int group_base, group_size;
  int width, height;
  int capacity, radius;
  float threshold;
  int wide;                      // points and pixel start on 16-byte boundaries, verdict on a 4-byte one, capacity % 4 == 0: a
                                 // thread's four points are three 16-byte loads, its verdicts one word, its pixels one 16-byte store
};

// Scene planes (include/rtuf.h, SCENE PLANES): per stream one float plane of the empty scene in metres, margins and a switch.
// The scene kernels of one launch group run behind whatever wrote the group's outputs and in front of the kernels that read
// its mask bits; streams are batch-absolute, and a stream whose filtering is disabled is skipped.
struct alignas(16) SceneStream { float abs_m, rel; uint32_t enabled, reserved; };
struct SceneArgs {
  const float* depth;            // [n][H][W] sensor planes (f32 metres or, with io_u16, uint16 millimetres): the whole batch
  const float* scene;            // [max_streams][H][W] the context's scene planes, float whatever the batch's element type
  const SceneStream* streams;    // [max_streams]
  float* masked;                 // Filter: [n][H][W], same element type as depth (may alias depth)
  uint8_t* mask;                 // Filter: [n][H][W] or nullptr
  uint32_t* bits;                // Bits / Cloud / Clearance: [n][H][ceil(W/32)], ORed into in place
  int group_base, group_size;
  int width, height;
  float replace_value;
  int io_u16;
  int wide;                      // every plane of the group starts on a 16-byte boundary and W % 4 == 0 (16UC1: W % 8 == 0): 16-byte accesses
};
// Learning: scene = scene_learned(scene, sensor, robot's bit) for streams 0 .. n - 1 (rtuf_numerics.h); bits are final.
struct SceneLearnArgs {
  const float* depth; const uint32_t* bits; float* scene;
  int n_streams, width, height, io_u16;
};

// Voxel occupancy grids (include/rtuf.h, VOXEL OCCUPANCY GRIDS): one insert into the context's grid, plane form (depth, bits,
// intr) or list form (points, counts, verdict).  Both run on lane 0 once everything in flight is retired, so the bits are
// final; streams 0 .. n_streams - 1.  The grid arrays are allocated in multiples of 16 bytes (voxel_clear_kernel).
struct VoxelArgs {
  float ox, oy, oz, inv;         // the grid: VoxelGrid's fields (rtuf_numerics.h)
  int nx, ny, nz;
  uint32_t* grid_bits;           // [ceil(n_voxels / 32)] ORed into
  uint32_t* grid_counts;         // [n_voxels] added to, modulo 2^32; or nullptr
  const PointTransform* world_tf;// [max_streams] world_from_optical (on = 0: none), or nullptr: no stream has one
  uint32_t* summary;             // [n][4] inserted, outside the grid, not kept, total; or nullptr.  Zeroed in front of the kernel
  // plane form
  const float* depth;            // [n][H][W] sensor planes (f32 metres or, with io_u16, uint16 millimetres)
  const uint32_t* bits;          // [n][H][ceil(W/32)] the final mask bits of these planes
  const CloudIntrinsics* intr;   // [max_streams]
  int width, height, io_u16;
  // list form
  const float* points;           // [n][capacity][3]
  const uint32_t* counts;        // [n] on the device
  const uint8_t* verdict;        // [n][capacity], 0 = taken; or nullptr: every entry is taken
  const PointTransform* point_tf;// [max_streams] rtuf_set_point_transforms' (applied first), or nullptr
  int capacity;
  int n_streams;
  int wide;                      // plane form: depth starts on a 16-byte (16UC1: 8-byte) boundary and W % 4 == 0; list form: the points
                                 // batch's rule (points on a 16-byte boundary, verdict on a 4-byte one, capacity % 4 == 0)
};
void launch_voxel_clear(uint32_t* p, size_t n_words, hipStream_t st);      // n_words % 4 == 0, p on a 16-byte boundary
void launch_voxel_insert(const VoxelArgs& a, hipStream_t st);              // a.points selects the list form

// Voxel free space (include/rtuf.h, VOXEL FREE SPACE): one carve of the context's free grid from the sensor planes of streams
// 0 .. n_streams - 1.  It runs on lane 0 once everything in flight is retired; the planes are only read.  The free words are
// allocated in multiples of 16 bytes, so the word pair of every wave of 64 voxels lies inside the array.
constexpr int kMaxCarveRadius = 4;
struct VoxelCarveArgs {
  float ox, oy, oz, size;        // the grid's origin and (float)voxel_size
  int nx, ny, nz;
  uint32_t n_voxels;
  uint32_t* free_bits;           // [ceil(n_voxels / 32)] ORed into, every word by one wave
  const PointTransform* inv_tf;  // [max_streams] optical_from_world (on = 0: the centre as it is), or nullptr: no stream has one
  const PointIntrinsics* intr;   // [max_streams] fx, fy, cx, cy
  const float* depth;            // [n][H][W] sensor planes (f32 metres or, with io_u16, uint16 millimetres)
  uint32_t* summary;             // [n][4] free, not free, not seen, n_voxels; or nullptr.  Zeroed in front of the kernel
  float margin;
  int radius, width, height, io_u16, n_streams;
};
void launch_voxel_carve(const VoxelCarveArgs& a, hipStream_t st);

struct FkArgs {
  const int32_t* parent;        // [F]
  const int32_t* joint_type;    // [F]
  const int32_t* depth;         // [F] distance from the root (0 for the root)
  const double* joint_origin;   // [F][12]  row-major 3x3 basis + origin
  const double* joint_axis;     // [F][3]
  const int32_t* link_frame;    // [L_model]
  const double* link_offset;    // [L_model][12]
  const double* q;              // [N][F]
  const double* root_tf;        // [N][12] or nullptr
  const uint8_t* enabled;       // [N] stream uses FK for this model
  double* link_tf;              // [N][L_total][16]
  Camera* cams;                 // [N]
  int n_streams, n_frames, n_links_model, link_base, n_links_total, camera_frame, max_depth;
};
void launch_fk(const FkArgs& a, hipStream_t st);
void launch_pose(const PoseArgs& a, hipStream_t st);
void launch_cull(const SetupArgs& a, hipStream_t st);
uint32_t launch_setup(const SetupArgs& a, uint32_t items_hint, bool sweep, hipStream_t st);    // returns the main grid size
void launch_clip(const SetupArgs& a, hipStream_t st);
size_t clip_spill_bytes(uint32_t clip_capacity);
void launch_bigrec(const SetupArgs& a, bool cover_pass, hipStream_t st);      // cover_pass: bigrec_kernel<0> runs first (and launch_tile gets a variant with `cover`)
void launch_init_headers(BinHeader* hdr, size_t n_bins, hipStream_t st);
// copies the counter blocks first, first + stride, ... (count of them) of a batch to the same places of the pinned host array
// ... and folds what they say about overflows into the batch's status word (PublishLimits: the capacities they are held against)
struct PublishLimits { uint32_t capacity, fcapacity, big_capacity; };
void launch_publish_counters(const Counters* src, Counters* host_dst, int first, int stride, int count, uint32_t* status, PublishLimits lim, hipStream_t st);
void launch_zero_residual_rows(unsigned long long* rows, size_t n_words, hipStream_t st);      // n_words 64-bit words from rows on
// the variant's instantiation for the launch's size; false, and nothing launched: there is none (tile_variant_legal(v) fails)
bool launch_tile(const TileArgs& a, TileVariant v, hipStream_t st);
void launch_compare(const CompareArgs& a, hipStream_t st);
void launch_dilate_compare(const DilateArgs& a, hipStream_t st);     // a.bits selects the mask-only variant, a.io_u16 the 16UC1 one
void launch_pad_compare(const PadArgs& a, hipStream_t st);           // as launch_dilate_compare
void launch_cloud(const CloudArgs& a, hipStream_t st);               // a.capacity selects the compacted form (count, scan, emit), a.io_u16 the 16UC1 variants
void launch_clearance(const ClearanceArgs& a, hipStream_t st);       // spheres, zero, clearance, finish: the group's rows of the table, a.io_u16 selects the 16UC1 variant
void launch_points(const PointsArgs& a, hipStream_t st);             // the group's rows of the summary to zero (a.summary), then points_filter_kernel
void launch_scene_apply(const SceneArgs& a, hipStream_t st);         // a.bits selects scene_apply_bits_kernel, else scene_apply_planes_kernel; a.io_u16 the 16UC1 variants
void launch_scene_learn(const SceneLearnArgs& a, hipStream_t st);
void launch_fill_f32(float* p, size_t n, float v, hipStream_t st);
void launch_spin(unsigned long long ticks, hipStream_t st);      // a one-wave kernel that idles for `ticks` of the 100 MHz clock

}  // namespace rtuf
