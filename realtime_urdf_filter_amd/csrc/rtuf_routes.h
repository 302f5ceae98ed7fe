// rtuf_routes.h -- which kernels a batch runs: the tile kernel's variant, and what runs behind it on the group's lane.
//
// The one place that decides it.  enqueue_batch (rtuf_api.cpp) asks route_of once, when a batch is first enqueued, keeps the
// Route with the batch slot (re-runs take it from there) and hands it to issue_plan; launch_tile (rtuf_kernels.hip) maps its
// TileVariant to a kernel instantiation, and tile_body asserts that the instantiation is a legal one.  A new batch kind, or a
// new variant of the tile kernel, starts here.
//
// Included by rtuf_device.h (so by the kernels and the host API) and by the CPU check tests/routes_check.cpp (plain g++, no
// ROCm headers), which holds route_of against a table written out by hand for every combination of its inputs.  Plain C++17.
#pragma once

namespace rtuf {

// What a caller can ask for (BatchRequest::kind).
enum class BatchKind { Filter, Bits, Render, Residual, Cloud, Clearance, Points };

// What the tile kernel leaves behind for every pixel:
//   Planes    masked depth plane + optional byte mask, compared in the kernel (the fused route)        tile_kernel & co.
//   ZSurface  the winners' window z, for compare_kernel, dilate_compare_kernel or pad_compare_kernel  tile_kernel<true>, tile_labels_kernel<true>
//             behind it (link padding: with `labels`, the plane then holds the winners' link slots)
//   Bits      one mask bit per pixel                                                                  tile_bits_kernel, tile_thresh_kernel
//   Render    the virtual depth plane, no sensor plane read                                           tile_render_kernel
//   Residual  no plane: per-label sums in a table                                                     tile_resid_kernel
enum class TileOut { Planes, ZSurface, Bits, Render, Residual };
constexpr int kTileOuts = 5;

// One instantiation of the tile kernel, but for the workgroup size (which launch_tile picks from the launch's size).
//   labels  the kernel also stores the link label plane
//   thresh  a drawn pixel is compared with its winner's link threshold instead of max_diff
//   u16     16UC1 planes in and out
//   cover   the batch ran the cover pass, so a bin's header may name a cover
struct TileVariant { TileOut out; bool labels, thresh, u16, cover; };

// The "never with" rules of the variants, all of them:
//   labels only beside Planes, ZSurface and Render (mask bits and residual tables have no label plane);
//   thresh only in Planes, Bits and Residual (the z-surface does not carry the winning link, a render batch compares nothing)
//     -- so labels and thresh together: Planes only;
//   the z-surface is float whatever the planes are: ZSurface has no u16 form (the kernel behind it converts).
constexpr bool tile_variant_legal(TileVariant v)
{
  const bool labels_ok = v.out == TileOut::Planes || v.out == TileOut::ZSurface || v.out == TileOut::Render;
  const bool thresh_ok = v.out == TileOut::Planes || v.out == TileOut::Bits || v.out == TileOut::Residual;
  return (!v.labels || labels_ok) && (!v.thresh || thresh_ok) && !(v.out == TileOut::ZSurface && v.u16);
}

// A variant as a small number (the dispatcher's switch, the plan's hash): distinct variants, distinct numbers.
constexpr int kTileVariantSlots = kTileOuts * 16;
constexpr int tile_variant_index(TileVariant v)
{
  return (int)v.out * 16 + (v.labels ? 8 : 0) + (v.thresh ? 4 : 0) + (v.u16 ? 2 : 0) + (v.cover ? 1 : 0);
}

// What runs behind the tile kernel on the launch group's lane: first the kernel that makes the outputs from the z-surface
// (Post), then -- scene planes in effect (include/rtuf.h, SCENE PLANES) -- the kernel that adds the scene's verdict to those
// outputs (scene), then the kernels that read the mask bits (Tail).
enum class Post { None, Compare, Dilate, Pad };
constexpr int kPosts = 4;
enum class Tail { None, Cloud, Clearance, Points };
constexpr int kTails = 4;

// ok == false: a combination the API refuses.  scene (last: older brace lists leave it false): scene_apply_planes_kernel behind
// a Filter batch's outputs, scene_apply_bits_kernel behind the mask bits of a Bits, Cloud or Clearance batch.
struct Route { TileVariant tile; Post post; Tail tail; bool ok; bool scene; };
constexpr bool runs_behind_tile(const Route& r) { return r.post != Post::None || r.tail != Tail::None || r.scene; }
constexpr int route_index(const Route& r)
{
  return tile_variant_index(r.tile) + kTileVariantSlots * ((int)r.post + kPosts * ((int)r.tail + kTails * (r.scene ? 1 : 0)));
}

// The facts a route follows from.
struct RouteFacts {
  BatchKind kind;
  bool u16;           // 16UC1 planes
  bool labels;        // the caller asked for a label plane
  bool thresh;        // per-link thresholds are in effect in the context (some model has thresholds of its own)
  bool two_kernel;    // the context's RTUF_FLAG_TWO_KERNEL
  int dilation;       // the context's silhouette dilation radius
  bool cover;         // the cover pass is on
  // padded: link padding is in effect in the context (some model holds a non-zero padding).  scene: scene planes are in effect in
  // the context (some stream has scene filtering enabled).  The two newest facts, scene last: older brace lists leave them false.
  bool padded; bool scene;
};

//   batch                                      tile output   modifiers              behind it
//   Filter                                     Planes        labels, thresh, u16    -
//   Filter, two-kernel flag                    ZSurface      labels                 Compare
//   Filter / Bits / Cloud / Clearance, dilated ZSurface      -                      Dilate (then Cloud / Clearance)
//   Filter / Bits / Cloud / Clearance, padded  ZSurface      labels (link slots)    Pad (then Cloud / Clearance)
//   Bits                                       Bits          thresh, u16            -
//   Render                                     Render        labels, u16            -
//   Residual                                   Residual      thresh, u16            -
//   Cloud                                      Bits          thresh, u16            Cloud
//   Clearance                                  Bits          thresh, u16            Clearance
//   Points                                     Render        -                      Points
// The two-kernel flag is for full planes: the mask-bits calls refuse it, the other kinds run as if it were not set.
// Thresholds do not enter a render batch.  Refused: a label plane beside anything but a filter or render batch, or with
// dilation; dilation with a render or residual batch; thresholds on the z-surface route.  Link padding goes over the
// z-surface whatever the two-kernel flag says, and the plane beside it belongs to the link slots: refused with a label plane,
// a render or residual batch, dilation or thresholds.
// Scene planes refuse nothing and change nothing in front of them: a Filter, Bits, Cloud or Clearance batch takes the route it
// would take without, plus the scene stage between Post and Tail; render and residual batches compare nothing against the scene.
// A point list batch (include/rtuf.h, POINT LIST BATCHES) is a render batch into a float plane of the library's with the points
// kernel behind it, whatever the other facts say: the two-kernel flag and the scene do not enter, and dilation, padding and
// thresholds are refused (they are not honoured yet).
constexpr Route route_of(const RouteFacts& f)
{
  const bool filter = f.kind == BatchKind::Filter, bits = f.kind == BatchKind::Bits;
  const bool render = f.kind == BatchKind::Render, residual = f.kind == BatchKind::Residual;
  if (f.kind == BatchKind::Points) {
    Route p{};
    p.tile = TileVariant{TileOut::Render, false, false, false, f.cover};
    p.post = Post::None;
    p.tail = Tail::Points;
    p.ok = !f.labels && f.dilation <= 0 && !f.padded && !f.thresh;
    p.scene = false;
    return p;
  }
  const bool dilated = f.dilation > 0, two = f.two_kernel && filter, thresh = f.thresh && !render;
  bool ok = !(f.labels && !filter && !render) && !(dilated && (f.labels || render || residual)) && !(f.two_kernel && bits);
  Route r{};
  if (f.padded) {
    ok = ok && !f.labels && !render && !residual && !dilated && !f.thresh;
    r.tile = TileVariant{TileOut::ZSurface, true, false, false, f.cover};
    r.post = Post::Pad;
  } else if (dilated || two) {
    ok = ok && !thresh;
    r.tile = TileVariant{TileOut::ZSurface, f.labels, false, false, f.cover};
    r.post = dilated ? Post::Dilate : Post::Compare;
  } else {
    const TileOut out = filter ? TileOut::Planes : render ? TileOut::Render : residual ? TileOut::Residual : TileOut::Bits;
    r.tile = TileVariant{out, f.labels, thresh, f.u16, f.cover};
    r.post = Post::None;
  }
  r.tail = f.kind == BatchKind::Cloud ? Tail::Cloud : f.kind == BatchKind::Clearance ? Tail::Clearance : Tail::None;
  r.ok = ok && tile_variant_legal(r.tile);
  r.scene = f.scene && !render && !residual;
  return r;
}

}  // namespace rtuf
