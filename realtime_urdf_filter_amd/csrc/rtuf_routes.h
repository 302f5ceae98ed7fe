// rtuf_routes.h -- which kernels a batch runs: the tile kernel's variant, and what runs behind it on the group's lane.
//
// The one place that decides it, and that refuses what has no route.  Every batch call of rtuf_api.cpp asks route_of through
// check_route, once its own arguments are in order, and returns the reason's message if there is one (enum class Refusal
// below); enqueue_batch asks route_of of the same facts once, when a batch is first enqueued, keeps the Route with the batch
// slot (re-runs take it from there) and hands it to issue_plan; launch_tile (rtuf_kernels.hip) maps its TileVariant to a kernel
// instantiation, and tile_body asserts that the instantiation is a legal one.  A new batch kind, a new variant of the tile
// kernel, or a new refusal starts here.
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

// Why a combination has no route: the API refuses it with this reason's message (check_route in rtuf_api.cpp, which holds the
// texts), before the call builds, allocates or enqueues anything.  route_of names the first reason that applies, per kind in
// this order -- the order in which the calls have always named them (L: a label plane is asked for, T: per-link thresholds are
// in effect, K: the two-kernel flag, D: dilation > 0, P: link padding is in effect):
//   Filter            L&D LabelsDilation, L&P LabelsPadding, P&D DilationPadding, P&T ThreshPadding, T&(K or D) ThreshZSurface
//   Bits (learn-scene too)   L NoLabelPlane, K BitsTwoKernel, P&D DilationPadding, P&T ThreshPadding, T&D ThreshZSurface
//   Render            D RenderDilation, L&P LabelsPadding, P RenderPadding
//   Residual          L NoLabelPlane, D ResidualDilation, P ResidualPadding
//   Cloud, Clearance  L NoLabelPlane, T&D ThreshDilation, P&D DilationPadding, P&T ThreshPadding
//   Points            L NoLabelPlane, D PointsDilation, P PointsPadding, T PointsThresh
// In words: a label plane goes with a filter or render batch only (NoLabelPlane: no call of the other kinds has the argument;
// the reason keeps route_of total), and not with dilation; dilation not with a render or residual batch; thresholds not on the
// z-surface route, which does not carry the winning link (ThreshZSurface and ThreshDilation are one rule with the two texts
// the calls have for it); the mask-bits calls refuse the two-kernel flag, which is for full planes; with link padding the
// plane beside the z-surface belongs to the link slots, so no label plane, render or residual batch, dilation or thresholds;
// a point list batch honours neither dilation nor padding nor thresholds yet.
// A call that is wrong in several ways at once, only one of them a refusal of this list, reports whichever of its checks comes
// first: the refusal behind the checks of the call's own arguments (the models are final, n, null arrays, n_labels, capacity,
// radius_px, max_distance, the width rules), before any check of what the context holds (a stream without cloud intrinsics, a
// label the table has no row for) and before the alignment of device buffers and the single planes of a host form are looked at.
enum class Refusal {
  None, NoLabelPlane, LabelsDilation, LabelsPadding, RenderDilation, RenderPadding, ResidualDilation, ResidualPadding, DilationPadding,
  ThreshPadding, ThreshZSurface, ThreshDilation, BitsTwoKernel, PointsDilation, PointsPadding, PointsThresh
};

// why != None: a combination the API refuses; the rest of the route is then what it would be, and nothing runs it.  scene (last:
// older brace lists leave it false): scene_apply_planes_kernel behind a Filter batch's outputs, scene_apply_bits_kernel behind
// the mask bits of a Bits, Cloud or Clearance batch.
struct Route {
  TileVariant tile; Post post; Tail tail; Refusal why; bool scene;
  constexpr bool ok() const { return why == Refusal::None; }
};
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
// The two-kernel flag is for full planes: the other kinds run as if it were not set.  Thresholds do not enter a render batch.
// Link padding goes over the z-surface whatever the two-kernel flag says, and the plane beside it belongs to the link slots.
// Scene planes refuse nothing and change nothing in front of them: a Filter, Bits, Cloud or Clearance batch takes the route it
// would take without, plus the scene stage between Post and Tail; render and residual batches compare nothing against the scene.
// A point list batch (include/rtuf.h, POINT LIST BATCHES) is a render batch into a float plane of the library's with the points
// kernel behind it, whatever the other facts say: the two-kernel flag and the scene do not enter.
// What is refused, and in which order the reasons are named: enum class Refusal above.
constexpr Route route_of(const RouteFacts& f)
{
  using R = Refusal;
  const bool filter = f.kind == BatchKind::Filter, render = f.kind == BatchKind::Render, residual = f.kind == BatchKind::Residual;
  const bool L = f.labels, T = f.thresh, K = f.two_kernel, D = f.dilation > 0, P = f.padded;
  R why = R::None;
  switch (f.kind) {
    case BatchKind::Filter:
      why = L && D ? R::LabelsDilation : L && P ? R::LabelsPadding : P && D ? R::DilationPadding : P && T ? R::ThreshPadding : T && (K || D) ? R::ThreshZSurface : R::None;
      break;
    case BatchKind::Bits:
      why = L ? R::NoLabelPlane : K ? R::BitsTwoKernel : P && D ? R::DilationPadding : P && T ? R::ThreshPadding : T && D ? R::ThreshZSurface : R::None;
      break;
    case BatchKind::Render: why = D ? R::RenderDilation : L && P ? R::LabelsPadding : P ? R::RenderPadding : R::None; break;
    case BatchKind::Residual: why = L ? R::NoLabelPlane : D ? R::ResidualDilation : P ? R::ResidualPadding : R::None; break;
    case BatchKind::Cloud:
    case BatchKind::Clearance:
      why = L ? R::NoLabelPlane : T && D ? R::ThreshDilation : P && D ? R::DilationPadding : P && T ? R::ThreshPadding : R::None;
      break;
    case BatchKind::Points: why = L ? R::NoLabelPlane : D ? R::PointsDilation : P ? R::PointsPadding : T ? R::PointsThresh : R::None; break;
  }
  Route r{};
  r.why = why;
  if (f.kind == BatchKind::Points) {
    r.tile = TileVariant{TileOut::Render, false, false, false, f.cover};
    r.post = Post::None;
    r.tail = Tail::Points;
    r.scene = false;
    return r;
  }
  if (P) {
    r.tile = TileVariant{TileOut::ZSurface, true, false, false, f.cover};
    r.post = Post::Pad;
  } else if (D || (K && filter)) {
    r.tile = TileVariant{TileOut::ZSurface, L, false, false, f.cover};
    r.post = D ? Post::Dilate : Post::Compare;
  } else {
    const TileOut out = filter ? TileOut::Planes : render ? TileOut::Render : residual ? TileOut::Residual : TileOut::Bits;
    r.tile = TileVariant{out, L, T && !render, f.u16, f.cover};
    r.post = Post::None;
  }
  r.tail = f.kind == BatchKind::Cloud ? Tail::Cloud : f.kind == BatchKind::Clearance ? Tail::Clearance : Tail::None;
  r.scene = f.scene && !render && !residual;
  return r;
}

}  // namespace rtuf
