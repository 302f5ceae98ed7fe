/* CPU check of the kernel routes (realtime_urdf_filter_amd/csrc/rtuf_routes.h), the product's own route_of and
 * tile_variant_legal, over every combination of route_of's inputs: 6 kinds x u16 x label plane x thresholds x two-kernel flag x
 * dilation 0 / > 0 x cover pass = 384.
 *   1. route_of agrees with kRows below: one row per class of combinations, written out from what the host API and the tile
 *      launcher did before there was a header -- which call's check refuses a combination, and otherwise which kernel the
 *      launcher's chain of tests came to.  Every combination falls into exactly one row.
 *   2. every route that is ok has a legal tile variant; a refused combination is not ok.
 *   3. the variants the routes reach, the variants tile_variant_legal admits, and kKernels below -- the 22 instantiations of
 *      the six wrapper kernels the launcher has always named, each with and without the cover code -- are one and the same set:
 *      44 variants, 88 kernels with the two workgroup sizes.
 *   4. tile_variant_index and route_index tell distinct variants and routes apart.
 * g++ -O2 -I realtime_urdf_filter_amd/csrc;  prints "ok <combinations> <variants> <kernels>" or the first failure. */
#include <stdio.h>

#include <set>

#include "rtuf_routes.h"

using namespace rtuf;

namespace {

enum { No = 0, Yes = 1, Any = -1 };
enum { Refused = 0, Ok = 1 };
constexpr BatchKind Filter = BatchKind::Filter, Bits = BatchKind::Bits, Render = BatchKind::Render, Residual = BatchKind::Residual,
                    Cloud = BatchKind::Cloud, Clearance = BatchKind::Clearance;

// A class of combinations (u16 and the cover pass never decide; Any: either) and what becomes of it.  For a row that is Ok:
// the tile kernel's output, whether the variant takes over the label plane / the thresholds / 16UC1 from the inputs (No: the
// variant has it off whatever the input says), and what runs behind the tile kernel.
struct Row {
  BatchKind kind; int labels, thresh, two_kernel, dilated;
  int ok; TileOut out; int keeps_labels, keeps_thresh, keeps_u16; Post post; Tail tail;
  const char* why;
};
constexpr TileOut kNoOut = TileOut::Planes;
const Row kRows[] = {
  // full planes: fused; the flag sends them over the z-surface to compare_kernel, a radius to dilate_compare_kernel
  {Filter, Any, Any, No, No,      Ok, TileOut::Planes, Yes, Yes, Yes, Post::None, Tail::None, "tile_kernel / tile_labels_kernel / tile_thresh_kernel"},
  {Filter, Any, No, Yes, No,      Ok, TileOut::ZSurface, Yes, No, No, Post::Compare, Tail::None, "tile_kernel<true> / tile_labels_kernel<true>"},
  {Filter, Any, Yes, Yes, No,     Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_thresh_route: thresholds with the two-kernel flag"},
  {Filter, No, No, Any, Yes,      Ok, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::None, "tile_kernel<true>"},
  {Filter, No, Yes, Any, Yes,     Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_thresh_route: thresholds with dilation"},
  {Filter, Yes, Any, Any, Yes,    Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_labels_call: labels with dilation"},
  // mask bits: fused only
  {Bits, Yes, Any, Any, Any,      Refused, kNoOut, No, No, No, Post::None, Tail::None, "no mask-bits call takes a label plane"},
  {Bits, No, Any, Yes, Any,       Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_bits_call: the two-kernel flag"},
  {Bits, No, Any, No, No,         Ok, TileOut::Bits, No, Yes, Yes, Post::None, Tail::None, "tile_bits_kernel / tile_thresh_kernel<BITS>"},
  {Bits, No, No, No, Yes,         Ok, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::None, "tile_kernel<true>"},
  {Bits, No, Yes, No, Yes,        Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_thresh_route: thresholds with dilation"},
  // virtual depth: neither thresholds nor the flag enter
  {Render, Any, Any, Any, Yes,    Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_render_call: dilation"},
  {Render, Any, Any, Any, No,     Ok, TileOut::Render, Yes, No, Yes, Post::None, Tail::None, "tile_render_kernel"},
  // residual tables: thresholds are honoured, the flag does not enter
  {Residual, Yes, Any, Any, Any,  Refused, kNoOut, No, No, No, Post::None, Tail::None, "no residual call takes a label plane"},
  {Residual, No, Any, Any, Yes,   Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_residuals_call: dilation"},
  {Residual, No, Any, Any, No,    Ok, TileOut::Residual, No, Yes, Yes, Post::None, Tail::None, "tile_resid_kernel"},
  // clouds and clearance tables: a mask-bits batch (the flag does not enter) with their kernels behind it
  {Cloud, Yes, Any, Any, Any,     Refused, kNoOut, No, No, No, Post::None, Tail::None, "no cloud call takes a label plane"},
  {Cloud, No, Any, Any, No,       Ok, TileOut::Bits, No, Yes, Yes, Post::None, Tail::Cloud, "tile_bits_kernel / tile_thresh_kernel<BITS>"},
  {Cloud, No, No, Any, Yes,       Ok, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::Cloud, "tile_kernel<true>"},
  {Cloud, No, Yes, Any, Yes,      Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_cloud_call: thresholds with dilation"},
  {Clearance, Yes, Any, Any, Any, Refused, kNoOut, No, No, No, Post::None, Tail::None, "no clearance call takes a label plane"},
  {Clearance, No, Any, Any, No,   Ok, TileOut::Bits, No, Yes, Yes, Post::None, Tail::Clearance, "tile_bits_kernel / tile_thresh_kernel<BITS>"},
  {Clearance, No, No, Any, Yes,   Ok, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::Clearance, "tile_kernel<true>"},
  {Clearance, No, Yes, Any, Yes,  Refused, kNoOut, No, No, No, Post::None, Tail::None, "check_clearance_call: thresholds with dilation"},
};

// The instantiations the tile launcher names, without the COVER and NT arguments every one of them has besides.
struct Kernel { const char* name; TileOut out; bool labels, thresh, u16; };
const Kernel kKernels[] = {
  {"tile_kernel<false, false>", TileOut::Planes, false, false, false},
  {"tile_kernel<false, true>", TileOut::Planes, false, false, true},
  {"tile_kernel<true, false>", TileOut::ZSurface, false, false, false},
  {"tile_bits_kernel<false>", TileOut::Bits, false, false, false},
  {"tile_bits_kernel<true>", TileOut::Bits, false, false, true},
  {"tile_labels_kernel<false, false>", TileOut::Planes, true, false, false},
  {"tile_labels_kernel<false, true>", TileOut::Planes, true, false, true},
  {"tile_labels_kernel<true, false>", TileOut::ZSurface, true, false, false},
  {"tile_thresh_kernel<false, false, false>", TileOut::Planes, false, true, false},      // <U16, BITS, LABELS>
  {"tile_thresh_kernel<true, false, false>", TileOut::Planes, false, true, true},
  {"tile_thresh_kernel<false, true, false>", TileOut::Bits, false, true, false},
  {"tile_thresh_kernel<true, true, false>", TileOut::Bits, false, true, true},
  {"tile_thresh_kernel<false, false, true>", TileOut::Planes, true, true, false},
  {"tile_thresh_kernel<true, false, true>", TileOut::Planes, true, true, true},
  {"tile_render_kernel<false, false>", TileOut::Render, false, false, false},            // <U16, LABELS>
  {"tile_render_kernel<true, false>", TileOut::Render, false, false, true},
  {"tile_render_kernel<false, true>", TileOut::Render, true, false, false},
  {"tile_render_kernel<true, true>", TileOut::Render, true, false, true},
  {"tile_resid_kernel<false, false>", TileOut::Residual, false, false, false},           // <U16, THRESH>
  {"tile_resid_kernel<true, false>", TileOut::Residual, false, false, true},
  {"tile_resid_kernel<false, true>", TileOut::Residual, false, true, false},
  {"tile_resid_kernel<true, true>", TileOut::Residual, false, true, true},
};
constexpr int kWorkgroupSizes = 2;       // 256 and 1,024 threads: launch_tile picks by the launch's size, not by the route

bool matches(int want, bool have) { return want == Any || (want == Yes) == have; }

}  // namespace

int main()
{
  const BatchKind kinds[] = {Filter, Bits, Render, Residual, Cloud, Clearance};
  std::set<int> reached, legal, named, routes;
  int combinations = 0;
  for (BatchKind kind : kinds)
    for (int m = 0; m < 64; m++) {
      const bool u16 = m & 1, labels = m & 2, thresh = m & 4, two = m & 8, dilated = m & 16, cover = m & 32;
      const RouteFacts f = {kind, u16, labels, thresh, two, dilated ? 3 : 0, cover};
      const Route r = route_of(f);
      const Row* row = nullptr;
      int hits = 0;
      for (const Row& q : kRows)
        if (q.kind == kind && matches(q.labels, labels) && matches(q.thresh, thresh) && matches(q.two_kernel, two) && matches(q.dilated, dilated)) { row = &q; hits++; }
      auto fail = [&](const char* what) {
        printf("kind %d u16 %d labels %d thresh %d two_kernel %d dilated %d cover %d: %s (%s)\n", (int)kind, u16, labels, thresh, two, dilated, cover, what, row ? row->why : "-");
        return 1;
      };
      if (hits != 1) return fail("not in exactly one row of the table");
      if (r.ok != (row->ok == Ok)) return fail(row->ok == Ok ? "refused, but the table admits it" : "admitted, but the table refuses it");
      combinations++;
      if (!r.ok) continue;
      if (!tile_variant_legal(r.tile)) return fail("an ok route with an illegal tile variant");
      if (r.tile.out != row->out) return fail("tile output");
      if (r.tile.labels != (row->keeps_labels == Yes && labels)) return fail("tile labels");
      if (r.tile.thresh != (row->keeps_thresh == Yes && thresh)) return fail("tile thresh");
      if (r.tile.u16 != (row->keeps_u16 == Yes && u16)) return fail("tile u16");
      if (r.tile.cover != cover) return fail("tile cover");
      if (r.post != row->post) return fail("post");
      if (r.tail != row->tail) return fail("tail");
      if (runs_behind_tile(r) != (row->post != Post::None || row->tail != Tail::None)) return fail("runs_behind_tile");
      reached.insert(tile_variant_index(r.tile));
      routes.insert(route_index(r));
    }
  // every variant there could be: which are legal, and do their numbers differ
  std::set<int> all;
  for (int out = 0; out < kTileOuts; out++)
    for (int m = 0; m < 16; m++) {
      const TileVariant v = {(TileOut)out, (m & 8) != 0, (m & 4) != 0, (m & 2) != 0, (m & 1) != 0};
      const int i = tile_variant_index(v);
      if (i < 0 || i >= kTileVariantSlots || !all.insert(i).second) { printf("tile_variant_index %d: out of range or taken twice\n", i); return 1; }
      if (tile_variant_legal(v)) legal.insert(i);
    }
  for (const Kernel& k : kKernels)
    for (int cover = 0; cover < 2; cover++) {
      const TileVariant v = {k.out, k.labels, k.thresh, k.u16, cover != 0};
      if (!tile_variant_legal(v)) { printf("%s: not a legal variant\n", k.name); return 1; }
      if (!named.insert(tile_variant_index(v)).second) { printf("%s: a second kernel for one variant\n", k.name); return 1; }
    }
  if (named.size() != 44) { printf("%d named variants, not 44\n", (int)named.size()); return 1; }
  if (reached != named) { printf("the routes reach %d variants, the launcher names %d: not the same set\n", (int)reached.size(), (int)named.size()); return 1; }
  if (legal != named) { printf("%d legal variants, the launcher names %d: not the same set\n", (int)legal.size(), (int)named.size()); return 1; }
  // routes that differ in anything differ in route_index: with nothing behind the tile kernel 8 plane, 4 bits, 4 render and 4
  // residual variants; the z-surface with and without labels before compare, without before dilate and each of the 3 tails;
  // the 4 bits variants before the cloud and the clearance kernels -- all with and without the cover pass
  if (routes.size() != 2 * (20 + 2 + 3 + 8)) { printf("%d distinct route numbers\n", (int)routes.size()); return 1; }
  printf("ok %d %d %d\n", combinations, (int)named.size(), (int)named.size() * kWorkgroupSizes);
  return 0;
}
